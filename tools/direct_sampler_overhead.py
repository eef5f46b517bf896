"""What the direct end-conditioned sampler (EPV_OPT_DIRECT_SAMPLER) costs run_mcmc: the same E-step
timed in alternation with the default options, with the default options on the separate kernels (EPV_FUSED_PHASE=0:
the like-for-like kernels of plain direct mode, which never takes the fused phase), with the direct sampler, and with
the direct sampler inside the fused phase (EPV_OPT_DIRECT_FUSED: set_direct_sampler(True, fused=True)), in one process,
on the layout bench.py uses on one GPU (a LocalGroup of 3 contexts on tree.nwk, 2 on the 16-leaf tree, where the plan
is the large-tree kernel and the fourth leg runs what the third does).
The "default" leg is the yardstick of the session.  Prints the medians and the spread.

  python tools/direct_sampler_overhead.py [--repeats 7] [--n 1000000]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epievo_amd import host  # noqa: E402
from epievo_amd.parallel import LocalGroup  # noqa: E402
from epievo_amd.workloads import config, ref_test_model  # noqa: E402

BURN_IN, BATCH = 10, 50
# leg -> (environment a context reads when it is created, options)
LEGS = {"default": ({}, {}), "default separate": ({"EPV_FUSED_PHASE": "0"}, {}), "direct": ({}, {"direct_sampler": True}),
        "direct fused": ({}, {"direct_sampler": True, "direct_fused": True})}


def one(cfg, n, repeats, shards):
    model, tree = ref_test_model(), config(cfg)
    fp = host.simulate(model, tree, n, 42)
    cap = int(max(16, 2 * fp.counts().max() + 8))
    runs = {}
    for leg, (env, opts) in LEGS.items():
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            g = LocalGroup(0, shards, BURN_IN + BATCH)
            g.set_tree(tree)
            g.set_model(model)
            g.upload_paths(fp, cap)
            g.set_direct_sampler(bool(opts.get("direct_sampler")), fused=bool(opts.get("direct_fused")))
            g.reset()
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        g.run_mcmc(BURN_IN, BATCH, 42, 0)        # warm-up
        runs[leg] = [g, [], g.phase_mode()]
    for r in range(repeats):
        for leg in LEGS:
            g, ts, _ = runs[leg]
            g.reset()
            t0 = time.perf_counter()
            g.run_mcmc(BURN_IN, BATCH, 42, (r + 1) * (BURN_IN + BATCH))
            ts.append(time.perf_counter() - t0)
    assert sum(s.direct_giveups() for leg in ("direct", "direct fused") for s in runs[leg][0].subs) == 0
    med = {leg: statistics.median(runs[leg][1]) for leg in LEGS}
    print("%-6s n=%d contexts=%d -L %d -B %d, %d repeats each, run_mcmc:" % (cfg, n, len(runs["default"][0].subs), BURN_IN,
                                                                             BATCH, repeats))
    for leg in LEGS:
        ts = runs[leg][1]
        print("  %-17s phase mode %d  median %9.2f ms (min %9.2f, max %9.2f)  x %.3f of default, x %.3f of default separate, "
              "x %.3f of direct" % (leg, runs[leg][2], med[leg] * 1e3, min(ts) * 1e3, max(ts) * 1e3, med[leg] / med["default"],
                                    med[leg] / med["default separate"], med[leg] / med["direct"]))
    spread = max(max(runs[leg][1]) - min(runs[leg][1]) for leg in ("direct", "direct fused"))
    print("  direct - direct fused: %.2f ms; the larger (max - min) of the two legs: %.2f ms"
          % ((med["direct"] - med["direct fused"]) * 1e3, spread * 1e3))
    for g, _, _ in runs.values():
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--n", type=int, default=1000000)
    a = ap.parse_args()
    one("tree", a.n, a.repeats, 3)
    one("bal16", a.n, a.repeats, 2)


if __name__ == "__main__":
    main()
