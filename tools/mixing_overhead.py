"""What the chain mixing diagnostics cost run_mcmc: the same E-step timed in alternation with every layer off, with
the mixing diagnostics at max_lag 1 and 8, and, in the same session for comparison, with the path average and with
the branch events, in one process, on the layout bench.py uses on one GPU (a LocalGroup of 3 contexts on tree.nwk, 2
on the 16-leaf tree).  Prints the medians and the spread.

  python tools/mixing_overhead.py [--repeats 7] [--points 100] [--n 1000000]
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


def one(cfg, n, P, repeats, shards):
    model, tree = ref_test_model(), config(cfg)
    fp = host.simulate(model, tree, n, 42)
    cap = int(max(16, 2 * fp.counts().max() + 8))
    modes = {"off": lambda g: None, "mixing K=1": lambda g: g.enable_mixing(1), "mixing K=8": lambda g: g.enable_mixing(8),
             "path average": lambda g: g.enable_path_average(P), "branch events": lambda g: g.enable_branch_events()}
    runs = {}
    for mode, enable in modes.items():
        g = LocalGroup(0, shards, BURN_IN + BATCH)
        g.set_tree(tree)
        g.set_model(model)
        g.upload_paths(fp, cap)
        g.reset()
        enable(g)
        g.run_mcmc(BURN_IN, BATCH, 42, 0)        # warm-up
        runs[mode] = [g, []]
    for r in range(repeats):
        for mode in modes:
            g, ts = runs[mode]
            g.reset()
            t0 = time.perf_counter()
            g.run_mcmc(BURN_IN, BATCH, 42, (r + 1) * (BURN_IN + BATCH))
            ts.append(time.perf_counter() - t0)
    for mode in ("mixing K=1", "mixing K=8"):
        ns, mp, pairs = runs[mode][0].mixing(counts=True)[:3]
        assert ns == mp == (repeats + 1) * BATCH and int(pairs[1]) == (repeats + 1) * (BATCH - 1)
    mo = statistics.median(runs["off"][1])
    print("%-6s n=%d contexts=%d -L %d -B %d, %d repeats each, run_mcmc:" % (cfg, n, len(runs["off"][0].subs), BURN_IN, BATCH,
                                                                           repeats))
    for mode in modes:
        ts = runs[mode][1]
        m = statistics.median(ts)
        print("  %-14s median %.2f ms (min %.2f, max %.2f)%s"
              % (mode, m * 1e3, min(ts) * 1e3, max(ts) * 1e3, "" if mode == "off" else ", overhead %+.1f %%" % (100.0 * (m / mo - 1.0))))
    for g, _ in runs.values():
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--points", type=int, default=100, help="grid points of the path average")
    ap.add_argument("--n", type=int, default=1000000)
    a = ap.parse_args()
    one("tree", a.n, a.points, a.repeats, 3)
    one("bal16", a.n, a.points, a.repeats, 2)


if __name__ == "__main__":
    main()
