"""What genomic regions cost run_mcmc: the same E-step timed in alternation without regions, with 24 and with 1000
equal regions, in one process, on the layout bench.py uses on one GPU (a LocalGroup of 3 contexts on tree.nwk, 2 on
the 16-leaf tree).  Regions add, per context and sweep, a small guard launch before and after each colour phase and
one after the statistics pass (epv_regions.h); the colour-phase kernels are the ones of the "off" leg.
The "off" leg launches what a build without the feature launches: it is the yardstick of the session.
Prints the medians and the spread, and writes them to profiles/regions_overhead.txt (--out FILE for another place,
--out '' for none).

  python tools/regions_overhead.py [--repeats 7] [--n 1000000] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epievo_amd import host  # noqa: E402
from epievo_amd.parallel import LocalGroup  # noqa: E402
from epievo_amd.workloads import config, ref_test_model  # noqa: E402

BURN_IN, BATCH = 10, 50
LEGS = (("off", 0), ("24 regions", 24), ("1000 regions", 1000))


def equal_regions(n, k):
    return [n // k + (1 if j < n % k else 0) for j in range(k)]


def one(cfg, n, repeats, shards, say):
    model, tree = ref_test_model(), config(cfg)
    fp = host.simulate(model, tree, n, 42)
    cap = int(max(16, 2 * fp.counts().max() + 8))
    runs = {}
    for leg, k in LEGS:
        g = LocalGroup(0, shards, BURN_IN + BATCH)
        g.set_tree(tree)
        g.set_model(model)
        g.upload_paths(fp, cap)
        if k:
            g.set_regions(equal_regions(n, k))
        g.reset()
        assert g.fixed_sites() == (2 * k - 2 if k else 0)
        g.run_mcmc(BURN_IN, BATCH, 42, 0)        # warm-up
        runs[leg] = [g, []]
    for r in range(repeats):
        for leg, _ in LEGS:
            g, ts = runs[leg]
            g.reset()
            t0 = time.perf_counter()
            g.run_mcmc(BURN_IN, BATCH, 42, (r + 1) * (BURN_IN + BATCH))
            ts.append(time.perf_counter() - t0)
    med = {leg: statistics.median(runs[leg][1]) for leg, _ in LEGS}
    say("%-6s n=%d contexts=%d -L %d -B %d, %d repeats each, run_mcmc:" % (cfg, n, len(runs["off"][0].subs), BURN_IN,
                                                                           BATCH, repeats))
    for leg, _ in LEGS:
        ts = runs[leg][1]
        say("  %-16s median %9.2f ms (min %9.2f, max %9.2f)  %+6.1f %% over off"
            % (leg, med[leg] * 1e3, min(ts) * 1e3, max(ts) * 1e3, 100.0 * (med[leg] / med["off"] - 1.0)))
    for g, _ in runs.values():
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_overhead.txt"),
                    help="file the lines are written to (an empty string: none)")
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    one("tree", a.n, a.repeats, 3, say)
    one("bal16", a.n, a.repeats, 2, say)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
