"""What the epoch statistics cost run_mcmc: the same E-step timed in alternation with every accumulator off, with
the epoch statistics on at P = 100 and at P = 8, with the window statistics on at W = 1000 and with the path
average on at P = 100 (the other per-branch time-grid accumulator), in one process, on the layout bench.py uses on
one GPU (a LocalGroup of 3 contexts on tree.nwk, 2 on the 16-leaf tree).
The "off" leg runs the kernels of a build without the accumulator: it is the yardstick of the session, the two
sibling legs are the others.  Prints the medians and the spread.

  python tools/epoch_stats_overhead.py [--repeats 7] [--n 1000000]
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
LEGS = ("off", "epochs P=100", "epochs P=8", "wstat W=1000", "pavg P=100")


def one(cfg, n, repeats, shards):
    model, tree = ref_test_model(), config(cfg)
    fp = host.simulate(model, tree, n, 42)
    cap = int(max(16, 2 * fp.counts().max() + 8))
    runs = {}
    for leg in LEGS:
        g = LocalGroup(0, shards, BURN_IN + BATCH)
        g.set_tree(tree)
        g.set_model(model)
        g.upload_paths(fp, cap)
        g.reset()
        arg = int(leg.split("=")[1]) if "=" in leg else 0
        if leg.startswith("epochs"):
            g.enable_epoch_stats(arg)
        if leg.startswith("wstat"):
            g.enable_window_stats(arg)
        if leg.startswith("pavg"):
            g.enable_path_average(arg)
        g.run_mcmc(BURN_IN, BATCH, 42, 0)        # warm-up
        runs[leg] = [g, []]
    for r in range(repeats):
        for leg in LEGS:
            g, ts = runs[leg]
            g.reset()
            t0 = time.perf_counter()
            g.run_mcmc(BURN_IN, BATCH, 42, (r + 1) * (BURN_IN + BATCH))
            ts.append(time.perf_counter() - t0)
    for leg in LEGS[1:3]:
        assert runs[leg][0].epoch_stats_samples() == (repeats + 1) * BATCH
    assert runs["wstat W=1000"][0].window_stats_samples() == (repeats + 1) * BATCH
    med = {leg: statistics.median(runs[leg][1]) for leg in LEGS}
    print("%-6s n=%d contexts=%d -L %d -B %d, %d repeats each, run_mcmc:" % (cfg, n, len(runs["off"][0].subs), BURN_IN,
                                                                             BATCH, repeats))
    for leg in LEGS:
        ts = runs[leg][1]
        print("  %-16s median %9.2f ms (min %9.2f, max %9.2f)  %+6.1f %% over off"
              % (leg, med[leg] * 1e3, min(ts) * 1e3, max(ts) * 1e3,
                 100.0 * (med[leg] / med["off"] - 1.0)))
    for g, _ in runs.values():
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
