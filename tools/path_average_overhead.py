"""What the on-device path average costs run_mcmc: the same E-step timed in alternation with
averaging off and with P points, in one process, on the layout bench.py uses on one GPU (a
LocalGroup of 3 contexts on tree.nwk, 2 on the 16-leaf tree).  Prints the medians and the spread.

  python tools/path_average_overhead.py [--repeats 7] [--points 100] [--n 1000000]
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
    runs = {}
    for mode in ("off", "on"):
        g = LocalGroup(0, shards, BURN_IN + BATCH)
        g.set_tree(tree)
        g.set_model(model)
        g.upload_paths(fp, cap)
        g.reset()
        if mode == "on":
            g.enable_path_average(P)
        g.run_mcmc(BURN_IN, BATCH, 42, 0)        # warm-up
        runs[mode] = [g, []]
    for r in range(repeats):
        for mode in ("off", "on"):
            g, ts = runs[mode]
            g.reset()
            t0 = time.perf_counter()
            g.run_mcmc(BURN_IN, BATCH, 42, (r + 1) * (BURN_IN + BATCH))
            ts.append(time.perf_counter() - t0)
    ns, _ = runs["on"][0].path_average(counts=True)
    assert ns == (repeats + 1) * BATCH
    off, on = runs["off"][1], runs["on"][1]
    mo, mn = statistics.median(off), statistics.median(on)
    print("%-6s n=%d contexts=%d P=%d -L %d -B %d: run_mcmc off median %.2f ms (min %.2f, max %.2f), "
          "on median %.2f ms (min %.2f, max %.2f), overhead %+.1f %% (%d repeats each)"
          % (cfg, n, len(runs["on"][0].subs), P, BURN_IN, BATCH, mo * 1e3, min(off) * 1e3, max(off) * 1e3,
             mn * 1e3, min(on) * 1e3, max(on) * 1e3, 100.0 * (mn / mo - 1.0), repeats))
    for g, _ in runs.values():
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--n", type=int, default=1000000)
    a = ap.parse_args()
    one("tree", a.n, a.points, a.repeats, 3)
    one("bal16", a.n, a.points, a.repeats, 2)


if __name__ == "__main__":
    main()
