"""What the on-device change tracts cost run_mcmc: the same E-step timed in alternation with every accumulator off,
with the change tracts on, with the domain turnover on, and with the branch events on, in one process, on the layout
bench.py uses on one GPU (a LocalGroup of 3 contexts on tree.nwk, 2 on the 16-leaf tree).
The "off" leg runs the kernels of a build without the accumulator: it is the yardstick of the session; the
"turnover" leg is there for comparison (the two layers share the pack launch shape; the tracts scan B rows with a
wider carry where the turnover scans 2 B).
Prints the medians and the spread, and writes them to profiles/change_tracts_overhead.txt (--out FILE for another
place, --out '' for none).

  python tools/change_tracts_overhead.py [--repeats 7] [--n 1000000] [--out FILE]
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
LEGS = ("off", "tracts", "turnover", "events")


def one(cfg, n, repeats, shards, say):
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
        if leg == "events":
            g.enable_branch_events()
        if leg == "turnover":
            g.enable_domain_turnover(BATCH)
        if leg == "tracts":
            g.enable_change_tracts(BATCH)
        g.run_mcmc(BURN_IN, BATCH, 42, 0)        # warm-up
        runs[leg] = [g, []]
    for r in range(repeats):
        for leg in LEGS:
            g, ts = runs[leg]
            g.reset()
            if leg == "turnover":
                g.reset_domain_turnover()        # (the edge records hold one batch; outside the timed part)
            if leg == "tracts":
                g.reset_change_tracts()
            t0 = time.perf_counter()
            g.run_mcmc(BURN_IN, BATCH, 42, (r + 1) * (BURN_IN + BATCH))
            ts.append(time.perf_counter() - t0)
    assert runs["events"][0].branch_events_samples() == (repeats + 1) * BATCH
    assert runs["turnover"][0].domain_turnover_samples() == BATCH
    assert runs["tracts"][0].change_tracts_samples() == BATCH
    ns, hist, len_sum = runs["tracts"][0].change_tracts()
    assert ns == BATCH and hist.any() and (hist.sum(axis=2) <= len_sum).all()
    med = {leg: statistics.median(runs[leg][1]) for leg in LEGS}
    say("%-6s n=%d contexts=%d -L %d -B %d, %d repeats each, run_mcmc:" % (cfg, n, len(runs["off"][0].subs), BURN_IN,
                                                                           BATCH, repeats))
    for leg in LEGS:
        ts = runs[leg][1]
        say("  %-16s median %9.2f ms (min %9.2f, max %9.2f)  %+6.1f %% over off"
            % (leg, med[leg] * 1e3, min(ts) * 1e3, max(ts) * 1e3, 100.0 * (med[leg] / med["off"] - 1.0)))
    say("  tracts' increment over off / turnover's increment over off: %.2f (rows scanned: %d against %d)"
        % ((med["tracts"] - med["off"]) / (med["turnover"] - med["off"]), tree.n_nodes - 1, 2 * (tree.n_nodes - 1)))
    for g, _ in runs.values():
        g.close()


def chunk_words():
    from epievo_amd.sampler import DeviceSampler
    model, tree = ref_test_model(), config("tree")
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(host.simulate(model, tree, 64, 1), 16)
    d.enable_change_tracts(1)
    words = d.change_tracts_layout()[5] // 64
    d.close()
    return words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "change_tracts_overhead.txt"),
                    help="file the lines are written to (an empty string: none)")
    a = ap.parse_args()
    lines = ["EPV_DOM_CHUNK_WORDS = %d (sites per block of the tract kernel / 64; the turnover's, reused unmeasured)"
             % chunk_words()]
    print(lines[0], flush=True)

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
