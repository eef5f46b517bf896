"""What EPV_OPT_LEAF_FAST buys in the E-step, through the C++ driver (the CLIs' code path), on
the config-3 shape (tree.nwk, n = 1e6, -L 10 -B 50) and on the 16-leaf tree at n = 1e6.  Four legs on ONE sampler,
alternating, the median of --rounds rounds each:
  none      no cell held
  mask-v1   a fraction of the leaf cells masked, the option off: the first proposal kernel (the behaviour before)
  mask      the same mask, the option on
  evidence  the same cells as evidence (r uniform in (0.05, 0.95)), the option on
One JSON line per (tree, leg): ms per MCMC step (reset + burn-in + batch sweeps of run_mcmc), min and max over the
rounds and the phase mode; then per tree whether each option-on leg beats mask-v1 by more than the larger (max - min)
of the two legs.

  python tools/leaf_fast_timing.py [--n 1000000] [--frac 0.1] [--rounds 7] [--steps 2] [--trees tree,bal16] [--out F]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epievo_amd import driver  # noqa: E402
from epievo_amd.workloads import simulate  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--frac", type=float, default=0.1)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--burn", type=int, default=10)
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--trees", default="tree,bal16")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "leaf_fast_timing.jsonl"))
a = ap.parse_args()

LEGS = [("none", False, False, False), ("mask-v1", True, False, False), ("mask", True, False, True),
        ("evidence", False, True, True)]          # name, mask held, table held, option on
MODES = ["V1", "V2", "V2 segments", "fused", "V3"]
lines = []
for name in a.trees.split(","):
    model, tree, fp = simulate(name, a.n, seed=1)
    B, n = tree.n_nodes - 1, fp.n_sites
    rng = np.random.default_rng(3)
    mask = np.zeros((B, n), np.uint8)
    for b in range(1, tree.n_nodes):
        if tree.subtree_sizes[b] == 1:
            mask[b - 1] = rng.random(n) < a.frac
    table = np.full((B, n), np.nan, np.float32)
    table[mask != 0] = rng.uniform(0.05, 0.95, int(mask.sum())).astype(np.float32)
    s = driver.CppSampler(a.burn, a.batch, devices=[0])
    s.reset(model, tree, fp)
    times = {leg[0]: [] for leg in LEGS}
    modes, it = {}, 0
    for rnd in range(a.rounds + 1):                 # (round 0 warms every leg up: allocations, first launches)
        for leg, held_mask, held_table, on in LEGS:
            s.set_leaf_fast(on)
            s.set_unobserved(mask if held_mask else None)
            s.set_leaf_evidence(table if held_table else None)
            s.reset(model)
            it += 1
            s.run_mcmc(5, it)                       # untimed: the leg's first step after the switch
            t0 = time.perf_counter()
            for _ in range(a.steps):
                it += 1
                s.reset(model)
                s.run_mcmc(5, it)
            if rnd:
                times[leg].append((time.perf_counter() - t0) / a.steps * 1e3)
            modes[leg] = s.phase_mode()
    layout = s.layout()["text"]
    s.close()
    recs = {}
    for leg, held_mask, held_table, on in LEGS:
        t = sorted(times[leg])
        recs[leg] = {"tree": name, "leg": leg, "n_sites": n, "held_cells": int(mask.sum()) if held_mask or held_table else 0,
                     "leaf_cells": int(sum(n for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1)),
                     "leaf_fast": on, "phase_mode": modes[leg], "phase": MODES[modes[leg]], "layout": layout,
                     "ms_per_step_median": t[len(t) // 2], "ms_per_step_min": t[0], "ms_per_step_max": t[-1],
                     "rounds": a.rounds, "steps_per_round": a.steps, "sweeps_per_step": a.burn + a.batch}
        print(json.dumps(recs[leg]), flush=True)
        lines.append(recs[leg])
    v1 = recs["mask-v1"]
    for leg in ("mask", "evidence"):
        r = recs[leg]
        spread = max(v1["ms_per_step_max"] - v1["ms_per_step_min"], r["ms_per_step_max"] - r["ms_per_step_min"])
        gain = v1["ms_per_step_median"] - r["ms_per_step_median"]
        verdict = {"tree": name, "leg": leg, "against": "mask-v1", "gain_ms": gain, "larger_spread_ms": spread,
                   "beats_v1_beyond_spread": bool(gain > spread),
                   "over_none_ms": r["ms_per_step_median"] - recs["none"]["ms_per_step_median"]}
        print(json.dumps(verdict), flush=True)
        lines.append(verdict)
if a.out:
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
