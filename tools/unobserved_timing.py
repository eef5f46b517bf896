"""Cost of missing leaf data in the E-step: the config-3 shape (tree.nwk, n = 1e6, -L 10 -B 50) through the
C++ driver (the CLIs' code path), default vs a fraction of the leaf cells unobserved (epvd_set_unobserved).
One JSON line per case: ms per MCMC step (burn-in + batch sweeps of run_mcmc) and the phase mode.

  python tools/unobserved_timing.py [--n 1000000] [--frac 0.1] [--steps 3] [--cases default,unobs] [--out F]
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
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--burn", type=int, default=10)
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--cases", default="default,unobs")
ap.add_argument("--out", default="")
a = ap.parse_args()

model, tree, fp = simulate("tree", a.n, seed=1)
B, n = tree.n_nodes - 1, fp.n_sites
rng = np.random.default_rng(3)
mask = np.zeros((B, n), np.uint8)
for b in range(1, tree.n_nodes):
    if tree.subtree_sizes[b] == 1:
        mask[b - 1] = rng.random(n) < a.frac
lines = []
for case in a.cases.split(","):
    s = driver.CppSampler(a.burn, a.batch, devices=[0])
    if case == "unobs":
        s.set_unobserved(mask)
    s.reset(model, tree, fp)
    s.run_mcmc(5, 0)                       # warm-up: allocations, first launches
    t0 = time.perf_counter()
    for it in range(1, a.steps + 1):
        s.reset(model)
        J, D, acc = s.run_mcmc(5, it)
    dt = (time.perf_counter() - t0) / a.steps
    sweeps = a.burn + a.batch
    rec = {"case": case, "n_sites": n, "unobserved_cells": int(mask.sum()) if case == "unobs" else 0,
           "leaf_cells": int(sum(n for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1)),
           "phase_mode": s.phase_mode(), "layout": s.layout()["text"], "ms_per_step": dt * 1e3,
           "site_updates_per_s": sweeps * (n - 2) / dt, "acc_rate": acc}
    s.close()
    print(json.dumps(rec), flush=True)
    lines.append(rec)
if a.out:
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
