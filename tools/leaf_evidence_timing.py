"""Cost of leaf evidence in the E-step: the config-3 shape (tree.nwk, n = 1e6, -L 10 -B 50) through the C++
driver (the CLIs' code path).  Four cases: the default, a mask on a fraction of the leaf cells
(epvd_set_unobserved), evidence on the same cells, and evidence on every leaf cell (epvd_set_leaf_evidence).
The cases alternate over the repeats, so that drift of the machine hits all of them alike.  One JSON line
per case and repeat, then one summary line per case (median ms per MCMC step: burn-in + batch sweeps of
run_mcmc) with the ratio to the mask run.

  python tools/leaf_evidence_timing.py [--n 1000000] [--frac 0.1] [--steps 10] [--repeats 7]
                                       [--cases default,mask,evidence,evidence_all] [--out F]
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
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--burn", type=int, default=10)
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--cases", default="default,mask,evidence,evidence_all")
ap.add_argument("--out", default="")
a = ap.parse_args()

model, tree, fp = simulate("tree", a.n, seed=1)
B, n = tree.n_nodes - 1, fp.n_sites
rng = np.random.default_rng(3)
leaf_rows = [b - 1 for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1]
mask = np.zeros((B, n), np.uint8)
for b in leaf_rows:
    mask[b] = rng.random(n) < a.frac
nan = np.float32(np.nan)
# soft values strictly inside (0, 1) on the cells of the mask / on every leaf cell
soft = (0.02 + 0.96 * rng.random((B, n))).astype(np.float32)
evidence = np.where(mask != 0, soft, nan).astype(np.float32)
evidence_all = np.full((B, n), nan, np.float32)
evidence_all[leaf_rows] = soft[leaf_rows]
cells = {"default": 0, "mask": int(mask.sum()), "evidence": int(mask.sum()), "evidence_all": len(leaf_rows) * n}

samplers = {}
for case in a.cases.split(","):
    s = driver.CppSampler(a.burn, a.batch, devices=[0])
    if case == "mask":
        s.set_unobserved(mask)
    elif case == "evidence":
        s.set_leaf_evidence(evidence)
    elif case == "evidence_all":
        s.set_leaf_evidence(evidence_all)
    s.reset(model, tree, fp)
    s.run_mcmc(5, 0)                       # warm-up: allocations, first launches
    samplers[case] = s
lines, it = [], 0
for rep in range(a.repeats):
    for case, s in samplers.items():
        t0 = time.perf_counter()
        for _ in range(a.steps):
            it += 1
            s.reset(model)
            J, D, acc = s.run_mcmc(5, it)
        dt = (time.perf_counter() - t0) / a.steps
        rec = {"case": case, "repeat": rep, "n_sites": n, "cells": cells[case], "leaf_cells": len(leaf_rows) * n,
               "phase_mode": s.phase_mode(), "layout": s.layout()["text"], "ms_per_step": dt * 1e3,
               "site_updates_per_s": (a.burn + a.batch) * (n - 2) / dt, "acc_rate": acc}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
for s in samplers.values():
    s.close()
med = {c: float(np.median([r["ms_per_step"] for r in lines if r["case"] == c])) for c in samplers}
for c in samplers:
    ms = [r["ms_per_step"] for r in lines if r["case"] == c]
    rec = {"case": c, "summary": True, "repeats": a.repeats, "steps": a.steps, "cells": cells[c],
           "ms_per_step_median": med[c], "ms_per_step_min": min(ms), "ms_per_step_max": max(ms)}
    if "mask" in med:
        rec["vs_mask"] = med[c] / med["mask"]
    print(json.dumps(rec), flush=True)
    lines.append(rec)
if a.out:
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
