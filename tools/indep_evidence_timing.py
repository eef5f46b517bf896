"""Cost of the leaf mask and of leaf evidence in the site-independent stage (epievo_initialization's kernels): the
config-3 shape (tree.nwk, n = 1e6) on one context.  Four cases: no table, a mask on a fraction of the leaf cells,
evidence on the same cells, evidence on every leaf cell.  Per case indep_expectation, one indep_update_paths call
and indep_node_posterior are timed with a host clock around the call (each ends in a stream synchronise; the
posterior's time includes its [N][n] read-out to the host).  The cases alternate over the repeats, so that drift
of the machine hits all of them alike.  One JSON line per case and repeat, then one summary line per case
(medians, and the ratio to the no-table case of the same session, which runs the kernels a context without tables
always ran).

  python tools/indep_evidence_timing.py [--n 1000000] [--frac 0.1] [--calls 200] [--repeats 7]
                                        [--out profiles/indep_evidence_timing.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epievo_amd.sampler import DeviceSampler  # noqa: E402
from epievo_amd.workloads import simulate  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--frac", type=float, default=0.1)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--cases", default="none,mask,evidence,evidence_all")
ap.add_argument("--out", default="")
a = ap.parse_args()

RATES = np.array([0.7, 1.9])
model, tree, fp = simulate("tree", a.n, seed=1)
B, n = tree.n_nodes - 1, fp.n_sites
rng = np.random.default_rng(3)
leaf_rows = [b - 1 for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1]
mask = np.zeros((B, n), np.uint8)
for b in leaf_rows:
    mask[b] = rng.random(n) < a.frac
nan = np.float32(np.nan)
soft = (0.02 + 0.96 * rng.random((B, n))).astype(np.float32)
evidence = np.where(mask != 0, soft, nan).astype(np.float32)
evidence_all = np.full((B, n), nan, np.float32)
evidence_all[leaf_rows] = soft[leaf_rows]
cells = {"none": 0, "mask": int(mask.sum()), "evidence": int(mask.sum()), "evidence_all": len(leaf_rows) * n}

devs = {}
for case in a.cases.split(","):
    d = DeviceSampler(0)
    d.auto_grow = True
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, 32)
    if case == "mask":
        d.set_unobserved(mask)
    elif case == "evidence":
        d.set_leaf_evidence(evidence)
    elif case == "evidence_all":
        d.set_leaf_evidence(evidence_all)
    d.indep_expectation(RATES)             # warm-up: allocations, first launches
    d.indep_update_paths(RATES, 1, 0xF0000000)
    d.indep_node_posterior(RATES)
    devs[case] = d


def timed(f):
    t0 = time.perf_counter()
    for _ in range(a.calls):
        f()
    return (time.perf_counter() - t0) / a.calls * 1e3


lines, sweep = [], 1
for rep in range(a.repeats):
    for case, d in devs.items():
        def update():
            global sweep
            sweep += 1
            d.indep_update_paths(RATES, 1, 0xF0000000 + sweep)
        rec = {"case": case, "repeat": rep, "n_sites": n, "cells": cells[case], "leaf_cells": len(leaf_rows) * n,
               "expectation_ms": timed(lambda: d.indep_expectation(RATES)),
               "update_paths_ms": timed(update),
               "node_posterior_ms": timed(lambda: d.indep_node_posterior(RATES))}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
for d in devs.values():
    d.close()
KEYS = ("expectation_ms", "update_paths_ms", "node_posterior_ms")
med = {c: {k: float(np.median([r[k] for r in lines if r["case"] == c])) for k in KEYS} for c in devs}
for c in devs:
    rec = {"case": c, "summary": True, "repeats": a.repeats, "calls": a.calls, "cells": cells[c]}
    for k in KEYS:
        v = [r[k] for r in lines if r["case"] == c]
        rec[k + "_median"], rec[k + "_min"], rec[k + "_max"] = med[c][k], min(v), max(v)
        if "none" in med:
            rec[k[:-3] + "_vs_none"] = med[c][k] / med["none"][k]
    print(json.dumps(rec), flush=True)
    lines.append(rec)
if a.out:
    with open(a.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
