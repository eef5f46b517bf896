"""Every colour-phase kernel path, the statistics kernels and the accumulate kernels on dense histories: paths of
tens of jumps (dense_cases.py), where the other GPU tests' inputs have two or three at the most.

What only such inputs reach: branches of more than 64 segments, which leave the segment lists for the bucketed
lists of the sequential kernel; two and more words of proposal states per (site, branch); the fused phase at its
largest capacity with every branch heavy; the LDS merge rings of the statistics kernels filling and wrapping;
lower_bound and the gain / loss counts of the accumulate kernels beyond two; log ratios that are sums over
hundreds of segments.

Each row runs in a fresh process with its knobs in the environment (a context reads them when it is created),
asserts the plan fields it names (DeviceSampler.phase_plan) and compares with the oracle's parallel rung B in the
same mode, bit for bit.  Every child prints one "result" line: the plan, the acceptance, K max, the overflow
count and search_finished / coop_tasks.

Plans.  A context sizes its LDS record pool from the mean jump count of the uploaded paths, and on these inputs
that "typical" demand is beyond what leaves five waves per CU -- on most of them beyond LDS altogether.  So without
a knob no dense row takes the second proposal kernel or the fused phase: trees the large-tree kernel takes go
there (every one here but multi), the others to the first kernel with its pool in global memory.  With
EPV_FORCE_LDS_POOL, the knob test_kernel_matrix.py's fused cat6 row uses for the same reason, the four small-tree
workloads at C = 31 take the fused phase; nothing denser does.  The second kernel's segment lists, its branches of
more than 64 segments and the fused generic body are reached by inputs that are dense in a window only
(dense_cases.MIXED): sparse on average when the plan is made, dense everywhere after a sweep.  Every row of the
homogeneous inputs is kept and asserts the plan it takes.

The fused phase's two exits.  The grouped search, which finishes a branch whose sole dirty segment it has settled,
takes a wave's segment list only when it has at most 32 entries; a wave of 16, 32 or 64 dense sites lists hundreds.
The rows that assert 0 < search_finished < coop_tasks therefore run four sites a wave (EPV_FUSED_LANES=4).

Sites per wave.  These inputs have 400 or 600 sites, where a context chooses 16 sites per wave by itself (plan_p2:
32 and 64 only above 98301 and 196605 sites), so the fused rows without EPV_FUSED_LANES run 16.  The rows named
-lanes32 and -lanes64 set the knob: four times the demand on the record pool, several rounds of the proposal loop
per wave, private lists four times as long, up to 192 (site, triple) tasks in the acceptance.  Every fused row
asserts its fused_lanes (test_fused_lanes.py runs the widths on sparse inputs at the launch tails).

Observed on the MI355X (acceptance, K max; search_finished / coop_tasks at 4 and at 16 sites a wave):
  pair x 4 0.753, 18 (47 and 1 / 2983)    cherry x 12 0.720, 16       star3 x 15 0.641, 22
  tree x 40 0.650, 19 (1034 and 0 / 10780; C = 12: 3 overflows)       star5 x 20 0.525, 24
  cat6 x 25 0.420, 27     tree x 150 0.374, 52 (C = 30: 1 overflow)   pair x 25 0.388, 72
  pair x 40 0.291, 109 (C = 58: 9 overflows)    tree x 300 0.184, 85  cat6 x 150 0.053, 108
  multi x 30 0.223, 71    bal8 x 100 0.172, 27  bal16 x 60 0.161, 19  flat rows 1.000, 87 / 59 / 46 / 42
  thinned: pair x 40 0.187, 100 (C = 55: 26 overflows)   tree x 300 0.157, 76   tree x 150 0.292, 44
  (C = 25: 24 overflows, 3 / 7923)   star5 x 20 0.522, 24   tree x 40 0.635, 16"""
import json
import os
import subprocess
import sys

import pytest

import dense_cases as dc

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))

_HEAD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import orc, dense_cases as dc, pavg_ref, bevents_ref
from epievo_amd.sampler import DeviceSampler
spec = json.loads(%(spec)r)
name, opts, expect = spec["workload"], spec.get("opts", {}), spec.get("expect", {})
model, tree, fp = dc.workload(name)
SEED = dc.ORACLE_SEED
dens = dc.density(fp)

def device(cap, rng=None):
    d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap); d.set_options(**opts)
    if rng:
        d.set_update_range(*rng)
    return d

def check_plan(d):
    plan = d.phase_plan()
    print("plan", json.dumps(plan), flush=True)
    bad = dict((k, (v, plan[k])) for k, v in expect.items() if plan[k] != v)
    assert not bad, "plan differs (expected, got): %%r; plan %%r" %% (bad, plan)
    return plan

def result(plan, cap, nacc, sweeps, cnt):
    print("result", json.dumps(dict(workload=name, cap=cap, W=dc.words(cap), propose=plan["propose"], gpool=plan["gpool"],
          small_nn=plan["small_nn"], fused_lanes=plan["fused_lanes"], jumps=plan["jumps"], accept=plan["accept"], acceptance=round(nacc / float(sweeps * (fp.n_sites - 2)), 3),
          kmax=dens["kmax"], over64=round(dens["over64"], 3), overflow=cnt["overflow"], search_finished=cnt["search_finished"],
          coop_tasks=cnt["coop_tasks"])), flush=True)
'''

# one launch plan against rung B: J, D, accepts, paths, cached likelihoods, overflow
_PARITY = _HEAD + r'''
cap = dc.capacity(name, fp, spec["cap"])
d = device(cap); d.reset()
plan = check_plan(d)
o = dc.oracle(name, cap, opts)
# (SAMPLE_ROOT: the two end sites' cached likelihoods are never read and not kept current, test_sample_root.py)
lo, hi = (1, -1) if opts.get("sample_root") else (0, None)
if spec["cap"] == "tight":
    # a capacity that overflows: the overflow decisions are the sequential sampler's, sweep by sweep
    nacc = 0
    for w in range(4, 9):
        try:
            nacc += d.sweep(1, SEED, sweep_base=w)
        except Exception as e:
            assert "rejected" in str(e) or "capacity" in str(e).lower(), e
        o.sweep(w)
        assert orc.paths_equal(d.paths(), o.paths()), "paths differ after overflow sweep %%d" %% w
        assert np.array_equal(d.tri_llh()[lo:hi].view(np.uint64), o.tri_llh()[lo:hi].view(np.uint64)), w
    cnt = d.counters()
    assert cnt["overflow"] == o.counters()["overflow"] > 0, (cnt, o.counters())
    sweeps = 5
else:
    Jd, Dd, nacc = d.run_mcmc(2, 3, SEED, sweep_base=4)
    Jo, Do, no, _ = o.run_mcmc(2, 3, sweep_base=4)
    cnt = d.counters()
    print("counters", cnt, "accepted", nacc, no, flush=True)
    assert nacc == no, (nacc, no)
    assert np.array_equal(Jd, Jo) and np.array_equal(Dd, Do)
    assert orc.paths_equal(d.paths(), o.paths())
    assert np.array_equal(d.tri_llh()[lo:hi].view(np.uint64), o.tri_llh()[lo:hi].view(np.uint64))
    assert cnt["overflow"] == o.counters()["overflow"] == 0, (cnt, o.counters())
    if model.rates.min() == model.rates.max():          # flat: every interior proposal is accepted
        assert nacc == 3 * (fp.n_sites - 2), nacc
    sweeps = 3
assert cnt["search_finished"] <= cnt["coop_tasks"], cnt
if spec.get("some"):        # both exits of the fused phase ran: the search's own finish and the assembly stage
    assert 0 < cnt["search_finished"] < cnt["coop_tasks"], cnt
assert d.phase_plan() == plan
result(plan, cap, nacc, sweeps, cnt)
d.close()
print("ok")
'''

# the block kernel (run_mcmc, suffstats) and the wave kernel (run_mcmc_counts) against rung B and the yardstick
_STATS = _HEAD + r'''
cap = dc.capacity(name, fp, "roomy")
rng = spec["range"]
first, last = rng if rng else (1, fp.n_sites - 2)
B = tree.n_nodes - 1
d, d2 = device(cap, rng), device(cap, rng)
d.reset(); d2.reset()
plan = check_plan(d)
o = dc.oracle(name, cap, opts)
dp = C.POINTER(C.c_double)
def orc_sweep(w):
    return sum(int(o.L.orc_sweep_phase(o.h, c, w, first, last, first, last)) for c in range(3))
def orc_stats():
    J, D = np.zeros(B * 8), np.zeros(B * 8)
    o.L.orc_suffstats_range(o.h, first, last, J.ctypes.data_as(dp), D.ctypes.data_as(dp))
    return J, D
orc_sweep(4)
no, Jo, Do = 0, np.zeros(B * 8), np.zeros(B * 8)
for w in (5, 6):
    no += orc_sweep(w)
    J1, D1 = orc_stats()
    Jo, Do = Jo + J1, Do + D1
Jo, Do = Jo / 2.0, Do / 2.0
Jd, Dd, nacc = d.run_mcmc(1, 2, SEED, sweep_base=4)                  # the block kernel, once per batch sweep
assert nacc == no, (nacc, no)
assert np.array_equal(Jd, Jo) and np.array_equal(Dd, Do)
assert orc.paths_equal(d.paths(), o.paths())
Js, Ds = d.suffstats()                                               # the block kernel on the resident paths
assert np.array_equal(Js, J1) and np.array_equal(Ds, D1)
counts, nacc2 = d2.run_mcmc_counts(1, 2, SEED, sweep_base=4)         # the wave kernel
assert nacc2 == no and orc.paths_equal(d2.paths(), o.paths())
Jw, Dw = d2.counts_to_stats(counts, 2)
assert np.array_equal(Jw, Jo) and np.array_equal(Dw, Do)
Jl, Dl = d2.counts_to_stats(counts[1:], 1)
assert np.array_equal(Jl, J1) and np.array_equal(Dl, D1)
# ... and all of them against the walk over the device's own paths, within the bound dense_cases derives
Jy, Dy, n_int = dc.yardstick(d.paths(), tree.branches, first, last)
assert np.array_equal(Jy.reshape(-1), Js.astype(np.int64)) and np.array_equal(Js, Js.astype(np.int64))
bound = dc.dwell_bound(n_int, Dy, dc.stat_scales(o))
err = np.abs(Ds.reshape(B, 8) - Dy)
print("worst D error / bound", float((err / bound).max()), "intervals per cell up to", int(n_int.max()), flush=True)
assert np.all(err <= bound), (err / bound).max()
result(plan, cap, nacc, 2, d.counters())
d.close(); d2.close()
print("ok")
'''

# the accumulate kernels of the path average and the branch events, after every batch sweep of run_mcmc
_ACCUM = _HEAD + r'''
cap = dc.capacity(name, fp, "roomy")
P, B, n = 9, tree.n_nodes - 1, fp.n_sites
d = device(cap)
d.enable_path_average(P); d.enable_branch_events(); d.reset()
plan = check_plan(d)
o = dc.oracle(name, cap, opts)
Jd, Dd, nacc = d.run_mcmc(2, 3, SEED, sweep_base=4)
o.sweep(4); o.sweep(5)
want_pa, want_be, no = np.zeros((B, n, P), np.uint32), np.zeros((6, B, n), np.uint32), 0
for w in (6, 7, 8):
    no += o.sweep(w)
    want_pa += pavg_ref.counts(o.paths(), tree.branches, P)
    want_be += bevents_ref.counts(o.paths())
assert nacc == no and orc.paths_equal(d.paths(), o.paths())
ns, pa = d.path_average(counts=True)
assert ns == 3 and pa.dtype == np.uint32 and np.array_equal(pa, want_pa)
ns, be = d.branch_events(counts=True)
assert ns == 3 and be.dtype == np.uint32 and np.array_equal(be, want_be)
assert int(want_be[4:].max()) > 2 and int(bevents_ref.counts(o.paths())[4:].max()) > 2     # gain / loss counts beyond two
ns, win = d.branch_event_windows(7)
assert ns == 3 and np.array_equal(win, bevents_ref.windows(want_be, 7))
result(plan, cap, nacc, 3, d.counters())
d.close()
print("ok")
'''

SEP = {"EPV_FUSED_PHASE": "0"}
SEG1, SEG0 = dict(SEP, EPV_SEG_JUMPS="1"), dict(SEP, EPV_SEG_JUMPS="0")
LDS = {"EPV_FORCE_LDS_POOL": "1"}
FUSED_LDS = {"EPV_FUSED_PHASE": "1", "EPV_FORCE_LDS_POOL": "1"}
V3 = dict(SEP, EPV_PROPOSE_V3="1")
FR, REF, SR = {"forward_rejection": True}, {"reference_proposal_ratio": True}, {"sample_root": True}
FRREF = {"forward_rejection": True, "reference_proposal_ratio": True}


def fused(nn, lanes=16):
    return dict(propose="fused", small_nn=nn, jumps="fused", accept="fused", gpool=False, listed=False,
                fused_lanes=lanes)


def v2(jumps, accept="accept_cache"):
    return dict(propose="V2", gpool=False, jumps=jumps, accept=accept, listed=True, small_nn=0, p3_words=0,
                fused_lanes=0)


def v3(words, jumps="jumps_all", accept="accept3", slab=False):
    return dict(propose="V3", p3_words=words, p3_slab_pool=slab, jumps=jumps, accept=accept, listed=True, gpool=False,
                small_nn=0, fused_lanes=0)


def v1(gpool, refq, jumps, accept="accept_cache"):
    return dict(propose="V1", gpool=gpool, refq=refq, jumps=jumps, accept=accept, listed=False, p3_words=0,
                fused_lanes=0)


LANES4 = dict(FUSED_LDS, EPV_FUSED_LANES="4")
LANES32, LANES64 = dict(FUSED_LDS, EPV_FUSED_LANES="32"), dict(FUSED_LDS, EPV_FUSED_LANES="64")

# (id, workload, capacity, env, options, expected plan fields, both fused exits ran).  The plans are the observed
# ones (MI355X); a comment says where a row was written for another.
PARITY = [
    # ---- the fused phase at C = 31, every branch heavy: the small-tree bodies NN = 2 .. 5.  With 16 sites and more
    # a wave its segment list is hundreds long and the wave-wide search and the assembly do everything; the
    # grouped search, whose own finish is the other exit, takes lists of at most 32 segments, so the rows that
    # assert both exits run four sites a wave.  The -wide rows run the width the context chooses at 600 sites, 16
    # (wide next to the four of the rows above them; the 64 of a large genome are the -lanes64 rows)
    ("fused-pair4", "weak-pair4", "roomy", LANES4, {}, fused(2, 4), True),
    ("fused-tree40", "weak-tree40", "roomy", LANES4, {}, fused(5, 4), True),
    ("fused-pair4-wide", "weak-pair4", "roomy", FUSED_LDS, {}, fused(2), False),
    ("fused-cherry12", "weak-cherry12", "roomy", FUSED_LDS, {}, fused(3), False),
    ("fused-star3x15", "weak-star3x15", "roomy", FUSED_LDS, {}, fused(4), False),
    ("fused-tree40-wide", "weak-tree40", "roomy", FUSED_LDS, {}, fused(5), False),
    ("fused-tree40-overflow", "weak-tree40", "tight", FUSED_LDS, {}, fused(5), False),
    ("fused-tree40-overflow-lanes4", "weak-tree40", "tight", LANES4, {}, fused(5, 4), False),
    # ... and at 64 and 32 sites a wave, the widths of genomes above 196605 and 98301 sites
    ("fused-pair4-lanes64", "weak-pair4", "roomy", LANES64, {}, fused(2, 64), False),
    ("fused-cherry12-lanes64", "weak-cherry12", "roomy", LANES64, {}, fused(3, 64), False),
    ("fused-star3x15-lanes64", "weak-star3x15", "roomy", LANES64, {}, fused(4, 64), False),
    ("fused-tree40-lanes64", "weak-tree40", "roomy", LANES64, {}, fused(5, 64), False),
    ("fused-tree40-overflow-lanes64", "weak-tree40", "tight", LANES64, {}, fused(5, 64), False),
    ("fused-tree40-lanes32", "weak-tree40", "roomy", LANES32, {}, fused(5, 32), False),
    # the generic body: star5 x 20 and cat6 x 25 are too dense for the fused phase under any knob (large-tree
    # kernel); star5 x 20 thinned outside a window takes it
    ("fused-star5x20", "weak-star5x20", "roomy", FUSED_LDS, {}, v3(1, accept="accept_cache"), False),
    ("fused-cat6x25", "weak-cat6x25", "roomy", FUSED_LDS, {}, v3(1), False),
    ("fused-mixed-star5x20", "mixed-star5x20", "roomy", FUSED_LDS, {}, fused(0), False),
    ("fused-mixed-star5x20-lanes64", "mixed-star5x20", "roomy", LANES64, {}, fused(0, 64), False),
    ("fused-mixed-star5x20-lanes32", "mixed-star5x20", "roomy", LANES32, {}, fused(0, 32), False),
    ("fused-mixed-tree40", "mixed-tree40", "roomy", FUSED_LDS, {}, fused(5), False),
    # the same inputs without a knob: the plan the context chooses for them
    ("default-pair4", "weak-pair4", "roomy", {}, {}, v3(1, accept="accept_cache"), False),
    ("default-tree40", "weak-tree40", "roomy", {}, {}, v3(1, accept="accept_cache"), False),
    # ---- two and more words of proposal states, every K <= 64: weak tree x 150 (C = 68, W = 3).  Too dense for the
    # second proposal kernel: the large-tree kernel whatever EPV_SEG_JUMPS says, and the first kernel's pool in
    # global memory with or without EPV_FORCE_GLOBAL_POOL
    ("w3-default", "weak-tree150", "roomy", {}, {}, v3(1, accept="accept_cache"), False),
    ("w3-seg", "weak-tree150", "roomy", SEG1, {}, v3(1, accept="accept_cache"), False),
    ("w3-noseg", "weak-tree150", "roomy", SEG0, {}, v3(1, accept="accept_cache"), False),
    ("w3-v1", "weak-tree150", "roomy", dict(SEP, EPV_PROPOSE_V1="1"), {}, v1(True, False, "jumps_all"), False),
    ("w3-v1-global", "weak-tree150", "roomy", dict(SEP, EPV_PROPOSE_V1="1", EPV_FORCE_GLOBAL_POOL="1"), {},
     v1(True, False, "jumps_all"), False),
    ("w3-no-cache", "weak-tree150", "roomy", dict(SEP, EPV_ACCEPT_NO_CACHE="1"), {}, v3(1), False),
    ("w3-fr", "weak-tree150", "roomy", {}, FR, v3(1, "jumps", "accept_cache"), False),
    ("w3-ref", "weak-tree150", "roomy", {}, REF, v1(True, True, "jumps_all"), False),
    ("w3-frref", "weak-tree150", "roomy", {}, FRREF, v1(True, True, "jumps"), False),
    ("w3-sr", "weak-tree150", "roomy", {}, SR, v1(True, True, "jumps_all"), False),
    # ... and thinned outside a window: the second proposal kernel at W = 2
    ("w2-mixed-tree150-seg", "mixed-tree150", "roomy", dict(SEG1, **LDS), {}, v2("segments"), False),
    ("w2-mixed-tree150-noseg", "mixed-tree150", "roomy", dict(SEG0, **LDS), {}, v2("jumps_all"), False),
    # its own maximum as capacity (C = 30, W = 1, K max 52), overflowing: written for the fused phase's limit case,
    # which the thinned input reaches (C = 25, K max 44)
    ("fused-tree150-overflow", "weak-tree150", "tight", FUSED_LDS, {}, v3(1, accept="accept_cache"), False),
    ("fused-mixed-tree150-overflow", "mixed-tree150", "tight", FUSED_LDS, {}, fused(5), False),
    ("fused-mixed-tree150-overflow-lanes64", "mixed-tree150", "tight", LANES64, {}, fused(5, 64), False),
    ("w3-multi30", "weak-multi30", "roomy", {}, {}, v1(True, False, "jumps_all"), False),
    # ---- more than 64 segments on a branch.  The homogeneous inputs go to the large-tree kernel, which keeps such a
    # branch's proposal states out of the two-word hand-over (epv_propose3.h, K <= 64)
    ("over64-pair40-seg", "weak-pair40", "roomy", SEG1, {}, v3(1, accept="accept_cache"), False),
    ("over64-pair40-noseg", "weak-pair40", "roomy", SEG0, {}, v3(1, accept="accept_cache"), False),
    ("over64-pair25-seg", "weak-pair25", "roomy", SEG1, {}, v3(1, accept="accept_cache"), False),
    ("over64-pair25-noseg", "weak-pair25", "roomy", SEG0, {}, v3(1, accept="accept_cache"), False),
    ("over64-tree300-seg", "weak-tree300", "roomy", SEG1, {}, v3(1, accept="accept_cache"), False),
    ("over64-tree300-noseg", "weak-tree300", "roomy", SEG0, {}, v3(1, accept="accept_cache"), False),
    ("over64-cat6x150-seg", "weak-cat6x150", "roomy", SEG1, {}, v3(1), False),
    ("over64-cat6x150-noseg", "weak-cat6x150", "roomy", SEG0, {}, v3(1), False),
    ("over64-flat-tree300-seg", "flat-tree300", "roomy", SEG1, {}, v3(1, accept="accept_cache"), False),
    ("over64-flat-tree300-noseg", "flat-tree300", "roomy", SEG0, {}, v3(1, accept="accept_cache"), False),
    ("over64-tree300-fr", "weak-tree300", "roomy", SEG1, FR, v3(1, "jumps", "accept_cache"), False),
    ("over64-pair40-seg-overflow", "weak-pair40", "tight", SEG1, {}, v3(1, accept="accept_cache"), False),
    ("over64-pair40-noseg-overflow", "weak-pair40", "tight", SEG0, {}, v3(1, accept="accept_cache"), False),
    # ... and thinned outside a window (dense_cases.MIXED), sparse enough on average for the second proposal
    # kernel: branches of more than 64 segments leave its segment lists for the bucketed lists of the sequential
    # kernel (epv_propose2.h, Kb <= 64) beside branches that stay, and after a sweep the lists fill up
    ("over64-mixed-pair40-seg", "mixed-pair40", "roomy", dict(SEG1, **LDS), {}, v2("segments"), False),
    ("over64-mixed-pair40-noseg", "mixed-pair40", "roomy", dict(SEG0, **LDS), {}, v2("jumps_all"), False),
    ("over64-mixed-pair25-seg", "mixed-pair25", "roomy", dict(SEG1, **LDS), {}, v2("segments"), False),
    ("over64-mixed-tree300-seg", "mixed-tree300", "roomy", dict(SEG1, **LDS), {}, v2("segments"), False),
    ("over64-mixed-tree300-noseg", "mixed-tree300", "roomy", dict(SEG0, **LDS), {}, v2("jumps_all"), False),
    ("over64-mixed-tree300-seg-fr", "mixed-tree300", "roomy", dict(SEG1, **LDS), FR, v2("segments"), False),
    ("over64-mixed-pair40-seg-overflow", "mixed-pair40", "tight", dict(SEG1, **LDS), {}, v2("segments"), False),
    # ---- large trees: the large-tree kernel with one- and two-word masks.  At this density EPV_P3_SLAB_POOL=2
    # sends the 16-leaf tree to the first kernel with its pool in global memory and accept3
    ("bal16x300-v3", "flat-bal16x300", "roomy", V3, {}, v3(1), False),
    ("bal16x300-v3-slab", "flat-bal16x300", "roomy", dict(V3, EPV_P3_SLAB_POOL="2"), {},
     v1(True, False, "jumps_all", "accept3"), False),
    ("bal16x60-v3", "weak-bal16x60", "roomy", V3, {}, v3(1), False),
    ("bal32x400-v3", "flat-bal32x400", "roomy", V3, {}, v3(1), False),
    ("bal64x500-v3", "flat-bal64x500", "roomy", V3, {}, v3(2), False),
    ("bal8x100-default", "weak-bal8x100", "roomy", {}, {}, v3(1), False),
]

# (id, workload, owned range or None for the whole genome): ranges of odd length that start and end inside a
# 64-site block (and, at n = 400, lie on both sides of a 256-site block boundary)
STATS = [
    ("stats-pair40", "weak-pair40", None), ("stats-pair40-range", "weak-pair40", (37, 331)),
    ("stats-tree300", "weak-tree300", None), ("stats-tree300-range", "weak-tree300", (37, 331)),
    ("stats-bal16x300", "flat-bal16x300", None), ("stats-bal16x300-range", "flat-bal16x300", (21, 171)),
]
ACCUM = [("accum-tree150", "weak-tree150"), ("accum-pair40", "weak-pair40")]


def _run(code, spec, env):
    src = code % dict(root=_ROOT, tests=_TESTS, spec=json.dumps(spec))
    r = subprocess.run([sys.executable, "-c", src], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("workload,cap,env,opts,expect,some", [r[1:] for r in PARITY], ids=[r[0] for r in PARITY])
def test_dense_row_matches_rung_b(workload, cap, env, opts, expect, some):
    _run(_PARITY, dict(workload=workload, cap=cap, opts=opts, expect=expect, some=some), env)


@pytest.mark.gpu
@pytest.mark.parametrize("workload,rng", [r[1:] for r in STATS], ids=[r[0] for r in STATS])
def test_statistics_kernels_on_dense_paths(workload, rng):
    """the 512-slot merge ring of the block kernel and the 128-slot ring of the wave kernel fill and wrap:
    paths of tens of jumps on all three sites, 30 branches in several blockIdx.y slices"""
    _run(_STATS, dict(workload=workload, range=rng), SEP)


@pytest.mark.gpu
@pytest.mark.parametrize("workload", [r[1] for r in ACCUM], ids=[r[0] for r in ACCUM])
def test_accumulate_kernels_on_dense_paths(workload):
    _run(_ACCUM, dict(workload=workload), {})


def test_rows_name_known_workloads():
    """no GPU: every row's workload exists, tight rows are the overflow workloads, ranges are as described"""
    assert len(set(r[0] for r in PARITY + STATS + ACCUM)) == len(PARITY) + len(STATS) + len(ACCUM)
    for r in PARITY:
        assert dc.base(r[1]) in dc.WORKLOADS and r[2] in ("roomy", "tight"), r[0]
        assert r[2] == "roomy" or r[1] in dc.OVERFLOW, r[0]
        if r[5].get("propose") == "fused":
            assert "fused" in dc.WORKLOADS[dc.base(r[1])][4] or r[2] == "tight", r[0]
    for _, w, rng in STATS:
        n = dc.WORKLOADS[w][3]
        if rng:
            first, last = rng
            assert 1 < first < last < n - 2 and (last - first + 1) % 2 == 1
            assert first % 64 and (last + 1) % 64 and first // 64 != last // 64
