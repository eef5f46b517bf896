"""The fused colour phase's 8-double heavy-segment records (epv_propose2.h): length and address word stay in slots 6
and 7, the eight fields come in two passes over slots 0..5 (P00, P11 before pruning; PT00, PT10, the no-jump bounds
and the Philox block behind it), and the downward pass parks a dirty heavy branch's sampled states and its
dirty-segment mask in its first record for the hand-over.  Nothing of that may change a bit.

Every case runs in a process of its own with its knobs in the environment (a context reads them when it is created),
asserts through DeviceSampler.phase_plan that the kernel it is about ran, and compares paths, cached likelihoods, J, D,
the accept counts and the overflow counter after three sweeps and after run_mcmc(2, 3) behind them with a reference,
bit for bit:

  a  tree.nwk, 245 sites (81 or 82 of a colour: two waves at 64 sites per wave, the second partial) at 16, 32 and
     64 sites per wave, capacity 16: launch tails at every width
  b  the same on dense histories (dense_cases: weak-tree40, every branch heavy) at capacity 16, and thinned to at
     most one jump per path at capacities 1 and 2, where nearly every proposal over the long branches overflows:
     K up to 2C+1, several dirty segments per branch, more than 32 segments in a wave, waves that need several rounds
  c  the other bodies: pair (NN = 2), cherry and star3 (3 and 4 nodes), the generic body on tree.nwk
     (EPV_P2_SMALL_TREE=0) and on the 8-leaf balanced tree
  d  EPV_OPT_LEAF_FAST with one masked and one evidence cell; EPV_OPT_DIRECT_FUSED on dense histories
  e  EPV_OPT_DIRECT_SAMPLER without EPV_OPT_DIRECT_FUSED, EPV_SEG_JUMPS=1, dense histories: the second kernel with
     10-double records in a pool planned next to a fused body (plan_p2's floor, tests/test_plan_records.py)

The reference is the oracle's parallel rung B.  The direct sampler has no oracle rung, so the direct rows of d and e
take what tests/test_direct_fused_gpu.py takes: the same chain in direct mode through the first proposal kernel
(EPV_PROPOSE_V1=1, fused phase off), which has a record pool of its own and shares no proposal code with the rows."""
import json
import os
import subprocess
import sys

import pytest

import dense_cases as dc
from common import config

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))

N_TAILS = 245
SEED = 23

_CHILD = r'''
import ctypes as C, json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import orc, dense_cases as dc
from common import config, ref_test_model
from epievo_amd import host
from epievo_amd.sampler import DeviceSampler, EPV_OK, EPV_ERR_CAPACITY
spec = json.loads(%(spec)r)
SEED = spec["seed"]

def inputs():
    if spec["input"] == "sparse":
        model, tree = ref_test_model(), config(spec["tree"])
        fp = host.simulate(model, tree, spec["n"], 11)
        return model, tree, fp, spec["cap"] or int(max(16, 2 * fp.counts().max() + 8))
    model, tree, fp = dc.workload(spec["workload"])
    if spec["input"] == "thinned":                     # at most one jump per path, end states kept
        fp = dc.thin(fp, 1, 0)
    assert int(fp.counts().max()) <= spec["cap"]
    return model, tree, fp, spec["cap"]

def held(tree, fp):
    """one masked and one evidence cell on two leaves, inside the first wave and inside the last"""
    B, n = tree.n_nodes - 1, fp.n_sites
    leaves = [b - 1 for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1]
    mask = np.zeros((B, n), np.uint8)
    mask[leaves[0], 7] = 1
    r = np.full((B, n), np.nan, np.float32)
    r[leaves[-1], n - 9] = 0.3
    return mask, r

def device(model, tree, fp, cap, env, direct=None):
    for k in [k for k in os.environ if k.startswith("EPV_")]:
        del os.environ[k]
    os.environ.update(env)                             # read when a context is created
    d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap)
    if spec.get("leaf_fast"):
        d.set_leaf_fast(True)
        mask, r = held(tree, fp)
        d.set_unobserved(mask); d.set_leaf_evidence(r)
    if direct is not None:
        d.set_direct_sampler(True, fused=direct)
    d.reset()
    return d

def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)

class Dev:
    """the device's side; an overflow leaves a valid chain and complete outputs (rc EPV_ERR_CAPACITY)"""
    def __init__(self, d):
        self.d = d
    def sweep(self, w):
        nacc = C.c_uint64(0)
        rc = self.d.L.epv_sweep(self.d.h, 1, SEED, w, C.byref(nacc))
        assert rc in (EPV_OK, EPV_ERR_CAPACITY), (rc, self.d.L.epv_last_error(self.d.h))
        return int(nacc.value)
    def run_mcmc(self, burn, batch, base):
        J, D = np.zeros(self.d.B * 8), np.zeros(self.d.B * 8)
        nacc = C.c_uint64(0)
        dp = C.POINTER(C.c_double)
        rc = self.d.L.epv_run_mcmc_sums(self.d.h, burn, batch, SEED, base, 1, J.ctypes.data_as(dp), D.ctypes.data_as(dp),
                                        C.byref(nacc))
        assert rc in (EPV_OK, EPV_ERR_CAPACITY), (rc, self.d.L.epv_last_error(self.d.h))
        return J, D, int(nacc.value)
    def suffstats(self): return self.d.suffstats()
    def paths(self): return self.d.paths()
    def tri_llh(self): return self.d.tri_llh()
    def overflow(self): return self.d.counters()["overflow"]

class Orc:
    def __init__(self, o):
        self.o = o
    def sweep(self, w): return int(self.o.sweep(w))
    def run_mcmc(self, burn, batch, base):
        J, D, nacc, _ = self.o.run_mcmc(burn, batch, sweep_base=base)
        return J, D, int(nacc)
    def suffstats(self): return self.o.suffstats()
    def paths(self): return self.o.paths()
    def tri_llh(self): return self.o.tri_llh()
    def overflow(self): return self.o.counters()["overflow"]

def same_state(a, b, what):
    assert orc.paths_equal(a.paths(), b.paths()), (what, "paths")
    assert np.array_equal(bits(a.tri_llh()), bits(b.tri_llh())), (what, "tri_llh")
    assert a.overflow() == b.overflow(), (what, "overflow", a.overflow(), b.overflow())

def compare(a, b):
    """three sweeps, then run_mcmc(2, 3) behind them: accept counts, paths, tri_llh, J, D, overflow counter"""
    for w in range(3):
        na, nb = a.sweep(w), b.sweep(w)
        assert na == nb, ("sweep", w, na, nb)
    same_state(a, b, "after 3 sweeps")
    (Ja, Da), (Jb, Db) = a.suffstats(), b.suffstats()
    assert np.array_equal(bits(Ja), bits(Jb)) and np.array_equal(bits(Da), bits(Db)), "J, D after 3 sweeps"
    Ja, Da, na = a.run_mcmc(2, 3, 3)
    Jb, Db, nb = b.run_mcmc(2, 3, 3)
    assert na == nb, ("run_mcmc", na, nb)
    assert np.array_equal(bits(Ja), bits(Jb)) and np.array_equal(bits(Da), bits(Db)), "J, D of run_mcmc"
    same_state(a, b, "after run_mcmc")
    return na

model, tree, fp, cap = inputs()
d = device(model, tree, fp, cap, spec["env"], spec.get("direct"))
plan = d.phase_plan()
print("plan", json.dumps(plan), flush=True)
bad = dict((k, (v, plan[k])) for k, v in spec["expect"].items() if plan[k] != v)
assert not bad, "plan differs (expected, got): %%r" %% bad
if spec.get("direct") is None:
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=SEED)
    if spec.get("leaf_fast"):
        mask, r = held(tree, fp)
        o.set_unobserved(mask); o.set_leaf_evidence(r)
        assert plan["unobs"] and plan["evidence"], plan
    o.reset()
    ref = Orc(o)
else:
    d1 = device(model, tree, fp, cap, {"EPV_PROPOSE_V1": "1", "EPV_FUSED_PHASE": "0"}, False)
    p1 = d1.phase_plan()
    assert p1["propose"] == "V1" and p1["direct"] and plan["direct"], (p1, plan)
    ref = Dev(d1)
nacc = compare(Dev(d), ref)
cnt = d.counters()
assert d.phase_plan() == plan
if spec.get("overflows"):
    assert cnt["overflow"] > 0, cnt
else:
    assert cnt["overflow"] == 0, cnt
if plan["propose"] == "fused":
    assert cnt["coop_tasks"] > 0, cnt              # dirty branches went through the hand-over
if spec.get("direct") is not None:
    assert d.direct_giveups() == 0
print("result", json.dumps(dict(accepted=nacc, counters=cnt, kmax=dc.density(fp)["kmax"], cap=cap)), flush=True)
print("ok")
'''

FUSED_ON = {"EPV_FUSED_PHASE": "1", "EPV_FORCE_LDS_POOL": "1"}
DENSE = "weak-tree40"


def fused(nn, lanes):
    return dict(propose="fused", small_nn=nn, jumps="fused", accept="fused", fused_lanes=lanes)


def sparse(tree, n, nn, lanes, cap=16, env=None, **more):
    return dict(input="sparse", tree=tree, n=n, cap=cap, env=dict(FUSED_ON, EPV_FUSED_LANES=str(lanes), **(env or {})),
                expect=fused(nn, lanes), **more)


def dense(cap, nn, lanes, thinned=False, env=None, expect=None, **more):
    return dict(input="thinned" if thinned else "dense", workload=DENSE, cap=cap,
                env=dict(FUSED_ON, EPV_FUSED_LANES=str(lanes), **(env or {})), expect=expect or fused(nn, lanes), **more)


GENERIC = {"EPV_P2_SMALL_TREE": "0"}
CASES = {}
for _L in (16, 32, 64):
    CASES["a-tails-lanes%d" % _L] = sparse("tree", N_TAILS, 5, _L)
    CASES["b-dense-cap16-lanes%d" % _L] = dense(16, 5, _L)
for _C in (1, 2):
    CASES["b-thinned-cap%d-lanes64" % _C] = dense(_C, 5, 64, thinned=True, overflows=True)
    CASES["b-thinned-cap%d-lanes16" % _C] = dense(_C, 5, 16, thinned=True, overflows=True)
CASES["c-pair"] = sparse("pair", 200, 2, 64, cap=0)
CASES["c-cherry"] = sparse("cherry", N_TAILS, 3, 64)
CASES["c-star3"] = sparse("star3", N_TAILS, 4, 32)
CASES["c-tree-generic"] = sparse("tree", N_TAILS, 0, 64, env=GENERIC)
CASES["c-bal8-generic"] = sparse("bal8", N_TAILS, 0, 64)
CASES["c-dense-generic"] = dense(16, 0, 64, env=GENERIC)
CASES["d-leaf-fast-tree"] = sparse("tree", N_TAILS, 5, 64, leaf_fast=True)
CASES["d-leaf-fast-dense-generic"] = dense(16, 0, 32, env=GENERIC, leaf_fast=True)
CASES["d-direct-fused-dense"] = dense(16, 5, 64, direct=True)
CASES["d-direct-fused-dense-generic"] = dense(16, 0, 16, env=GENERIC, direct=True)
CASES["e-direct-v2-segments-dense"] = dense(16, 0, 64, env={"EPV_SEG_JUMPS": "1"}, direct=False,
                                            expect=dict(propose="V2", jumps="segments", direct=True))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_records_match_the_reference(case):
    spec = dict(CASES[case], seed=SEED)
    src = _CHILD % dict(root=_ROOT, tests=_TESTS, spec=json.dumps(spec))
    clean = dict((k, v) for k, v in os.environ.items() if not k.startswith("EPV_"))
    r = subprocess.run([sys.executable, "-c", src], env=clean, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


# ---- without a GPU: the inputs are what the cases say
def test_tails_fill_a_wave_and_a_part_of_one():
    for colour in range(3):
        count = len([s for s in range(1, N_TAILS - 1) if s % 3 == colour])
        assert 64 < count < 128 and count % 16 and count % 32, (colour, count)


def test_dense_inputs_fit_their_capacities():
    model, tree, fp = dc.workload(DENSE)
    assert tree.n_nodes == 5 and int(fp.counts().max()) <= 16
    dens = dc.density(fp)
    assert dens["kmax"] >= 10 and dens["k1"] < 0.5, dens            # heavy records on most branches
    # more than 32 heavy segments in a wave of 16 sites
    B, n = tree.n_nodes - 1, fp.n_sites
    nj = fp.counts().reshape(B, n)
    K = nj[:, :-2] + nj[:, 2:] + 1
    assert int(K[:, 0:48:3].sum()) > 32
    thin = dc.thin(fp, 1, 0)
    assert int(thin.counts().max()) == 1 and (thin.init == fp.init).all()
    for c in sorted(CASES):
        assert json.dumps(CASES[c])
    assert config("bal8").n_nodes == 15 and config("star3").n_nodes == 4 and config("cherry").n_nodes == 3
