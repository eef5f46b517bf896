"""The fused colour phase after its integer and scalar work was trimmed (plain-C Philox multiplies in the
fused kernels, no proposal-ratio load): every result must still be the parallel rung's
(oracle rung B), bit for bit -- paths, cached triple likelihoods, J, D and the accept counts -- with the
small-tree body and with the generic one, each asserted to be the body that ran.

  * trees and path selection: tree.nwk (5 nodes) and the single branch with T = 1, n = 193 (one full wave
    of 64 sites per colour and a partial one whose first and last lanes read the edge columns) and
    n = 1000 (several waves per launch), three sweeps;
  * seeds with high bits set in both words and sweep numbers up to 2^32 - 2: the round keys wrap;
  * pool rounds: a window of sites whose every path carries 2 or 3 jumps at capacity 4, so that a wave
    needs several rounds of its LDS pool, lists more than 32 dirty segments and takes the assembly stage;
  * the device's Philox blocks themselves against the oracle's, in every form a kernel inlines."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))

SEEDS = (0xFFFFFFFF9E3779B9, 0xBB67AE85F0000001)
SWEEP_BASE = 2 ** 32 - 4          # sweeps 2^32 - 4, - 3, - 2

# the dense window of the pool-rounds input: 96 consecutive sites inside the 192 that one wave owns (a
# wave of the fused phase takes 64 sites of a colour, every third site from 192 w + ...), i.e. 32 of
# its lanes in every colour
DENSE_N, DENSE_LO, DENSE_HI, DENSE_CAP = 1000, 384, 479, 4


def dense_window_paths(tree, n, lo, hi, seed):
    """FlatPaths with 2 or 3 jumps on every branch of the sites lo .. hi and none elsewhere; the start state
    of a branch is the end state of its parent's, the root states are random"""
    from epievo_amd import host
    rng = np.random.RandomState(seed)
    N = tree.n_nodes
    parent = [int(p) for p in tree.parent_ids]
    T = [float(x) for x in tree.branches]
    site = np.arange(n)
    root = rng.randint(0, 2, n).astype(np.uint8)
    init = np.zeros((N - 1, n), np.uint8)
    cnt = np.zeros((N - 1, n), np.int64)
    end = {0: root}
    for node in range(1, N):
        init[node - 1] = end[parent[node]]
        cnt[node - 1] = np.where((site >= lo) & (site <= hi), 2 + (site + node) % 2, 0)
        end[node] = init[node - 1] ^ (cnt[node - 1] & 1).astype(np.uint8)
    off = np.zeros((N - 1) * n + 1, np.uint64)
    off[1:] = np.cumsum(cnt.reshape(-1))
    jumps = []
    for node in range(1, N):
        for s in range(n):
            k = int(cnt[node - 1, s])
            if k:
                jumps.extend(np.sort(rng.uniform(0.05, 0.95, k)) * T[node])
    return host.FlatPaths(n, N, init.reshape(-1), off, np.array(jumps))


_CODE = r'''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import orc
from common import simulate, config, ref_test_model
from epievo_amd.sampler import DeviceSampler
from test_fused_inst_diet import dense_window_paths, DENSE_LO, DENSE_HI
seed, base, dense = %(seed)d, %(base)d, %(dense)r
if dense:
    model, tree = ref_test_model(), config(%(cfg)r)
    fp = dense_window_paths(tree, %(n)d, DENSE_LO, DENSE_HI, 5)
    cap = %(cap)d
    cnt = fp.counts().reshape(tree.n_nodes - 1, -1)
    assert cnt.max() <= cap and cnt[:, DENSE_LO:DENSE_HI + 1].min() >= 2
    # one wave, one colour: 32 lanes of the window, each with K = 5 .. 7 segments on every branch, i.e. at
    # least B (K + 1) records of 2 doubles and B K heavy records of 10 -- against a pool that plan_p2 accepts
    # for LDS only while a wave's whole share stays within a fifth of the CU's 160 KiB (its lds_ok
    # condition; this line has to follow that limit if it ever moves): more than one round
    B = tree.n_nodes - 1
    assert 32 * B * (2 * 6 + 10 * 5) * 8 > 160 * 1024 // 5
else:
    model, tree, fp = simulate(%(cfg)r, %(n)d, seed=8)
    cap = int(max(16, 2 * fp.counts().max() + 8))

def run(knob):
    os.environ["EPV_P2_SMALL_TREE"] = knob       # read when a context is created
    d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap); d.reset()
    assert d.phase_mode() == 3                    # EPV_PHASE_FUSED
    plan = d.phase_plan()
    assert plan["propose"] == "fused" and plan["small_nn"] == (tree.n_nodes if knob == "1" else 0), plan
    J, D, nacc = d.run_mcmc(1, 2, seed, sweep_base=base)
    out = dict(J=J, D=D, nacc=nacc, paths=d.paths(), tri=d.tri_llh(), cnt=d.counters())
    d.close()
    return out

o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed); o.reset()
Jo, Do, no, _ = o.run_mcmc(1, 2, sweep_base=base)
assert o.counters()["overflow"] == 0
for knob in ("1", "0"):
    r = run(knob)
    assert r["nacc"] == no and no > 0, (knob, r["nacc"], no)
    assert orc.paths_equal(r["paths"], o.paths()), knob
    assert np.array_equal(r["tri"].view(np.uint64), o.tri_llh().view(np.uint64)), knob
    assert np.array_equal(r["J"], Jo) and np.array_equal(r["D"].view(np.uint64), Do.view(np.uint64)), knob
    assert r["cnt"]["overflow"] == 0
    if dense:
        # branches handed to the search and the assembly: more than the grouped search finished itself, and
        # more dirty segments than its 32-segment lists take in the window's wave
        assert r["cnt"]["coop_tasks"] > r["cnt"]["search_finished"] and r["cnt"]["coop_tasks"] > 3 * 32, r["cnt"]
print("ok")
'''


def _run(cfg, n, seed, base, dense=False, cap=0):
    code = _CODE % dict(root=_ROOT, tests=_TESTS, cfg=cfg, n=n, seed=seed, base=base, dense=dense, cap=cap)
    e = dict(os.environ, EPV_FUSED_PHASE="1")
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.parametrize("cfg", ["tree", "pair"])
@pytest.mark.parametrize("n", [193, 1000])
def test_trees_and_path_selection(cfg, n):
    _run(cfg, n, 29, 0)


@pytest.mark.parametrize("cfg,n", [("tree", 193), ("tree", 1000), ("pair", 1000)])
@pytest.mark.parametrize("seed", SEEDS)
def test_seeds_and_sweeps_that_wrap_the_round_keys(cfg, n, seed):
    _run(cfg, n, seed, SWEEP_BASE)


@pytest.mark.parametrize("seed", [31, SEEDS[0]])
def test_pool_rounds_on_a_dense_window(seed):
    _run("tree", DENSE_N, seed, 0 if seed == 31 else SWEEP_BASE, dense=True, cap=DENSE_CAP)


def test_device_philox_blocks_equal_the_oracle():
    """every form of epv_keyed_block (inline-asm multiplies, plain ones, plain ones at call sites with
    compile-time zeros) against orc_kat_keyed_block, for zero and non-zero trial, segment and block"""
    import orc
    from epievo_amd.sampler import DeviceSampler
    L = orc.orc_lib()
    ctr = np.array([(site, sweep, b, k, t, blk)
                    for site in (0, 1, 12345, 0xFFFFFFFF) for sweep in (0, 7, 0xFFFFFFFF)
                    for b in (0, 1, 4095) for k in (0, 3, 4095) for t in (0, 1, 0xFFFFFFFF)
                    for blk in (0, 1, 255)], dtype=np.uint32)
    d = DeviceSampler(0)
    try:
        for seed in (0,) + SEEDS:
            got = d.philox_kat(seed, ctr)
            want = np.zeros((len(ctr), 2))
            two = np.zeros(2)
            for i, row in enumerate(ctr):
                L.orc_kat_keyed_block(seed, *[int(x) for x in row], orc._p(two, C.c_double))
                want[i] = two
            for form in range(3):
                assert np.array_equal(got[:, form].view(np.uint64), want.view(np.uint64)), (hex(seed), form)
    finally:
        d.close()
