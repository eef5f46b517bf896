"""Dense histories on the CPU (dense_cases.py): the inputs of test_dense_histories_gpu.py are what they claim to
be, and the oracle itself is pinned on them -- rung B's exact statistics to a walk over the paths in plain
Python, rung A to the linked reference, rung B to rung A statistically.  Until now rung A was pinned to the
reference on the fuzz range only and rung B to rung A on test.param inputs only: paths of two or three jumps."""
import numpy as np
import pytest

import dense_cases as dc
import orc
import refvec

TABLE = [w for w in dc.WORKLOADS if dc.WORKLOADS[w][3] <= 1000]


@pytest.mark.parametrize("name", TABLE)
def test_row_preconditions(name):
    """a change in host.simulate cannot quietly turn a dense row sparse: every label of the row holds on the
    generated input, and the oracle accepts some proposals but not all (weak), or all (flat).  The thresholds
    are conditions, not measurements; the measured values are in the table of dense_cases."""
    model_name, _, _, n, labels = dc.WORKLOADS[name]
    _, tree, fp = dc.workload(name)
    dens = dc.density(fp)
    cap = dc.capacity(name, fp)
    if "fused" in labels:
        assert cap == 31 and dc.words(cap) == 1 and dens["mean"] >= 2.0, dens
        assert dens["max"] <= cap
    if "w2" in labels:
        assert 2 * cap + 1 > 64 and dc.words(cap) >= 2, cap
    if "over64" in labels:
        assert dens["over64"] >= 0.03, dens
    else:
        assert dens["over64"] < 0.03, dens
    if "both" in labels:
        assert 1.0 - dens["over64"] >= 0.03, dens
    o = dc.oracle(name, cap)
    _, _, nacc, acc = o.run_mcmc(2, 3, sweep_base=4)
    assert o.counters()["overflow"] == 0
    if model_name == "flat":
        assert nacc == 3 * (n - 2)
    else:
        assert 0.02 < acc < 0.98, acc


def test_one_row_exercises_both_list_routes():
    assert any("both" in dc.WORKLOADS[w][4] for w in TABLE)


@pytest.mark.parametrize("name", dc.OVERFLOW)
def test_overflow_rows_overflow(name):
    _, _, fp = dc.workload(name)
    o = dc.oracle(name, dc.capacity(name, fp, "tight"))
    for w in range(4, 9):
        o.sweep(w)
    assert o.counters()["overflow"] >= 1


@pytest.mark.parametrize("name", sorted(dc.MIXED))
def test_mixed_rows_are_sparse_on_average_and_dense_in_the_window(name):
    """thin() keeps the data and the window: the same leaf states, a mean jump count well below the base
    workload's, and inside the window the base workload's own K"""
    base, lo, hi = dc.MIXED[name]
    _, tree, fp0 = dc.workload(base)
    _, _, fp = dc.workload(name)
    B, n = fp.n_nodes - 1, fp.n_sites
    assert np.array_equal(fp.init, fp0.init) and np.array_equal(fp.counts() & 1, fp0.counts() & 1)
    nj, nj0 = fp.counts().reshape(B, n), fp0.counts().reshape(B, n)
    assert np.array_equal(nj[:, lo:hi + 1], nj0[:, lo:hi + 1]) and nj[:, :lo].max() <= 1 and nj[:, hi + 1:].max() <= 1
    assert fp.counts().mean() < 0.5 * fp0.counts().mean()
    off, off0 = fp.offsets.astype(np.int64), fp0.offsets.astype(np.int64)
    for e in range(B * n):
        assert np.array_equal(fp.jumps[off[e]:off[e + 1]], fp0.jumps[off0[e]:off0[e] + off[e + 1] - off[e]])
    K = nj[:, :-2] + nj[:, 2:] + 1
    if "over64" in dc.WORKLOADS[base][4]:
        assert (K > 64).sum() >= 1 and (K <= 64).sum() >= 1
    o = dc.oracle(name, dc.capacity(name, fp))
    _, _, _, acc = o.run_mcmc(2, 3, sweep_base=4)
    assert 0.02 < acc < 0.98 and o.counters()["overflow"] == 0
    assert o.paths().counts().mean() > 2.0 * fp.counts().mean()      # the chain fills the sparse sites in


@pytest.mark.parametrize("name", ["weak-tree150", "weak-pair40", "flat-bal16x300"])
def test_yardstick_against_rung_b(name):
    """J as integers; D per (branch, context) within the bound dense_cases.dwell_bound derives: the number of
    intervals summed into the cell times half a quantum 2^-k_b (each interval is rounded to a multiple of the
    quantum once, and nothing else about the integer sum is inexact), plus 1e-12 relative for the one fp64
    subtraction per interval and the one int64 -> double conversion per cell -- the tolerance
    test_exact_stats.py already uses between the integer and the fp64 sums."""
    _, tree, fp = dc.workload(name)
    o = dc.oracle(name, dc.capacity(name, fp))
    for w in range(3):
        o.sweep(w)
    J, D = o.suffstats()
    B = tree.n_nodes - 1
    Jy, Dy, n_int = dc.yardstick(o.paths(), tree.branches)
    assert np.array_equal(J, J.astype(np.int64)) and np.array_equal(J.astype(np.int64).reshape(B, 8), Jy)
    bound = dc.dwell_bound(n_int, Dy, dc.stat_scales(o))
    err = np.abs(D.reshape(B, 8) - Dy)
    assert np.all(err <= bound), float((err / bound).max())
    # the yardstick is not vacuous: cells hold thousands of intervals, and time is conserved
    assert n_int.max() > 1000
    np.testing.assert_allclose(Dy.sum(axis=1), (fp.n_sites - 2) * tree.branches[1:], rtol=1e-12)


def test_yardstick_on_a_hand_made_triple():
    """three sites, one branch of length 1: left 0 jumps at 0.25, middle 1 jumps at 0.5 and 0.75, right 0 stays"""
    from epievo_amd import host
    fp = host.FlatPaths(3, 2, [0, 1, 0], [0, 1, 3, 3], [0.25, 0.5, 0.75])
    J, D, n_int = dc.yardstick(fp, np.array([0.0, 1.0]))
    wantD, wantJ = np.zeros(8), np.zeros(8, np.int64)
    wantD[0b010], wantD[0b110], wantD[0b100] = 0.25 + 0.0, 0.25 + 0.25, 0.25     # 010 -> 110 -> 100 -> 110
    wantJ[0b110], wantJ[0b100] = 1, 1
    assert np.array_equal(D[0], wantD) and np.array_equal(J[0], wantJ) and n_int.sum() == 4


@pytest.mark.parametrize("name,workload", [("dense_pair", "weak-pair10"), ("dense_tree", "weak-tree100")])
def test_rung_a_vs_linked_reference_on_dense_input(name, workload):
    """the reference-schedule rung against the LINKED reference, live (against its stored outputs,
    tests/golden/ref/, where oracle/_ref is absent), on paths of ten jumps: what test_fuzz.py compares"""
    model, tree, fp = dc.workload(workload, 60)
    assert fp.counts().mean() > 4.0 and fp.counts().max() >= 15

    def reference():
        R = orc.Reference(tree, model, fp, seed=dc.ORACLE_SEED)
        R.reset(1, 2)
        llh0 = R.tri_llh()
        Jr, Dr, accr = R.run_mcmc()
        return dict(llh0=llh0, J=Jr, D=Dr, acc=np.float64(accr), **refvec.pack_paths("paths", R.paths()))

    r = refvec.reference_outputs(name, reference)
    o = orc.Oracle(tree, model, fp, "A", seed=dc.ORACLE_SEED)
    o.reset()
    assert np.array_equal(o.tri_llh(), r["llh0"])
    Jo, Do, nacc, acc = o.run_mcmc(1, 2)
    assert np.array_equal(Jo, r["J"]) and np.array_equal(Do, r["D"]) and acc == float(r["acc"])
    assert 0.0 < acc < 1.0
    assert orc.paths_equal(o.paths(), refvec.unpack_paths("paths", r))


@pytest.mark.parametrize("name", ["weak-pair10", "weak-tree100"])
def test_rung_b_chain_matches_rung_a_chain_statistically_on_dense_input(name):
    """the criteria of test_statistical.py's test_rung_b_chain_matches_rung_a_chain_statistically, unchanged"""
    model, tree, fp = dc.workload(name)
    res = {}
    for rung in ("A", "B"):
        o = orc.Oracle(tree, model, fp, rung, cap=dc.capacity(name, fp) if rung == "B" else 0, seed=1)
        o.reset()
        J, D, nacc, acc = o.run_mcmc(4, 12)
        assert rung == "A" or o.counters()["overflow"] == 0
        res[rung] = (J, D, acc)
    JA, DA, accA = res["A"]
    JB, DB, accB = res["B"]
    assert abs(accA - accB) < 0.01
    # J per (branch, context): Poisson counts averaged over 12 correlated sweeps
    sd = np.sqrt(np.maximum(JA, 1.0))
    assert np.all(np.abs(JA - JB) < 6.0 * sd + 2.0)
    # total dwell time is conserved exactly; its split over contexts fluctuates
    B = tree.n_nodes - 1
    np.testing.assert_allclose(DA.reshape(B, 8).sum(1), DB.reshape(B, 8).sum(1), rtol=1e-9)
    assert np.all(np.abs(DA - DB) < 0.05 * DA.reshape(B, 8).sum(1, keepdims=True).repeat(8, 1).reshape(-1) + 1.0)
