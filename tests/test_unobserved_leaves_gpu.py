"""Missing leaf data on the GPU (epv_set_unobserved): an unobserved leaf cell is marginalised in the
proposal, so the chain resamples its end state; everything else is today's sampler."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
from common import simulate, ref_test_model, TEST_PARAM_TEXT, TREE_NWK_TEXT
from epievo_amd import _build, host
from epievo_amd.sampler import DeviceSampler, EpvError
from test_unobserved_leaves import leaf_ends, write_states, leaves
import test_mcmc_posterior as post
from leaf_law import MISSING, TRIALS, _exact_completions, _mixture      # noqa: F401

pytestmark = pytest.mark.gpu


def _dev(tree, model, fp, cap=None, opts=None):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap or int(max(16, 2 * fp.counts().max() + 8)))
    if opts:
        d.set_options(**opts)
    return d


def _mask(tree, n, frac, seed):
    """a random fraction of the leaf cells flagged, [N-1, n]"""
    rng = np.random.default_rng(seed)
    m = np.zeros((tree.n_nodes - 1, n), np.uint8)
    for b in range(1, tree.n_nodes):
        if tree.subtree_sizes[b] == 1:
            m[b - 1] = rng.random(n) < frac
    return m


def _run(d, burn=2, batch=3, seed=19):
    d.reset()
    J, D, nacc = d.run_mcmc(burn, batch, seed, sweep_base=4)
    return J, D, nacc, d.paths(), d.tri_llh(), d.phase_plan()["word"]


def _same(a, b):
    assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert orc.paths_equal(a[3], b[3])
    assert np.array_equal(a[4].view(np.uint64), b[4].view(np.uint64))
    assert a[5] == b[5]


@pytest.mark.parametrize("cfg,n,propose", [("tree", 3000, "fused"), ("bal16", 2000, "V3")])
def test_an_empty_mask_changes_nothing(cfg, n, propose):
    model, tree, fp = simulate(cfg, n, seed=6)
    base = _dev(tree, model, fp)
    assert base.phase_plan()["propose"] == propose
    ref = _run(base)
    zeros = _dev(tree, model, fp)
    zeros.set_unobserved(np.zeros((tree.n_nodes - 1, n), np.uint8))
    assert zeros.unobserved_cells() == 0
    _same(_run(zeros), ref)
    cleared = _dev(tree, model, fp)
    cleared.set_unobserved(_mask(tree, n, 0.1, 1))
    assert cleared.unobserved_cells() > 0 and cleared.phase_plan()["unobs"]
    cleared.set_unobserved(None)
    assert cleared.unobserved_cells() == 0
    _same(_run(cleared), ref)


@pytest.mark.parametrize("cfg,n,gpool,opts", [("tree", 3000, False, {}), ("bal16", 2000, True, {}),
                                              ("tree", 3000, False, {"reference_proposal_ratio": True})])
def test_one_unobserved_cell_takes_the_first_kernel(cfg, n, gpool, opts):
    model, tree, fp = simulate(cfg, n, seed=6)
    d = _dev(tree, model, fp, opts=opts)
    m = np.zeros((tree.n_nodes - 1, n), np.uint8)
    leaf = [b for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1][0]
    m[leaf - 1, n // 2] = 1
    d.set_unobserved(m)
    assert d.unobserved_cells() == 1
    plan = d.phase_plan()
    assert d.phase_mode() == 0 and plan["propose"] == "V1" and plan["word"] >> 17 & 1
    assert plan["gpool"] == gpool and plan["refq"] == bool(opts)
    d.reset()
    d.run_mcmc(1, 2, 5)


def test_observed_leaves_stay_pinned_and_unobserved_ones_move():
    model, tree, fp = simulate("tree", 3000, seed=6)
    n = fp.n_sites
    m = _mask(tree, n, 0.2, 2)
    m[:, 0] = m[:, -1] = 1
    for b in range(1, tree.n_nodes):
        if tree.subtree_sizes[b] != 1:
            m[b - 1] = 0
    d = _dev(tree, model, fp)
    d.set_unobserved(m)
    d.reset()
    d.run_mcmc(10, 50, 7)
    before, after = leaf_ends(tree, fp)[1:], leaf_ends(tree, d.paths())[1:]
    leaf_rows = tree.subtree_sizes[1:] == 1
    obs = (m == 0) & leaf_rows[:, None]
    assert np.array_equal(after[obs], before[obs])
    inner = (m != 0).copy()
    inner[:, [0, -1]] = False
    changed = (after != before) & inner
    assert changed.sum() > 0.05 * inner.sum(), (changed.sum(), inner.sum())
    assert np.array_equal(after[:, [0, -1]], before[:, [0, -1]])


def test_both_ratio_modes_give_the_same_chain_under_the_mask():
    model, tree, fp = simulate("tree", 3000, seed=8)
    m = _mask(tree, fp.n_sites, 0.2, 3)
    out = []
    for opts in ({}, {"reference_proposal_ratio": True}):
        d = _dev(tree, model, fp, opts=opts)
        d.set_unobserved(m)
        d.reset()
        J, D, nacc = d.run_mcmc(5, 20, 31)
        out.append((J, D, nacc, d.paths()))
    assert out[0][2] == out[1][2] and np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert orc.paths_equal(out[0][3], out[1][3])


# ------------------------------------------------------------------ the exact posterior
# test_mcmc_posterior's 14-site tree case; two leaf cells unobserved: (D, 3) where leaf D flips, and
# (C, 6) where nothing does.  The target mixes the exact posterior of each completion of the two cells,
# weighted by how many of a fixed number of forward simulations each completion keeps (leaf_law.py).

@pytest.fixture(scope="module")
def exact_case():
    model = ref_test_model()
    tree, leaf, fp = post._tree_case()
    kept, mom = _exact_completions(model, tree, leaf)
    # (no evidence: every completion weighs what the simulations kept, and the effective count is their total)
    return model, tree, leaf, fp, _mixture(kept, mom, None)


@pytest.mark.parametrize("seed,opts", [(21, {}), (22, {}), (23, {}), (24, {"forward_rejection": True})])
def test_chain_matches_the_exact_posterior_with_unobserved_cells(exact_case, seed, opts):
    model, tree, leaf, fp, (exact, p1, kept) = exact_case
    n = len(post.TROOT)
    m = np.zeros((tree.n_nodes - 1, n), np.uint8)
    for name, s in MISSING:
        m[tree.node_names.index(name) - 1, s] = 1
    d = _dev(tree, model, fp, cap=32, opts=opts)
    d.set_unobserved(m)
    d.enable_path_average(2)
    d.reset()
    J, D, nacc = d.run_mcmc(300, 12000, seed)
    post._check_tree(J, D, 1200.0, exact, tree, want=kept)
    ns, avg = d.path_average()
    _, first, _ = d.path_average_layout()
    assert ns == 12000
    for i, (name, s) in enumerate(MISSING):
        pc = avg[tree.node_names.index(name) - 1, s - first, 1]
        sig = np.sqrt(max(p1[i] * (1 - p1[i]), 1e-4) * (1.0 / kept + 1.0 / 1200.0))
        assert abs(pc - p1[i]) < 5 * sig + 1e-3, (name, s, pc, p1[i], sig)
    # every observed leaf cell still carries its data
    es = leaf_ends(tree, d.paths())
    for b in range(1, tree.n_nodes):
        if tree.subtree_sizes[b] == 1:
            keep = m[b - 1] == 0
            assert np.array_equal(es[b][keep], leaf[b][keep])


# ------------------------------------------------------------------ the C++ driver
def test_sharded_driver_under_the_mask_equals_one_context(monkeypatch):
    from epievo_amd import driver
    monkeypatch.setenv("EPV_ROW_BLOCKS", "4")
    model, tree, fp = simulate("tree", 40000, seed=12)
    m = _mask(tree, fp.n_sites, 0.15, 4)
    d = _dev(tree, model, fp, cap=16)
    d.set_unobserved(m)
    exp = []
    for it in range(2):
        d.reset()
        J, D, nacc = d.run_mcmc(1, 2, 99, sweep_base=it * 3)
        exp.append((J, D, nacc / float(2 * (fp.n_sites - 2))))
    exp_paths = d.paths()
    for devices in ([0], [0, 0, 0]):
        s = driver.CppSampler(1, 2, devices=devices, capacity=16)
        s.set_unobserved(m)                # before the first reset: must reach every part build() makes
        s.reset(model, tree, fp)
        assert s.layout()["parts_here"] > 1
        for it in range(2):
            if it:
                s.reset(model)             # keeps the mask
            J, D, acc = s.run_mcmc(99, it)
            assert np.array_equal(J, exp[it][0]) and np.array_equal(D, exp[it][1]) and acc == exp[it][2], devices
        assert orc.paths_equal(s.paths(), exp_paths), devices
        assert s.phase_mode() == 0
        s.close()


def test_mask_lifecycle_and_errors():
    model, tree, fp = simulate("tree", 3000, seed=6)
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.B, d.n_sites = tree.n_nodes - 1, fp.n_sites
    with pytest.raises(EpvError) as e:          # no paths yet
        d.set_unobserved(np.ones((tree.n_nodes - 1, fp.n_sites), np.uint8))
    assert e.value.code == 4                    # EPV_ERR_STATE
    d.upload_paths(fp, 16)
    default = d.phase_plan()["word"]
    internal = [b for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] > 1][0]
    m = np.zeros((tree.n_nodes - 1, fp.n_sites), np.uint8)
    m[internal - 1, 100] = 1
    with pytest.raises(EpvError) as e:
        d.set_unobserved(m)
    assert e.value.code == 1 and "branch %d" % internal in str(e.value)   # EPV_ERR_ARG
    assert d.unobserved_cells() == 0
    with pytest.raises(ValueError):
        d.set_unobserved(np.ones(5, np.uint8))
    ok = _mask(tree, fp.n_sites, 0.1, 5)
    d.set_unobserved(ok)
    assert d.unobserved_cells() == int(ok.sum()) and d.phase_plan()["word"] != default
    d.set_capacity(32)                          # kept
    assert d.unobserved_cells() == int(ok.sum())
    d.reset()
    d.run_mcmc(1, 1, 3)
    d.upload_paths(fp, 16)                      # new paths, new data: cleared
    assert d.unobserved_cells() == 0 and d.phase_plan()["word"] == default
    from epievo_amd import driver
    s = driver.CppSampler(1, 1, devices=[0], capacity=16)
    s.set_unobserved(np.ones((tree.n_nodes - 1, fp.n_sites + 1), np.uint8))
    with pytest.raises(driver.DriverError):     # length differs from the genome of the reset
        s.reset(model, tree, fp)
    s.close()


# ------------------------------------------------------------------ the programs
def test_cli_missing_cells_end_to_end(tmp_path):
    d = str(tmp_path)
    model, tree, fp = simulate("tree", 600, seed=5)
    open(d + "/p.param", "w").write(TEST_PARAM_TEXT)
    open(d + "/t.nwk", "w").write(TREE_NWK_TEXT)
    host.write_paths(d + "/in.paths", tree.node_names, tree.branches, fp)
    ends = leaf_ends(tree, fp)
    rng = np.random.default_rng(9)
    miss = [(c, s) for c in leaves(tree) for s in range(1, fp.n_sites - 1) if rng.random() < 0.3]
    write_states(d + "/m.states", tree, leaves(tree), ends, missing=miss)
    bin_ = _build.BIN_DIR
    r = subprocess.run([os.path.join(bin_, "epievo_est_histories"), "-B", "20", "-L", "20", "-s", "3", "-v",
                        "-o", d + "/out.paths", "-m", d + "/m.states", "-a", d + "/avg", "-n", "2",
                        d + "/p.param", d + "/t.nwk", d + "/in.paths"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "[UNOBSERVED LEAF CELLS: %d of %d]" % (len(miss), len(leaves(tree)) * fp.n_sites) in r.stderr
    out, names, _ = host.read_paths(d + "/out.paths")
    es = leaf_ends(tree, out)
    missing = set(miss)
    moved = 0
    for c in leaves(tree):
        b = tree.node_names.index(c)
        for s in range(fp.n_sites):
            if (c, s) in missing:
                moved += es[b, s] != ends[b, s]
            else:
                assert es[b, s] == ends[b, s], (c, s)
    assert moved > 0
    # the average (2 points: branch start and end): at an observed leaf cell the end is exactly the data
    avg, node = {}, None
    for line in open(d + "/avg"):
        if line.startswith("NODE:"):
            node = line[5:].split("\t")[0].strip()
            avg[node] = []
        else:
            avg[node].append([float(x) for x in line.split()])
    for c in leaves(tree):
        b = tree.node_names.index(c)
        a = np.array(avg[c])
        assert a.shape == (fp.n_sites, 2)
        obs = np.array([(c, s) not in missing for s in range(fp.n_sites)])
        assert np.array_equal(a[obs, 1], ends[b, obs].astype(np.float64))
        assert np.any((a[~obs, 1] > 0) & (a[~obs, 1] < 1))
    r2 = subprocess.run([os.path.join(bin_, "epievo_est_params_histories"), "-i", "2", "-B", "3", "-L", "2", "-s", "4",
                         "-o", d + "/o2.paths", "-p", d + "/o2.param", "-m", d + "/m.states",
                         d + "/p.param", d + "/t.nwk", d + "/in.paths"], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr
    assert os.path.getsize(d + "/o2.param") > 0
