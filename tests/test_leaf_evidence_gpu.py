"""Leaf evidence on the GPU (epv_set_leaf_evidence): a leaf cell with r = P(state 1 | its own observation)
starts Felsenstein pruning from (1 - r, r).  r = 0 / 1 is today's data and r = 0.5 today's unobserved cell,
bit for bit; in between the chain follows the exact posterior under the evidence."""
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
from test_unobserved_leaves_gpu import _dev, _mask, _run, _same
from leaf_law import MISSING, TRIALS, EVIDENCE, _exact_completions, _mixture, _sigma      # noqa: F401
from test_leaf_evidence import write_probs
import test_mcmc_posterior as post

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)


def _cap(fp):
    return int(max(16, 2 * fp.counts().max() + 8))


def _leaf_rows(tree):
    return tree.subtree_sizes[1:] == 1


def _data_evidence(tree, fp):
    """r = float32(leaf end state) at every leaf cell, NaN on the other branches"""
    r = np.full((tree.n_nodes - 1, fp.n_sites), NAN, np.float32)
    rows = _leaf_rows(tree)
    r[rows] = leaf_ends(tree, fp)[1:][rows].astype(np.float32)
    return r


def _same_results(a, b):
    """J, D, accept count, paths and tri_llh as uint64 (the plan word is a[5], compared where stated)"""
    assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert orc.paths_equal(a[3], b[3])
    assert np.array_equal(a[4].view(np.uint64), b[4].view(np.uint64))


# ------------------------------------------------------------------ 1. the empty table
@pytest.mark.parametrize("cfg,n,propose", [("tree", 3000, "fused"), ("bal16", 2000, "V3")])
def test_an_empty_table_changes_nothing(cfg, n, propose):
    model, tree, fp = simulate(cfg, n, seed=6)
    base = _dev(tree, model, fp)
    assert base.phase_plan()["propose"] == propose and not base.phase_plan()["evidence"]
    ref = _run(base)
    null = _dev(tree, model, fp)
    null.set_leaf_evidence(None)
    assert null.leaf_evidence_cells() == 0
    _same(_run(null), ref)
    nans = _dev(tree, model, fp)
    nans.set_leaf_evidence(np.full((tree.n_nodes - 1, n), NAN, np.float32))
    assert nans.leaf_evidence_cells() == 0
    _same(_run(nans), ref)
    cleared = _dev(tree, model, fp)
    cleared.set_leaf_evidence(_data_evidence(tree, fp))
    assert cleared.leaf_evidence_cells() == int(_leaf_rows(tree).sum()) * n and cleared.phase_plan()["evidence"]
    cleared.set_leaf_evidence(None)
    assert cleared.leaf_evidence_cells() == 0
    _same(_run(cleared), ref)


# ------------------------------------------------------------------ 2. evidence equal to the data
@pytest.mark.parametrize("cfg,n,gpool,opts", [("tree", 3000, False, {}), ("bal16", 2000, True, {}),
                                              ("tree", 3000, False, {"reference_proposal_ratio": True})])
def test_evidence_equal_to_the_data_is_the_default_run_and_the_oracle(cfg, n, gpool, opts):
    model, tree, fp = simulate(cfg, n, seed=6)
    cap = _cap(fp)
    ref = _run(_dev(tree, model, fp, cap=cap, opts=opts))
    d = _dev(tree, model, fp, cap=cap, opts=opts)
    d.set_leaf_evidence(_data_evidence(tree, fp))
    plan = d.phase_plan()
    assert d.phase_mode() == 0 and plan["propose"] == "V1" and plan["word"] >> 18 & 1 and plan["evidence"]
    assert plan["gpool"] == gpool and plan["refq"] == bool(opts) and not plan["unobs"]
    got = _run(d)
    _same_results(got, ref)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=19)
    if opts:
        o.set_proposal_mode(True)
    o.reset()
    Jo, Do, no, _ = o.run_mcmc(2, 3, sweep_base=4)
    assert got[2] == no and np.array_equal(got[0], Jo) and np.array_equal(got[1], Do)
    assert orc.paths_equal(got[3], o.paths())
    assert np.array_equal(got[4].view(np.uint64), o.tri_llh().view(np.uint64))


# ------------------------------------------------------------------ 3. evidence equal to the mask
@pytest.mark.parametrize("opts", [{}, {"reference_proposal_ratio": True}, {"forward_rejection": True}])
def test_evidence_of_one_half_is_the_mask_run(opts):
    model, tree, fp = simulate("tree", 3000, seed=8)
    m = _mask(tree, fp.n_sites, 0.2, 3)
    masked = _dev(tree, model, fp, opts=opts)
    masked.set_unobserved(m)
    ref = _run(masked, burn=5, batch=20, seed=31)
    d = _dev(tree, model, fp, opts=opts)
    d.set_leaf_evidence(np.where(m != 0, np.float32(0.5), NAN).astype(np.float32))
    assert d.leaf_evidence_cells() == int(m.sum()) and d.unobserved_cells() == 0
    _same_results(_run(d, burn=5, batch=20, seed=31), ref)
    # (the chain did move leaf states, so the comparison saw the new code)
    assert not np.array_equal(leaf_ends(tree, ref[3]), leaf_ends(tree, fp))


# ------------------------------------------------------------------ 4. precedence
@pytest.mark.parametrize("opts", [{}, {"reference_proposal_ratio": True}])
def test_evidence_wins_over_the_mask(opts):
    model, tree, fp = simulate("tree", 3000, seed=8)
    n = fp.n_sites
    a, b = _mask(tree, n, 0.15, 5), _mask(tree, n, 0.15, 6)
    b[a != 0] = 0                                   # A and B disjoint
    only_a = _dev(tree, model, fp, opts=opts)
    only_a.set_unobserved(a)
    ref = _run(only_a, burn=5, batch=20, seed=31)
    d = _dev(tree, model, fp, opts=opts)
    d.set_unobserved(a | b)
    r = np.where(b != 0, leaf_ends(tree, fp)[1:].astype(np.float32), NAN).astype(np.float32)
    d.set_leaf_evidence(r)
    assert d.unobserved_cells() == int((a | b).sum()) and d.leaf_evidence_cells() == int(b.sum())
    plan = d.phase_plan()
    assert plan["unobs"] and plan["evidence"] and plan["propose"] == "V1"
    _same_results(_run(d, burn=5, batch=20, seed=31), ref)
    # the cells of B are pinned: the mask alone on A u B walks another chain
    both = _dev(tree, model, fp, opts=opts)
    both.set_unobserved(a | b)
    other = _run(both, burn=5, batch=20, seed=31)
    assert not orc.paths_equal(other[3], ref[3])


# ------------------------------------------------------------------ the law
# test_mcmc_posterior's 14-site tree case with the two cells of test_unobserved_leaves_gpu: (D, 3) and (C, 6).
# The target mixes the exact posterior of each completion c of the two cells with weight kept_c * e_c, where
# kept_c is what a fixed number of forward simulations keeps (the prior weight of the completion's data) and
# e_c = prod (r_i or 1 - r_i) the evidence.  Standard errors come from the reference's counts alone: the Kish
# effective count (sum k_c e_c)^2 / sum k_c e_c^2 stands where the number of kept draws does for one target.
# The target lives in leaf_law.py, which computes the completions once per process.


@pytest.fixture(scope="module")
def exact_case():
    model = ref_test_model()
    tree, leaf, fp = post._tree_case()
    kept, mom = _exact_completions(model, tree, leaf)
    print("kept per completion", kept)
    return model, tree, leaf, fp, _mixture(kept, mom, EVIDENCE), _mixture(kept, mom, None)


def test_the_evidence_moves_the_target_away_from_the_mask(exact_case):
    """what makes the test below mean something: under the evidence each soft cell's exact probability is at
    least 10 of the test's sigma away from its value under the plain mask"""
    model, tree, leaf, fp, (exact, p1, kish), (_, p1_mask, _) = exact_case
    for i, (name, s) in enumerate(MISSING):
        sig = _sigma(p1[i], kish)
        print(name, s, "mask", p1_mask[i], "evidence", p1[i], "sigma", sig, "kish", kish)
        assert abs(p1[i] - p1_mask[i]) >= 10 * sig, (name, s, p1[i], p1_mask[i], sig)


@pytest.mark.parametrize("seed,opts", [(21, {}), (22, {}), (23, {}), (24, {"forward_rejection": True}),
                                       (25, {"reference_proposal_ratio": True})])
def test_chain_matches_the_exact_posterior_under_leaf_evidence(exact_case, seed, opts):
    """(the reference-ratio case: without the target's leaf factor in the ratio that mode follows the mask's
    law)"""
    model, tree, leaf, fp, (exact, p1, kish), _ = exact_case
    n = len(post.TROOT)
    r = np.full((tree.n_nodes - 1, n), NAN, np.float32)
    for (name, s), ri in zip(MISSING, EVIDENCE):
        r[tree.node_names.index(name) - 1, s] = ri
    d = _dev(tree, model, fp, cap=32, opts=opts)
    d.set_leaf_evidence(r)
    d.enable_path_average(2)
    d.reset()
    J, D, nacc = d.run_mcmc(300, 12000, seed)
    Jm, Dm, Jse, Dse = exact
    print("max |J - exact|", np.abs(J - Jm).max(), "max |D - exact|", np.abs(D - Dm).max())
    post._check_tree(J, D, 1200.0, exact, tree, want=kish)
    ns, avg = d.path_average()
    _, first, _ = d.path_average_layout()
    assert ns == 12000
    for i, (name, s) in enumerate(MISSING):
        pc = avg[tree.node_names.index(name) - 1, s - first, 1]
        sig = _sigma(p1[i], kish)
        print(name, s, "chain", pc, "exact", p1[i], "sigma", sig)
        assert abs(pc - p1[i]) < 5 * sig + 1e-3, (name, s, pc, p1[i], sig)
    # every other leaf cell still carries its data
    es = leaf_ends(tree, d.paths())
    for b in range(1, tree.n_nodes):
        if tree.subtree_sizes[b] == 1:
            keep = np.isnan(r[b - 1])
            assert np.array_equal(es[b][keep], leaf[b][keep])


# ------------------------------------------------------------------ 5. the C++ driver
def _random_evidence(tree, n, frac, seed):
    rng = np.random.default_rng(seed)
    r = np.full((tree.n_nodes - 1, n), NAN, np.float32)
    for b in range(1, tree.n_nodes):
        if tree.subtree_sizes[b] == 1:
            pick = rng.random(n) < frac
            r[b - 1, pick] = rng.random(int(pick.sum())).astype(np.float32)
    return r


def test_sharded_driver_under_evidence_equals_one_context(monkeypatch):
    from epievo_amd import driver
    monkeypatch.setenv("EPV_ROW_BLOCKS", "4")
    model, tree, fp = simulate("tree", 40000, seed=12)
    r = _random_evidence(tree, fp.n_sites, 0.15, 4)
    d = _dev(tree, model, fp, cap=16)
    d.set_leaf_evidence(r)
    exp = []
    for it in range(2):
        d.reset()
        J, D, nacc = d.run_mcmc(1, 2, 99, sweep_base=it * 3)
        exp.append((J, D, nacc / float(2 * (fp.n_sites - 2))))
    exp_paths = d.paths()
    assert not np.array_equal(leaf_ends(tree, exp_paths), leaf_ends(tree, fp))
    for devices in ([0], [0, 0, 0]):
        s = driver.CppSampler(1, 2, devices=devices, capacity=16)
        s.set_leaf_evidence(r)             # before the first reset: must reach every part build() makes
        s.reset(model, tree, fp)
        assert s.layout()["parts_here"] > 1
        for it in range(2):
            if it:
                s.reset(model)             # keeps the table
            J, D, acc = s.run_mcmc(99, it)
            assert np.array_equal(J, exp[it][0]) and np.array_equal(D, exp[it][1]) and acc == exp[it][2], devices
        assert orc.paths_equal(s.paths(), exp_paths), devices
        assert s.phase_mode() == 0
        s.close()


# ------------------------------------------------------------------ 6. life cycle and errors
def test_evidence_lifecycle_and_errors():
    model, tree, fp = simulate("tree", 3000, seed=6)
    B, n = tree.n_nodes - 1, fp.n_sites
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.B, d.n_sites = B, n
    with pytest.raises(EpvError) as e:          # no paths yet
        d.set_leaf_evidence(np.full((B, n), 0.5, np.float32))
    assert e.value.code == 4                    # EPV_ERR_STATE
    d.upload_paths(fp, 16)
    default = d.phase_plan()["word"]
    internal = [b for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] > 1][0]
    leaf = [b for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1][1]
    r = np.full((B, n), NAN, np.float32)
    r[internal - 1, 100] = 0.5
    with pytest.raises(EpvError) as e:
        d.set_leaf_evidence(r)
    assert e.value.code == 1 and "branch %d at site 100" % internal in str(e.value)   # EPV_ERR_ARG
    for bad in (1.5, -0.25, np.inf, -np.inf):
        r = np.full((B, n), NAN, np.float32)
        r[leaf - 1, 77] = bad
        with pytest.raises(EpvError) as e:
            d.set_leaf_evidence(r)
        assert e.value.code == 1 and "branch %d at site 77" % leaf in str(e.value), bad
    assert d.leaf_evidence_cells() == 0 and d.phase_plan()["word"] == default
    with pytest.raises(ValueError):
        d.set_leaf_evidence(np.ones(5, np.float32))
    ok = _random_evidence(tree, n, 0.1, 5)
    k = int((~np.isnan(ok)).sum())
    d.set_leaf_evidence(ok)
    assert d.leaf_evidence_cells() == k
    assert d.phase_plan()["word"] != default and d.phase_plan()["evidence"] and d.phase_mode() == 0
    d.set_capacity(32)                          # kept
    assert d.leaf_evidence_cells() == k
    d.reset()
    d.run_mcmc(1, 1, 3)
    assert d.leaf_evidence_cells() == k         # kept by reset and the run
    d.set_model(model)
    assert d.leaf_evidence_cells() == k
    d.upload_paths(fp, 16)                      # new paths, new data: cleared
    assert d.leaf_evidence_cells() == 0 and d.phase_plan()["word"] == default
    from epievo_amd import driver
    s = driver.CppSampler(1, 1, devices=[0], capacity=16)
    s.set_leaf_evidence(np.full((B, n + 1), 0.5, np.float32))
    with pytest.raises(driver.DriverError):     # length differs from the genome of the reset
        s.reset(model, tree, fp)
    s.close()


def test_python_mirror_reapplies_the_table_after_an_upload():
    from epievo_amd.sampler import SingleSiteSampler
    model, tree, fp = simulate("tree", 3000, seed=6)
    r = _random_evidence(tree, fp.n_sites, 0.1, 5)
    k = int((~np.isnan(r)).sum())
    s = SingleSiteSampler(1, 2, capacity=16)
    s.set_leaf_evidence(r)                      # before paths: held back
    s.reset(model, tree, fp)
    assert s.dev.leaf_evidence_cells() == k
    s.reset(model, tree, fp)                    # the upload clears the device table, the mirror puts it back
    assert s.dev.leaf_evidence_cells() == k and s.dev.phase_plan()["evidence"]
    s.set_leaf_evidence(None)
    assert s.dev.leaf_evidence_cells() == 0


# ------------------------------------------------------------------ 7. the programs
def _read_average(path):
    avg, node = {}, None
    for line in open(path):
        if line.startswith("NODE:"):
            node = line[5:].split("\t")[0].strip()
            avg[node] = []
        else:
            avg[node].append([float(x) for x in line.split()])
    return {k: np.array(v) for k, v in avg.items()}


def _est_histories(d, tag, *extra):
    return subprocess.run([os.path.join(_build.BIN_DIR, "epievo_est_histories"), "-B", "20", "-L", "20", "-s", "3", "-v",
                           "-o", d + "/%s.paths" % tag, "-a", d + "/%s.avg" % tag, "-n", "2"] + list(extra) +
                          [d + "/p.param", d + "/t.nwk", d + "/in.paths"], capture_output=True, text=True, timeout=300)


def test_cli_leaf_probs_end_to_end(tmp_path):
    d = str(tmp_path)
    model, tree, fp = simulate("tree", 600, seed=5)
    open(d + "/p.param", "w").write(TEST_PARAM_TEXT)
    open(d + "/t.nwk", "w").write(TREE_NWK_TEXT)
    host.write_paths(d + "/in.paths", tree.node_names, tree.branches, fp)
    ends = leaf_ends(tree, fp)
    rng = np.random.default_rng(9)
    cells = [(c, s) for c in leaves(tree) for s in range(1, fp.n_sites - 1) if rng.random() < 0.3]
    n_leaf_cells = len(leaves(tree)) * fp.n_sites
    # a file of 0 / 1 / N is the -m run of the same seed, byte for byte
    write_states(d + "/m.states", tree, leaves(tree), ends, missing=cells)
    write_probs(d + "/n.probs", tree, leaves(tree), ends, {c: "N" for c in cells})
    rm = _est_histories(d, "m", "-m", d + "/m.states")
    rn = _est_histories(d, "n", "-l", d + "/n.probs")
    assert rm.returncode == 0 and rn.returncode == 0, rm.stderr + rn.stderr
    assert "[LEAF CELLS WITH EVIDENCE: %d of %d]" % (len(cells), n_leaf_cells) in rn.stderr
    assert open(d + "/m.paths", "rb").read() == open(d + "/n.paths", "rb").read()
    assert open(d + "/m.avg", "rb").read() == open(d + "/n.avg", "rb").read()
    # soft cells
    soft = {c: "%.6f" % rng.uniform(0.05, 0.95) for c in cells}
    write_probs(d + "/s.probs", tree, leaves(tree), ends, soft)
    rs = _est_histories(d, "s", "-l", d + "/s.probs")
    assert rs.returncode == 0, rs.stderr
    assert "[LEAF CELLS WITH EVIDENCE: %d of %d]" % (len(cells), n_leaf_cells) in rs.stderr
    out, names, _ = host.read_paths(d + "/s.paths")
    es = leaf_ends(tree, out)
    avg = _read_average(d + "/s.avg")
    inside = 0
    for c in leaves(tree):
        b = tree.node_names.index(c)
        hard = np.array([(c, s) not in soft for s in range(fp.n_sites)])
        assert np.array_equal(es[b, hard], ends[b, hard]), c          # every 0/1 cell ends at its data
        a = avg[c]
        assert a.shape == (fp.n_sites, 2)
        assert np.array_equal(a[hard, 1], ends[b, hard].astype(np.float64))
        inside += int(np.sum((a[~hard, 1] > 0) & (a[~hard, 1] < 1)))
    assert inside > 0
    r2 = subprocess.run([os.path.join(_build.BIN_DIR, "epievo_est_params_histories"), "-i", "2", "-B", "3", "-L", "2",
                         "-s", "4", "-o", d + "/o2.paths", "-p", d + "/o2.param", "-l", d + "/s.probs",
                         d + "/p.param", d + "/t.nwk", d + "/in.paths"], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr
    assert os.path.getsize(d + "/o2.param") > 0
