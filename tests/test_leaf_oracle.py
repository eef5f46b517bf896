"""The oracle's leaf vector (orc_set_unobserved, orc_set_leaf_evidence), without a GPU.

pruning() starts a leaf from (1 - r, r) where the cell holds evidence r, from (1, 1) where the mask flags it
and from the indicator of the path's end state otherwise; both rungs run that one function.  Here: the
identities that tie the three cases together, that a mask moves masked cells and only those, the law of
both rungs against the exact mixture of leaf_law.py, and what a hard cell that contradicts the resident
path does in either ratio mode.  The GPU is held to rung B bit for bit in test_leaf_matrix.py."""
import time

import numpy as np
import pytest

import orc
from common import simulate
from test_unobserved_leaves import leaf_ends
import leaf_law
import test_mcmc_posterior as post

NAN = np.float32(np.nan)
MODES = {"telescoped": dict(ref=False, sr=False), "reference": dict(ref=True, sr=False),
         "sample_root": dict(ref=True, sr=True)}


def _cap(fp):
    return int(max(16, 2 * fp.counts().max() + 8))


def _oracle(tree, model, fp, rung, mode, seed=19, mask=None, r=None):
    o = orc.Oracle(tree, model, fp, rung, cap=_cap(fp) if rung == "B" else 0, seed=seed)
    o.set_proposal_mode(MODES[mode]["ref"])
    o.set_sample_root(MODES[mode]["sr"])
    o.set_unobserved(mask)
    o.set_leaf_evidence(r)
    o.reset()
    return o


def _run(o, burn=2, batch=3):
    J, D, nacc, _ = o.run_mcmc(burn, batch, sweep_base=4)
    return J, D, nacc, o.paths(), o.tri_llh()


def _same(a, b):
    assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert orc.paths_equal(a[3], b[3])
    assert np.array_equal(a[4].view(np.uint64), b[4].view(np.uint64))


def _leaf_rows(tree):
    return tree.subtree_sizes[1:] == 1


def _mask(tree, n, frac, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((tree.n_nodes - 1, n), np.uint8)
    rows = _leaf_rows(tree)
    m[rows] = rng.random((int(rows.sum()), n)) < frac
    return m


# ------------------------------------------------------------------ identities
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("rung", ["A", "B"])
@pytest.mark.parametrize("cfg,n", [("tree", 300), ("bal16", 120)])
def test_leaf_vector_identities(cfg, n, rung, mode):
    model, tree, fp = simulate(cfg, n, seed=6)
    rows = _leaf_rows(tree)
    ends = leaf_ends(tree, fp)[1:]
    plain = _run(_oracle(tree, model, fp, rung, mode))
    # evidence equal to the data is the plain run: r = 0 / 1 is the indicator bit for bit
    data = np.full((tree.n_nodes - 1, n), NAN, np.float32)
    data[rows] = ends[rows].astype(np.float32)
    _same(_run(_oracle(tree, model, fp, rung, mode, r=data)), plain)
    # 0.5 on the cells of a mask is the mask run: (1, 1) times an exact power of two
    a, b = _mask(tree, n, 0.2, 3), _mask(tree, n, 0.2, 4)
    b[a != 0] = 0
    masked = _run(_oracle(tree, model, fp, rung, mode, mask=a))
    assert not orc.paths_equal(masked[3], plain[3])
    half = np.where(a != 0, np.float32(0.5), NAN).astype(np.float32)
    _same(_run(_oracle(tree, model, fp, rung, mode, r=half)), masked)
    # a non-NaN r wins over the mask: data on the cells of B leaves the mask of A alone
    pinned = np.where(b != 0, ends.astype(np.float32), NAN).astype(np.float32)
    _same(_run(_oracle(tree, model, fp, rung, mode, mask=a | b, r=pinned)), masked)
    assert not orc.paths_equal(_run(_oracle(tree, model, fp, rung, mode, mask=a | b))[3], masked[3])
    # clearing restores the plain run
    o = _oracle(tree, model, fp, rung, mode, mask=a | b, r=half)
    o.set_unobserved(None)
    o.set_leaf_evidence(None)
    _same(_run(o), plain)


# ------------------------------------------------------------------ the two ratio modes under soft evidence
def _soft(tree, fp, frac, seed):
    """random r in (0, 1) on a fraction of the leaf cells, extreme values among them"""
    rng = np.random.default_rng(seed)
    n = fp.n_sites
    r = np.full((tree.n_nodes - 1, n), NAN, np.float32)
    for b in np.flatnonzero(_leaf_rows(tree)):
        pick = np.flatnonzero(rng.random(n) < frac)
        r[b, pick] = (2.0 ** -20 + (1.0 - 2.0 ** -19) * rng.random(len(pick))).astype(np.float32)
        r[b, pick[:4]] = [0.02, 0.8, 2.0 ** -24, 1.0 - 2.0 ** -24]
    return r


@pytest.mark.parametrize("rung", ["A", "B"])
@pytest.mark.parametrize("cfg,n", [("tree", 300), ("bal16", 120)])
def test_both_ratio_modes_walk_the_same_chain_under_soft_evidence(cfg, n, rung):
    """q(old)/q(new) times the target's leaf factor is 1: what the reference-ratio mode evaluates is
    rounding noise, as without evidence (test_proposal_ratio.py), and the chains coincide.  Without the
    target's share the difference is log(r / (1 - r)) wherever a soft leaf cell changes state."""
    model, tree, fp = simulate(cfg, n, seed=6)
    r = _soft(tree, fp, 0.3, 11)
    tel = _oracle(tree, model, fp, rung, "telescoped", r=r)
    ref = _oracle(tree, model, fp, rung, "reference", r=r)
    a, b = _run(tel, 5, 20), _run(ref, 5, 20)
    moved = leaf_ends(tree, a[3])[1:] != leaf_ends(tree, fp)[1:]
    assert (moved & ~np.isnan(r)).sum() >= 10
    print("max |log q(old) - log q(new) + leaf factor|", ref.max_qdiff())
    assert ref.max_qdiff() < 1e-10          # the bound of test_proposal_ratio.py
    _same(a, b)


# ------------------------------------------------------------------ non-vacuity
@pytest.mark.parametrize("rung", ["A", "B"])
@pytest.mark.parametrize("cfg,n", [("tree", 300), ("bal16", 120)])
def test_a_mask_moves_masked_cells_and_no_others(cfg, n, rung):
    model, tree, fp = simulate(cfg, n, seed=6)
    m = _mask(tree, n, 0.2, 3)
    out = _run(_oracle(tree, model, fp, rung, "telescoped", mask=m))
    before, after = leaf_ends(tree, fp)[1:], leaf_ends(tree, out[3])[1:]
    rows = _leaf_rows(tree)[:, None]
    moved = (after != before) & rows
    assert (moved & (m != 0)).sum() >= 1
    assert not (moved & (m == 0)).any()
    assert not moved[:, [0, -1]].any()          # the genome's end sites are never updated


# ------------------------------------------------------------------ the law
def _chain(o, tree, burn, batch):
    """run_mcmc's averages, and the frequency of state 1 at the end of every branch over the batch sweeps"""
    B, n = tree.n_nodes - 1, o.n_sites
    for w in range(burn):
        o.sweep(w)
    J, D, p1 = np.zeros(B * 8), np.zeros(B * 8), np.zeros((B, n))
    for w in range(burn, burn + batch):
        o.sweep(w)
        j, d = o.suffstats()
        J += j
        D += d
        p1 += leaf_ends(tree, o.paths())[1:]
    return J / batch, D / batch, p1 / batch


@pytest.fixture(scope="module")
def exact_case():
    return leaf_law.exact_case()


@pytest.mark.parametrize("rung,seed", [("A", 3), ("B", 4)])
@pytest.mark.parametrize("content", ["evidence", "mask"])
def test_oracle_chains_match_the_exact_mixture(exact_case, content, rung, seed):
    """the chain of test_chain_matches_the_exact_posterior_under_leaf_evidence / _with_unobserved_cells
    (300 + 12000 sweeps, the same bounds), run by the oracle"""
    model, tree, leaf, fp, under_evidence, under_mask = exact_case
    exact, p1, kish = under_evidence if content == "evidence" else under_mask
    n = len(post.TROOT)
    o = orc.Oracle(tree, model, fp, rung, cap=32 if rung == "B" else 0, seed=seed)
    cells = [(tree.node_names.index(name) - 1, s) for name, s in leaf_law.MISSING]
    if content == "evidence":
        r = np.full((tree.n_nodes - 1, n), NAN, np.float32)
        for (b, s), ri in zip(cells, leaf_law.EVIDENCE):
            r[b, s] = ri
        o.set_leaf_evidence(r)
    else:
        m = np.zeros((tree.n_nodes - 1, n), np.uint8)
        for b, s in cells:
            m[b, s] = 1
        o.set_unobserved(m)
    o.reset()
    t0 = time.perf_counter()
    J, D, freq = _chain(o, tree, 300, 12000)
    print("chain of 12300 sweeps: %.1f s" % (time.perf_counter() - t0))
    print("max |J - exact|", np.abs(J - exact[0]).max(), "max |D - exact|", np.abs(D - exact[1]).max())
    post._check_tree(J, D, 1200.0, exact, tree, want=kish)
    for i, (b, s) in enumerate(cells):
        sig = leaf_law._sigma(p1[i], kish)
        print(leaf_law.MISSING[i], "chain", freq[b, s], "exact", p1[i], "sigma", sig)
        assert abs(freq[b, s] - p1[i]) < 5 * sig + 1e-3, (leaf_law.MISSING[i], freq[b, s], p1[i], sig)
    # every other leaf cell still carries its data
    es = leaf_ends(tree, o.paths())
    for b in range(1, tree.n_nodes):
        if tree.subtree_sizes[b] == 1:
            keep = np.array([(b - 1, s) not in cells for s in range(n)])
            assert np.array_equal(es[b][keep], leaf[b][keep])


# ------------------------------------------------------------------ a hard cell against the resident path
def contradicting_case():
    """tree.nwk, n = 600: three leaf cells (one per leaf) whose r is 0 or 1 AGAINST the path's end state.
    -> model, tree, fp, r, [(branch - 1, site, the evidence's state)]"""
    model, tree, fp = simulate("tree", 600, seed=6)
    ends = leaf_ends(tree, fp)[1:]
    leaf_b = [b - 1 for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1]
    r = np.full((tree.n_nodes - 1, fp.n_sites), NAN, np.float32)
    cells = []
    for b, s in zip(leaf_b, (33, 300, 566)):
        want = 1 - int(ends[b, s])
        r[b, s] = want
        cells.append((b, s, want))
    return model, tree, fp, r, cells


def column_changed(tree, a, b, s):
    """has the history of local site s changed between the FlatPaths a and b (any branch)"""
    B, n = tree.n_nodes - 1, a.n_sites
    for br in range(B):
        i = br * n + s
        ja, jb = a.jumps[int(a.offsets[i]):int(a.offsets[i + 1])], b.jumps[int(b.offsets[i]):int(b.offsets[i + 1])]
        if a.init[i] != b.init[i] or not np.array_equal(ja, jb):
            return True
    return False


def check_repair(tree, fp, snapshots, cells):
    """default ratio: each contradicting cell holds the evidence's state from its site's first accepted
    update on (the first sweep that changes the site's history) and never leaves it -> cells repaired"""
    done = 0
    for b, s, want in cells:
        states = [int(leaf_ends(tree, p)[1:][b, s]) for p in snapshots]
        changed = [column_changed(tree, fp, p, s) for p in snapshots]
        for w in range(len(snapshots)):
            if any(changed[:w + 1]):
                assert states[w] == want, (b, s, w, states, changed)
            else:
                assert states[w] == 1 - want, (b, s, w, states, changed)
        done += states[-1] == want
    return done


def test_contradicting_hard_cell_is_repaired_under_the_default_ratio():
    model, tree, fp, r, cells = contradicting_case()
    assert {w for _, _, w in cells} == {0, 1}          # both directions occur
    o = _oracle(tree, model, fp, "B", "telescoped", seed=29, r=r)
    snaps = []
    for w in range(5):
        o.sweep(w)
        snaps.append(o.paths())
    assert check_repair(tree, fp, snaps, cells) == len(cells)
    assert np.isfinite(o.tri_llh()[1:-1]).all()


def test_contradicting_hard_cell_under_the_reference_ratio():
    """The sums of the reference-ratio mode are not finite on such a site.  r = 1 against state 0: the
    current path's last segment has P(end 0) = PT0 * q0 / p = 0 exactly, its sum holds log(0) = -inf, the
    target's share log q[1] - log q[0] = +inf, the ratio is NaN and the update is rejected every time.
    r = 0 against state 1: the sum holds log(1 - p0) with p0 = 1 up to rounding, so -inf, NaN or the log of
    a residue of 1e-16, and the site is rejected or accepted as that rounding falls; an accepted update
    repairs the cell as in the default mode.  Nothing non-finite reaches tri_llh, J or D."""
    model, tree, fp, r, cells = contradicting_case()
    o = _oracle(tree, model, fp, "B", "reference", seed=29, r=r)
    t = _oracle(tree, model, fp, "B", "telescoped", seed=29, r=r)
    snaps = []
    for w in range(5):
        o.sweep(w)
        t.sweep(w)
        snaps.append(o.paths())
    check_repair(tree, fp, snaps, cells)
    for b, s, want in cells:
        moved = column_changed(tree, fp, snaps[-1], s)
        print("cell", b, s, "r =", want, "moved" if moved else "never accepted")
        if want == 1:
            assert not moved
    J, D = o.suffstats()
    assert np.isfinite(J).all() and np.isfinite(D).all() and np.isfinite(o.tri_llh()).all()
    # where the two ratio modes differ
    assert not orc.paths_equal(o.paths(), t.paths())
