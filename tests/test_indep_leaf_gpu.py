"""Leaf masks and leaf evidence in the site-independent kernels (epv_indep_expectation, epv_indep_update_paths,
epv_indep_node_posterior): the identities with data and with the mask bit for bit against the oracle's rung B
(whose orc_indep_* functions take no table: they see hard data only), and the law against the numpy yardstick of
indep_law.py."""
import functools
import itertools

import numpy as np
import pytest

import indep_law as law
import orc
from common import simulate
from epievo_amd import host

pytestmark = pytest.mark.gpu
RATES = np.array([0.7, 1.9])
# tree 601: 256-lane stats blocks, three blocks, the last partial, n no multiple of 32; bal16 203: the 64-lane
# launch shape, four blocks, the last partial; multi 300: a trifurcation; tree 3: the smallest genome
SHAPES = [("tree", 601), ("bal16", 203), ("multi", 300), ("tree", 3)]
SWEEP0 = 0xF0000000


@functools.lru_cache(maxsize=None)
def _sim(cfg, n, seed=6):
    return simulate(cfg, n, seed=seed)


def _dev(tree, model, fp, cap=32):
    from epievo_amd.sampler import DeviceSampler
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    return d


def _leaves(tree):
    return [v for v in range(1, tree.n_nodes) if tree.subtree_sizes[v] == 1]


def _end_states(fp):
    B = fp.n_nodes - 1
    return fp.init.reshape(B, -1) ^ (fp.counts().reshape(B, -1) & 1).astype(np.uint8)


def _node_states(tree, fp):
    """(N, n): row 0 the root (the start of its first child's branch), row v the end of branch v"""
    es = _end_states(fp)
    return np.vstack([fp.init.reshape(tree.n_nodes - 1, -1)[:1], es])


def _sites(n):
    s = {0, 1, 31, 32, 33, 63, 64, 65, 191, 192, 193, n - 34, n - 33, n - 2, n - 1}
    return sorted(x for x in s if 0 <= x < n)


HARD, MINUS0 = "hard", "-0"
VALUES = [HARD, 0.5, MINUS0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.02, 0.8]


def _table(tree, fp, values=VALUES, shift=0):
    """cells at _sites(n) on every leaf, the rest NaN.  HARD: 0 or 1 agreeing with the data; MINUS0: -0 where
    the data are 0 (a hard 0 with its sign bit set), the data's 1 elsewhere"""
    es = _end_states(fp)
    r = np.full(es.shape, np.nan, np.float32)
    k = shift
    for v in _leaves(tree):
        for s in _sites(fp.n_sites):
            x = values[k % len(values)]
            k += 1
            if x is HARD:
                x = float(es[v - 1, s])
            elif x is MINUS0:
                x = 1.0 if es[v - 1, s] else -0.0
            r[v - 1, s] = x
    return r


def _soft(r):
    return ~np.isnan(r) & (r != 0) & (r != 1)


def _run(d, sweeps=3, seed=123):
    """J, D, node posterior, then the paths after each of `sweeps` update sweeps"""
    J, D = d.indep_expectation(RATES)
    post = d.indep_node_posterior(RATES)
    paths = []
    for w in range(sweeps):
        d.indep_update_paths(RATES, seed, sweep=SWEEP0 + w)
        paths.append(d.paths())
    return J, D, post, paths


def _same(a, b, with_post=True):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (not with_post or np.array_equal(a[2], b[2]))
            and all(orc.paths_equal(p, q) for p, q in zip(a[3], b[3])))


def _rung_b(tree, model, fp, sweeps=3, seed=123):
    o = orc.Oracle(tree, model, fp, "B", cap=32, seed=seed)
    J, D = o.indep_expectation(RATES)
    paths = []
    for w in range(sweeps):
        o.indep_update_paths(RATES, SWEEP0 + w)
        paths.append(o.paths())
    return J, D, None, paths


@pytest.mark.parametrize("cfg,n", SHAPES)
def test_nothing_held_is_nothing(cfg, n):
    model, tree, fp = _sim(cfg, n)
    exp = _rung_b(tree, model, fp)
    B = tree.n_nodes - 1
    for how in ("nan", "zero mask", "cleared"):
        d = _dev(tree, model, fp)
        if how == "nan":
            d.set_leaf_evidence(np.full((B, n), np.nan, np.float32))
        elif how == "zero mask":
            d.set_unobserved(np.zeros((B, n), np.uint8))
        else:
            d.set_leaf_evidence(_table(tree, fp))
            m = np.zeros((B, n), np.uint8)
            m[_leaves(tree)[0] - 1, 0] = 1
            d.set_unobserved(m)
            d.set_leaf_evidence(None)
            d.set_unobserved(None)
        assert d.leaf_evidence_cells() == 0 and d.unobserved_cells() == 0
        assert _same(_run(d), exp, with_post=False), how


@pytest.mark.parametrize("cfg,n", SHAPES)
def test_hard_evidence_is_data(cfg, n):
    """r = float32(leaf state) on every leaf cell (-0 for a 0 at the listed sites): the table instantiations run
    and give rung B bit for bit"""
    model, tree, fp = _sim(cfg, n)
    es = _end_states(fp)
    r = np.full(es.shape, np.nan, np.float32)
    lv = [v - 1 for v in _leaves(tree)]
    r[lv] = es[lv]
    t = _table(tree, fp, [HARD, MINUS0])
    r[~np.isnan(t)] = t[~np.isnan(t)]
    d = _dev(tree, model, fp)
    d.set_leaf_evidence(r)
    assert d.leaf_evidence_cells() == len(lv) * n
    got = _run(d)
    assert _same(got, _rung_b(tree, model, fp), with_post=False)
    plain = _dev(tree, model, fp)
    assert np.array_equal(got[2], plain.indep_node_posterior(RATES))


@pytest.mark.parametrize("cfg,n", SHAPES)
def test_half_is_the_mask(cfg, n):
    model, tree, fp = _sim(cfg, n)
    cells = ~np.isnan(_table(tree, fp))
    half = np.where(cells, np.float32(0.5), np.float32(np.nan)).astype(np.float32)
    a = _dev(tree, model, fp)
    a.set_leaf_evidence(half)
    b = _dev(tree, model, fp)
    b.set_unobserved(cells)
    ra, rb = _run(a), _run(b)
    assert _same(ra, rb)
    plain = _run(_dev(tree, model, fp))
    assert not np.array_equal(ra[0], plain[0]) and not np.array_equal(ra[2], plain[2])
    assert any(not orc.paths_equal(p, q) for p, q in zip(ra[3], plain[3]))
    # where both are given the evidence wins: a mask on every leaf cell under the full table is the table alone
    r = _table(tree, fp)
    c = _dev(tree, model, fp)
    c.set_leaf_evidence(r)
    e = _dev(tree, model, fp)
    e.set_leaf_evidence(r)
    e.set_unobserved(~np.isnan(r))
    assert _same(_run(c), _run(e))


@pytest.mark.parametrize("cfg,n", SHAPES)
def test_sites_are_independent(cfg, n):
    model, tree, fp = _sim(cfg, n)
    r = _table(tree, fp)
    d = _dev(tree, model, fp)
    d.set_leaf_evidence(r)
    got, plain = _run(d), _run(_dev(tree, model, fp))
    other = np.setdiff1d(np.arange(n), _sites(n))
    hard = ~_soft(r)
    hard[[v - 1 for v in range(1, tree.n_nodes) if tree.subtree_sizes[v] != 1]] = False   # leaf rows only
    moved = False
    for p, q in zip(got[3], plain[3]):
        if len(other):
            cols = np.zeros(n, bool)
            cols[other] = True
            assert _columns_equal(p, q, cols)
        es = _end_states(p)
        assert np.array_equal(es[hard], _end_states(fp)[hard])
        moved = moved or not np.array_equal(es, _end_states(q))
    assert moved                                  # a listed site changed a leaf end state
    assert np.array_equal(got[2][:, other], plain[2][:, other])


def _columns_equal(p, q, cols):
    """the paths of the flagged sites equal bit for bit"""
    B, n = p.n_nodes - 1, p.n_sites
    if not np.array_equal(p.init.reshape(B, n)[:, cols], q.init.reshape(B, n)[:, cols]):
        return False
    cp, cq = p.counts().reshape(B, n), q.counts().reshape(B, n)
    if not np.array_equal(cp[:, cols], cq[:, cols]):
        return False
    op, oq = p.offsets[:-1].reshape(B, n), q.offsets[:-1].reshape(B, n)
    for b in range(B):
        for s in np.nonzero(cols & (cp[b] > 0))[0]:
            if not np.array_equal(p.jumps[int(op[b, s]):int(op[b, s]) + int(cp[b, s])],
                                  q.jumps[int(oq[b, s]):int(oq[b, s]) + int(cq[b, s])]):
                return False
    return True


def _law_table(tree, fp, seed=11):
    """r in [0.02, 0.98] plus hard and 0.5 cells at the listed sites, and a mask on a few cells without r"""
    rng = np.random.default_rng(seed)
    n = fp.n_sites
    es = _end_states(fp)
    r = np.full(es.shape, np.nan, np.float32)
    mask = np.zeros(es.shape, np.uint8)
    for v in _leaves(tree):
        for s in _sites(n):
            kind = rng.integers(0, 6)
            if kind <= 2:
                r[v - 1, s] = rng.uniform(0.02, 0.98)
            elif kind == 3:
                r[v - 1, s] = es[v - 1, s]
            elif kind == 4:
                r[v - 1, s] = 0.5
            else:
                mask[v - 1, s] = 1
    return r, mask


@pytest.mark.parametrize("cfg,n", SHAPES)
def test_node_posterior_against_the_yardstick(cfg, n):
    """absolute 1e-12: a probability is reached through fewer than 20 N fp64 operations on normalised positive
    terms, N <= 31, so 1e-13 bounds the rounding and the bound leaves a factor of ten"""
    model, tree, fp = _sim(cfg, n)
    st = _node_states(tree, fp)
    r, mask = _law_table(tree, fp)
    d = _dev(tree, model, fp)
    for rr, mm in ((None, None), (r, mask)):
        if rr is not None:
            d.set_leaf_evidence(rr)
            d.set_unobserved(mm)
        got = d.indep_node_posterior(RATES)
        assert got.shape == (tree.n_nodes, n)
        q = law.leaf_q(tree, st, rr, mm)
        err = np.abs(got - law.marginals_pruning(tree, RATES, q)[0]).max()
        print(cfg, n, "table" if rr is not None else "data", "route 2: max abs error %.3g" % err)
        assert err <= 1e-12
        if cfg in ("tree", "multi"):
            err = np.abs(got - law.marginals_enum(tree, RATES, q)[0]).max()
            print(cfg, n, "route 1: max abs error %.3g" % err)
            assert err <= 1e-12


@functools.lru_cache(maxsize=None)
def _completion_stats(cfg):
    """(completions, J_c (C, 2B), D_c (C, 2B)) from rung B's indep_expectation on a 4-site genome whose sites all
    carry completion c, divided by 4 (the tree-order sum of four equal terms and the division are exact)"""
    model, tree, _ = _sim(cfg, 3)
    lv = _leaves(tree)
    comps = list(itertools.product((0, 1), repeat=len(lv)))
    Jc, Dc = [], []
    for c in comps:
        st = np.zeros((tree.n_nodes, 4), np.uint8)
        for v, x in zip(lv, c):
            st[v] = x
        p0 = host.initialize_paths_heuristic(1, tree, st)
        J, D = orc.Oracle(tree, model, p0, "B", cap=32).indep_expectation(RATES)
        Jc.append(J / 4)
        Dc.append(D / 4)
    return comps, np.array(Jc), np.array(Dc)


@pytest.mark.parametrize("cfg,n", SHAPES)
def test_expectation_against_the_completion_mixture(cfg, n):
    """J and D are the per-site mixtures over the hard completions c of the leaves with weight
    L(c) prod (r_i or 1 - r_i); rtol 1e-10 as between the GPU and the sequential rung in test_gpu_indep.py"""
    model, tree, fp = _sim(cfg, n)
    r, mask = _law_table(tree, fp, seed=12)
    d = _dev(tree, model, fp)
    d.set_leaf_evidence(r)
    d.set_unobserved(mask)
    J, D = d.indep_expectation(RATES)
    T = np.asarray(tree.branches)[1:]
    np.testing.assert_allclose(D[0::2] + D[1::2], n * T, rtol=1e-10)
    if cfg not in ("tree", "multi"):
        return
    comps, Jc, Dc = _completion_stats(cfg)
    lv = _leaves(tree)
    q = law.leaf_q(tree, _node_states(tree, fp), r, mask)
    w = np.zeros((len(comps), n))
    for k, c in enumerate(comps):
        st = np.zeros((tree.n_nodes, 1), np.uint8)
        for v, x in zip(lv, c):
            st[v] = x
        like = law.marginals_pruning(tree, RATES, law.leaf_q(tree, st))[1][0]
        w[k] = like * np.prod([q[v, :, x] for v, x in zip(lv, c)], axis=0)
    w /= w.sum(0)
    Je, De = w.sum(1) @ Jc, w.sum(1) @ Dc
    print(cfg, n, "max rel error J %.3g D %.3g" % (np.abs(J / Je - 1).max(), np.abs(D / De - 1).max()))
    np.testing.assert_allclose(J, Je, rtol=1e-10)
    np.testing.assert_allclose(D, De, rtol=1e-10)
    # and the table matters: the hard-data sums are somewhere else
    Jh, Dh = _dev(tree, model, fp).indep_expectation(RATES)
    assert np.abs(Jh / Je - 1).max() > 1e-6


def test_update_draws_from_the_conditional_law():
    """tree, n = 30000, r = (0.8, 0.02, 0.35) on C, D, F at every site.  The update keeps the root, and given the
    root every site is an independent draw from one law: in each root group the frequency of state 1 at C, D, F
    and at the internal node E lies within 5 binomial standard errors of the exact probability (route 1 with the
    root fixed).  Deterministic: fixed seeds, the bound is a property of the law"""
    n = 30000
    model, tree, fp = _sim("tree", n, seed=6)
    names = list(tree.node_names)
    r = np.full((tree.n_nodes - 1, n), np.nan, np.float32)
    for name, x in (("C", 0.8), ("D", 0.02), ("F", 0.35)):
        r[names.index(name) - 1] = x
    d = _dev(tree, model, fp)
    d.set_leaf_evidence(r)
    root = fp.init.reshape(tree.n_nodes - 1, n)[0]
    q = law.leaf_q(tree, np.zeros((tree.n_nodes, 1), np.uint8), r[:, :1])
    exact = [law.marginals_enum(tree, RATES, q, root=x)[0][:, 0] for x in (0, 1)]
    for w in range(3):
        d.indep_update_paths(RATES, 123, sweep=SWEEP0 + w)
        p = d.paths()
        assert np.array_equal(p.init.reshape(tree.n_nodes - 1, n)[0], root)
        es = _end_states(p)
        for x in (0, 1):
            grp = root == x
            m = int(grp.sum())
            assert m >= 2000, m
            for name in ("C", "D", "F", "E"):
                v = names.index(name)
                pe = exact[x][v]
                f = es[v - 1, grp].mean()
                se = np.sqrt(pe * (1 - pe) / m)
                print("sweep %d root %d (%d sites) %s: %.4f exact %.4f (%.2f se)" % (w, x, m, name, f, pe, (f - pe) / se))
                assert abs(f - pe) <= 5 * se, (w, x, name, f, pe, se)


@pytest.mark.parametrize("cfg,n", [("tree", 601), ("bal16", 203)])
def test_tables_survive_what_they_should(cfg, n):
    model, tree, fp = _sim(cfg, n)
    r, mask = _law_table(tree, fp)
    d = _dev(tree, model, fp)
    d.set_leaf_evidence(r)
    d.set_unobserved(mask)
    nb = np.asarray(tree.branches) * np.linspace(0.6, 1.7, tree.n_nodes)
    d.scale_jump_times(nb)
    assert d.leaf_evidence_cells() == int((~np.isnan(r)).sum()) and d.unobserved_cells() == int(mask.sum())
    t2 = host.Tree(tree.subtree_sizes, tree.parent_ids, nb, tree.node_names)
    f = _dev(t2, model, fp)
    f.set_leaf_evidence(r)
    f.set_unobserved(mask)
    assert np.array_equal(d.indep_node_posterior(RATES), f.indep_node_posterior(RATES))
    assert np.array_equal(d.indep_expectation(RATES)[0], f.indep_expectation(RATES)[0])
    # new paths are new data: the tables are gone and the expectation is rung B's again
    d.upload_paths(fp, 32)
    assert d.leaf_evidence_cells() == 0 and d.unobserved_cells() == 0
    Jo, Do = orc.Oracle(t2, model, fp, "B", cap=32).indep_expectation(RATES)
    Jd, Dd = d.indep_expectation(RATES)
    assert np.array_equal(Jd, Jo) and np.array_equal(Dd, Do)
