"""Spatial correlations counted on the device during run_mcmc (epv_set_spatial_correlation): the context's unclosed
part -- n11 [R, L + 1] and every edge word of every sample -- and the closed result equal, bit for bit, what numpy
computes from the CPU oracle's paths after every batch sweep (rung B, the same Philox sweeps; tests/corr_ref.py);
counting changes neither J, D, the accept count, the paths, tri_llh nor the plan.  With the domain size spectra on
in the same run, the disagreeing neighbour pairs of a node row are its runs minus one per sample.  What simulated
inputs do not pin comes from synthetic meta words on the single branch: exactly two ones d sites apart for lags
around every word edge, on bit 0, on bit 63, across the boundary of two chunks of the count kernel and with the
right site on the last site of the stretch or just beyond it; all-ones, constant-zero and random rows with tails
that start on a word boundary and inside a word, max_lag a multiple of 64 and not; an unaligned range.  A
LocalGroup of three (one shard of exactly max_lag sites) and a ShardedSampler equal one context after merge and
close; a shard shorter than max_lag is refused before any sweep; the cap, the reset and the lifecycle; a masked
leaf and a sampled root; all nine summaries on give what each gives alone.

On the single branch (`pair`) both end states of the branch are data, so every sample has the same rows: there the
samples cannot differ, and that assertion is made on the trees with B > 1."""
import numpy as np
import pytest

import corr_ref as cr
import orc
import test_summaries_together_gpu as six
from common import _tmp, ref_test_model, simulate
from epievo_amd import host
from epievo_amd.host import FlatPaths
from epievo_amd.parallel import LocalGroup, NullComm, ShardedSampler
from epievo_amd.sampler import EPV_ERR_ARG, EPV_ERR_STATE, DeviceSampler, EpvError

pytestmark = pytest.mark.gpu

NO_FUSED = {"EPV_FUSED_PHASE": "0"}
SEED, BASE, BURN_IN, BATCH = 77, 5, 1, 3
OFF_TEXT = "spatial correlations are off: epv_set_spatial_correlation first"
# a caterpillar of five leaves: B = 8 branches, exactly one full chunk of the pack kernel's meta loads
CAT5_NWK = "((((A:0.05,B:0.07)U:0.04,C:0.1)V:0.03,D:0.15)W:0.06,E:0.2)R:0.0;\n"


def _inputs(cfg, n, seed=6):
    if cfg == "cat5":
        model, tree = ref_test_model(), host.Tree.read(_tmp("cat5.nwk", CAT5_NWK))
        return model, tree, host.simulate(model, tree, n, seed)
    return simulate(cfg, n, seed=seed)


def _dev(tree, model, fp, cap):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    return d


def _cap(fp):
    return int(max(16, 2 * fp.counts().max() + 8))


def _oracle_parts(o, tree, L, burn_in, batch, base, lo=0, cnt=None):
    """the yardstick applied to the oracle's paths after every batch sweep -> (the summed part, every sample's part)"""
    for w in range(burn_in):
        o.sweep(base + w)
    total, per_sample = None, []
    for w in range(batch):
        o.sweep(base + burn_in + w)
        x = cr.rows(o.paths(), tree)
        x = x[:, lo:x.shape[1] if cnt is None else lo + cnt]
        p = cr.part(x, L)
        per_sample.append(p)
        total = p if total is None else cr.add_parts(total, p)
    return total, per_sample


def _assert_part(got, want):
    ns, cnt, n11, edges = got
    assert n11.dtype == edges.dtype == np.uint64
    assert ns == want[2].shape[0] and cnt == want[0] and edges.shape == want[2].shape and n11.shape == want[1].shape
    assert np.array_equal(edges, want[2])                      # every edge word of every sample
    assert np.array_equal(n11, want[1])
    L = n11.shape[1] - 1
    if L % 64:
        assert not (edges[..., -1] >> np.uint64(L % 64)).any()  # the spare bits of the last edge word


CASES = [("tree", 40000, 256, {}, 3), ("tree", 3001, 65, NO_FUSED, 1), ("tree", 257, 64, {}, None),
         ("tree", 65, 65, {}, None), ("tree", 3, 2, {}, None), ("pair", 4000, 100, {}, None),
         ("bal16", 3000, 1024, {}, 4), ("cat5", 3000, 130, {}, None)]


@pytest.mark.parametrize("cfg,n,L,env,mode", CASES, ids=["%s-%d" % c[:2] for c in CASES])
def test_part_matches_oracle_and_changes_nothing(monkeypatch, cfg, n, L, env, mode):
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # read when a context is created
    model, tree, fp = _inputs(cfg, n)
    cap = _cap(fp)
    N = tree.n_nodes
    B = N - 1
    on, off = _dev(tree, model, fp, cap), _dev(tree, model, fp, cap)
    assert on.phase_mode() == off.phase_mode() and (mode is None or on.phase_mode() == mode)
    on.enable_spatial_correlation(L, BATCH)
    on.enable_domain_stats(BATCH)         # (for the cross-check that ties the two together)
    assert on.phase_plan()["word"] == off.phase_plan()["word"]
    on.reset()
    off.reset()
    # 1. nothing else changes
    J1, D1, a1 = on.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    J0, D0, a0 = off.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert a1 == a0 and np.array_equal(J1, J0) and np.array_equal(D1, D0)
    assert orc.paths_equal(on.paths(), off.paths())
    assert np.array_equal(on.tri_llh(), off.tri_llh())
    assert on.phase_plan()["word"] == off.phase_plan()["word"]
    # 2. the part and the closed result, bit for bit
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=SEED)
    o.reset()
    want, per_sample = _oracle_parts(o, tree, L, BURN_IN, BATCH, BASE)
    assert orc.paths_equal(on.paths(), o.paths())
    assert on.spatial_correlation_samples() == BATCH
    lay = on.spatial_correlation_layout()
    assert lay[:4] == (N + B, L, 0, n) and lay[4] % 64 == 0 and lay[4] >= 64       # sites 0 and n - 1 included
    got = on.spatial_correlation_part()
    _assert_part(got, want)
    ns, n11, left1, right1 = on.spatial_correlation()
    closed = cr.close(*want)
    assert ns == BATCH and all(g.dtype == np.uint64 and np.array_equal(g, w) for g, w in zip((n11, left1, right1), closed))
    # 3. invariants, and the domain size spectra of the same run
    assert (n11 <= np.minimum(left1, right1)).all() and (left1 + right1 - n11 <= cr.pairs(BATCH, n, L)[None]).all()
    assert np.array_equal(n11[:, 0], left1[:, 0]) and np.array_equal(n11[:, 0], right1[:, 0])
    dns, dhist, dlen = on.domain_stats()
    assert dns == BATCH
    for v in range(N):
        disagree = int(left1[v, 1] - n11[v, 1]) + int(right1[v, 1] - n11[v, 1])
        assert disagree == int(dhist[v].sum()) - BATCH
    # 4. not vacuous (asserted on the oracle's side)
    if n >= 3000:
        assert (closed[0][:N] > 0).all()                                       # every node row, every lag
        assert int(closed[0][N:, 1].sum()) >= 1                                # clustered changes exist
        if B > 1:                         # (on the single branch both ends are fixed: only jump times move)
            for i in range(BATCH):
                for j in range(i):
                    assert not np.array_equal(per_sample[i][1], per_sample[j][1])   # the samples differ
    on.close()
    off.close()


# ---- synthetic meta words on the single branch
def _pair_paths(tree, a, c):
    """FlatPaths of the single branch with init state a and c + 0 or 2 jumps per site (so that k is not c itself);
    rows: node 0 = a, node 1 = a XOR c, the branch's changes = c"""
    n = len(a)
    k = c.astype(np.int64) + 2 * (np.arange(n) % 3 == 0)
    T = float(tree.branches[1])
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(k)
    frac = (np.arange(int(k.sum())) - np.repeat(off[:-1].astype(np.int64), k) + 1.0) / (np.repeat(k, k) + 1.0)
    fp = FlatPaths(n, 2, a.astype(np.uint8), off, T * frac)
    x = cr.rows(fp, tree)
    assert np.array_equal(x[0], a) and np.array_equal(x[1], a ^ c) and np.array_equal(x[2], c)
    return fp, x


def _take_two(tree, model, fp, L):
    d = _dev(tree, model, fp, 16)
    d.enable_spatial_correlation(L, 2)
    d.reset()
    d.accumulate_spatial_correlation()
    d.accumulate_spatial_correlation()
    return d


def _twice(p):
    return cr.add_parts(p, p)


@pytest.fixture(scope="module")
def pair_setup():
    model, tree, _ = simulate("pair", 8, seed=6)
    d = _dev(tree, model, simulate("pair", 64, seed=1)[2], 16)
    d.enable_spatial_correlation(1, 1)
    cs = d.spatial_correlation_layout()[4]
    d.close()
    assert cs % 64 == 0 and cs >= 1088        # (a chunk holds max_lag and a word: the positions below do not collide)
    return model, tree, cs


@pytest.mark.parametrize("d_lag", [1, 63, 64, 65, 127, 128, 129, 1023, 1024])
def test_two_ones_give_one_pair_at_their_lag_and_nothing_elsewhere(pair_setup, d_lag):
    """pairs more than max_lag apart from each other: the left site on bit 0 of a word, on bit 63, in the last word
    of the first chunk (the right site in the next chunk for most lags), somewhere in the second chunk, and with the
    right site on the very last site.  Then the stretch is cut, from an unaligned first site, so that the fourth
    pair's right site is the first site beyond it: that pair must not count"""
    model, tree, cs = pair_setup
    L = 1024
    n = 2 * cs + 5
    starts = [64 * 20, 64 * 60 + 63, cs - 64 + 30, n - 4000 - d_lag, n - 1 - d_lag]
    assert all(b - a > 2 * L for a, b in zip(starts[:-1], starts[1:]))
    assert (starts[2] + d_lag >= cs) == (d_lag >= 34)
    a, c = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for p in starts:
        c[p] = c[p + d_lag] = 1
    fp, x = _pair_paths(tree, a, c)
    one = cr.part(x, L)
    want = np.zeros(L + 1, np.uint64)
    want[0], want[d_lag] = 10, 5
    assert np.array_equal(one[1][1], want) and np.array_equal(one[1][2], want) and not one[1][0].any()
    dev = _take_two(tree, model, fp, L)
    assert dev.spatial_correlation_layout() == (3, L, 0, n, cs)
    _assert_part(dev.spatial_correlation_part(), _twice(one))
    # the stretch [37, starts[3] + d_lag - 1]: the right site of the fourth pair is the first site beyond it
    hi = starts[3] + d_lag - 1
    dev.set_update_range(37, hi)
    with pytest.raises(EpvError) as e:
        dev.accumulate_spatial_correlation()
    assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    dev.enable_spatial_correlation(L, 2)
    dev.reset()
    first, cnt = dev.spatial_correlation_layout()[2:4]
    assert (first, cnt) == (37, hi - 37 + 1)
    dev.accumulate_spatial_correlation()
    dev.accumulate_spatial_correlation()
    cut = cr.part(x[:, first:first + cnt], L)
    want[0], want[d_lag] = 7, 3
    assert np.array_equal(cut[1][2], want)                      # the pair that leaves the range does not count
    assert cr.unpack_bits(cut[2][0, 2, 1], L)[L - d_lag] == 1   # its left site is among the last d_lag of the stretch
    _assert_part(dev.spatial_correlation_part(), _twice(cut))
    dev.close()


# (sites, max_lag): two chunks and five sites; a tail that starts on a word boundary with max_lag a multiple of 64;
# a tail that starts inside a word with max_lag not a multiple; a tail on a word boundary with max_lag not a multiple;
# max_lag = the stretch; lag 1 alone; three sites
ROWS = [(None, 1024), (1024 + 192, 1024), (1000, 100), (164, 100), (777, 64), (130, 130), (64, 1), (3, 3)]


@pytest.mark.parametrize("n,L", ROWS, ids=["%s-%d" % r for r in ROWS])
def test_all_ones_rows_and_random_rows(pair_setup, n, L):
    """a = 1 everywhere and random changes: node 0 is all ones (n11[d] = cnt - d exactly), node 1 and the change row
    are random with ones up to both ends"""
    model, tree, cs = pair_setup
    n = 2 * cs + 5 if n is None else n
    rng = np.random.default_rng(n + L)
    a, c = np.ones(n, np.uint8), (rng.random(n) < 0.4).astype(np.uint8)
    c[[0, n - 1]] = 1
    fp, x = _pair_paths(tree, a, c)
    one = cr.part(x, L)
    assert np.array_equal(one[1][0], n - np.arange(L + 1))
    dev = _take_two(tree, model, fp, L)
    ns, cnt, n11, edges = dev.spatial_correlation_part()
    assert np.array_equal(n11[0], np.uint64(2) * (np.uint64(n) - np.arange(L + 1, dtype=np.uint64)))
    assert (cr.unpack_bits(edges[:, 0], L) == 1).all()
    _assert_part((ns, cnt, n11, edges), _twice(one))
    ns, n11, left1, right1 = dev.spatial_correlation()
    assert np.array_equal(left1[0], n11[0]) and np.array_equal(right1[0], n11[0])
    assert all(np.array_equal(g, w) for g, w in zip((n11, left1, right1), cr.close(*_twice(one))))
    dev.close()


def test_constant_zero_rows(pair_setup):
    model, tree, cs = pair_setup
    n = cs + 300
    fp, x = _pair_paths(tree, np.zeros(n, np.uint8), np.zeros(n, np.uint8))
    assert fp.counts().sum() > 0 and not x.any()               # jumps there are, an even number at every site
    dev = _take_two(tree, model, fp, 200)
    ns, cnt, n11, edges = dev.spatial_correlation_part()
    assert ns == 2 and cnt == n and not n11.any() and not edges.any() and edges.shape == (2, 3, 2, 4)
    assert not any(a.any() for a in dev.spatial_correlation()[1:])
    dev.close()


# ---- groups
L_GROUP = 1024


@pytest.fixture(scope="module")
def one_context():
    """tree at n = 3400 with max_lag = 1024: one context's part and result, shared by the group tests.  A LocalGroup
    of three cuts it into shards of 1024 (exactly max_lag), 1280 and 1096 sites"""
    n = 3400
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    d = _dev(tree, model, fp, cap)
    d.enable_spatial_correlation(L_GROUP, BATCH)
    d.reset()
    run = d.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    part, closed = d.spatial_correlation_part(), d.spatial_correlation()
    d.close()
    return model, tree, fp, cap, n, run, part, closed


def test_local_group_of_three_equals_one_context(one_context):
    model, tree, fp, cap, n, (J1, D1, a1), part, closed = one_context
    g = LocalGroup(0, 3, sweeps_per_refresh=10)          # (halos of 256 sites: three shards fit 3400 sites)
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    assert len(g.subs) == 3
    g.enable_spatial_correlation(L_GROUP, BATCH)
    with pytest.raises(RuntimeError, match="reset\\(\\) the group"):
        g.accumulate_spatial_correlation()
    g.reset()
    J3, D3, a3 = g.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert a3 == a1 and np.array_equal(J3, J1) and np.array_equal(D3, D1)
    R = 2 * tree.n_nodes - 1
    assert g.spatial_correlation_samples() == BATCH and g.spatial_correlation_layout()[:4] == (R, L_GROUP, 0, n)
    shard_parts = [s.spatial_correlation_part() for s in g.subs]
    assert [p[1] for p in shard_parts] == [1024, 1280, 1096]   # one shard of exactly max_lag sites
    # pairs cross the cuts: the merge counts pairs that no shard could count
    assert sum(int(p[2][:, 1:].sum()) for p in shard_parts) < int(part[2][:, 1:].sum())
    assert sum(int(p[2][:, 0].sum()) for p in shard_parts) == int(part[2][:, 0].sum())
    _assert_part(g.spatial_correlation_part(), part[1:])
    got = g.spatial_correlation()
    assert got[0] == BATCH and all(np.array_equal(a, b) for a, b in zip(got[1:], closed[1:]))
    g.reset_spatial_correlation()
    assert g.spatial_correlation_samples() == 0 and not g.spatial_correlation()[1].any()
    g.close()


@pytest.mark.parametrize("k", [1, 3])
def test_sharded_sampler_equals_one_context(one_context, k):
    model, tree, fp, cap, n, _, part, closed = one_context
    ss = ShardedSampler(NullComm(), 0, (lambda dev: LocalGroup(dev, 3, 10)) if k > 1 else None)
    ss.setup(model, tree, fp, [0, n], capacity=cap, sweeps_per_refresh=10)
    assert len(getattr(ss.dev, "subs", [ss.dev])) == k
    ss.enable_spatial_correlation(L_GROUP, BATCH)
    ss.reset()
    ss.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert ss.spatial_correlation_samples() == BATCH
    _assert_part(ss.spatial_correlation_part(), part[1:])
    got = ss.spatial_correlation()
    assert got[0] == BATCH and all(np.array_equal(a, b) for a, b in zip(got[1:], closed[1:]))
    ss.reset_spatial_correlation()
    assert not ss.spatial_correlation()[1].any()
    ss.dev.close()


def test_a_shard_shorter_than_max_lag_is_refused_before_any_sweep():
    """tree at n = 3301 in three shards of 1024, 1280 and 997 sites with max_lag = 1024; and one context whose
    stretch is shorter than max_lag"""
    n = 3301
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    g = LocalGroup(0, 3, sweeps_per_refresh=10)
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    assert len(g.subs) == 3
    g.enable_spatial_correlation(1024, BATCH)
    g.reset()
    before = g.paths()
    with pytest.raises(EpvError) as e:
        g.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert e.value.code == EPV_ERR_ARG and "997 sites" in str(e.value) and "max_lag = 1024" in str(e.value)
    assert orc.paths_equal(g.paths(), before)                  # no shard swept
    assert all(s.spatial_correlation_samples() == 0 for s in g.subs)
    g.close()
    d = _dev(tree, model, fp, cap)
    with pytest.raises(EpvError) as e:
        d.enable_spatial_correlation(1025, 1)
    assert e.value.code == EPV_ERR_ARG
    d.set_update_range(100, 199)
    with pytest.raises(EpvError) as e:
        d.enable_spatial_correlation(101, 1)
    assert e.value.code == EPV_ERR_ARG and "100 sites" in str(e.value) and "max_lag = 101" in str(e.value)
    assert d.spatial_correlation_layout() == (0, 0, 0, 0, 0)   # the layer is off
    d.enable_spatial_correlation(100, 1)                       # exactly max_lag sites are taken
    d.set_update_range(100, 198)                               # a range that shrinks below max_lag before a sample
    d.reset()
    paths = d.paths()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(1, 1, 5)
    assert e.value.code == EPV_ERR_ARG and "99 sites" in str(e.value) and orc.paths_equal(d.paths(), paths)
    d.close()


def test_lifecycle_and_cap():
    n, L = 3001, 70
    model, tree, fp = simulate("tree", n, seed=6)
    R, LW = 2 * tree.n_nodes - 1, 2
    d = _dev(tree, model, fp, _cap(fp))
    # off: nothing to read, nothing to add to, nothing counted
    for call in (d.spatial_correlation, d.spatial_correlation_part, d.accumulate_spatial_correlation,
                 d.reset_spatial_correlation):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and OFF_TEXT in str(e.value)
    assert d.spatial_correlation_samples() == 0 and d.spatial_correlation_layout() == (0, 0, 0, 0, 0)
    d.reset()
    d.run_mcmc(0, 1, 5)
    assert d.spatial_correlation_samples() == 0
    for bad in ((L, 2 ** 21 + 1), (L, 0), (1025, 2)):
        with pytest.raises(EpvError) as e:
            d.enable_spatial_correlation(*bad)
        assert e.value.code == EPV_ERR_ARG
    d.enable_spatial_correlation(L, 2)
    # before the first sample a new site range lays the part out again
    d.set_update_range(10, 2000)
    assert d.spatial_correlation_layout()[:4] == (R, L, 10, 1991)
    d.set_update_range(1, n - 2)
    d.reset()
    assert d.spatial_correlation_layout()[:4] == (R, L, 0, n)
    # a run whose batch would pass max_samples is refused before its first sweep
    paths = d.paths()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(1, 3, 5)
    assert e.value.code == EPV_ERR_STATE and "samples" in str(e.value) and "spatial correlations" in str(e.value)
    assert d.spatial_correlation_samples() == 0 and orc.paths_equal(d.paths(), paths)
    d.run_mcmc(0, 2, 5)
    assert d.spatial_correlation_samples() == 2
    ns, cnt, n11, edges = d.spatial_correlation_part()
    assert np.array_equal(edges[1], cr.part(cr.rows(d.paths(), tree), L)[2][0])   # the last sample is the resident paths'
    paths = d.paths()
    for call in (d.accumulate_spatial_correlation, lambda: d.run_mcmc(0, 1, 5, sweep_base=2)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE
    assert d.spatial_correlation_samples() == 2 and orc.paths_equal(d.paths(), paths)
    assert np.array_equal(d.spatial_correlation_part()[2], n11)
    # kept over reset, set_model and scale_jump_times; a changed range after a sample is an error
    d.reset()
    d.set_model(model)
    d.scale_jump_times(tree.branches * 2.0)
    d.reset()
    assert d.spatial_correlation_samples() == 2 and np.array_equal(d.spatial_correlation_part()[2], n11)
    d.reset_spatial_correlation()
    assert d.spatial_correlation_samples() == 0
    ns, cnt, n0, edges0 = d.spatial_correlation_part()
    assert ns == 0 and cnt == n and not n0.any() and edges0.shape == (0, R, 2, LW)
    d.run_mcmc(0, 1, 5, sweep_base=2)
    assert d.spatial_correlation_samples() == 1
    d.set_update_range(10, 2000)
    d.reset()
    for call in (d.accumulate_spatial_correlation, lambda: d.run_mcmc(0, 1, 5, sweep_base=3)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    assert d.spatial_correlation_samples() == 1
    d.enable_spatial_correlation(0, 0)
    with pytest.raises(EpvError):
        d.spatial_correlation()
    assert d.spatial_correlation_layout() == (0, 0, 0, 0, 0)
    d.run_mcmc(0, 1, 5, sweep_base=3)                          # off again: runs, counts nothing
    assert d.spatial_correlation_samples() == 0
    d.close()


def test_masked_leaf():
    n, batch, L = 601, 8, 70
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    N = tree.n_nodes
    leaves = [b for b in range(1, N) if tree.subtree_sizes[b] == 1]
    leaf = max(leaves, key=lambda b: tree.branches[b])
    m = np.zeros((N - 1, n), np.uint8)
    m[leaf - 1, [1, 31, 32, 33, 63, 64, 65, n - 2]] = 1
    m[leaf - 1, 200:260] = 1
    d = _dev(tree, model, fp, cap)
    d.set_unobserved(m)
    d.enable_spatial_correlation(L, batch)
    d.reset()
    d.run_mcmc(0, batch, 41)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=41)
    o.set_unobserved(m)
    o.reset()
    want, per_sample = _oracle_parts(o, tree, L, 0, batch, 0)
    assert orc.paths_equal(d.paths(), o.paths())
    _assert_part(d.spatial_correlation_part(), want)
    assert any(not np.array_equal(per_sample[0][1][leaf], p[1][leaf]) for p in per_sample)   # the masked leaf moves
    for v in leaves:                                           # an observed leaf's row is its data
        if v != leaf:
            assert all(np.array_equal(per_sample[0][1][v], p[1][v]) for p in per_sample)
    d.close()


def test_sampled_root():
    """set_options(sample_root=True): the root state moves, so row 0 does"""
    n, L = 1000, 70
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    d = _dev(tree, model, fp, cap)
    d.set_options(sample_root=True)
    d.enable_spatial_correlation(L, 4)
    d.reset()
    d.run_mcmc(1, 4, 23, sweep_base=2)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=23)
    o.set_sample_root(True)
    o.reset()
    want, per_sample = _oracle_parts(o, tree, L, 1, 4, 2)
    assert orc.paths_equal(d.paths(), o.paths())
    root0 = fp.init.reshape(tree.n_nodes - 1, n)[0]
    assert (o.paths().init.reshape(tree.n_nodes - 1, n)[0] != root0).any()        # the root did move
    _assert_part(d.spatial_correlation_part(), want)
    assert any(not np.array_equal(per_sample[0][1][0], p[1][0]) for p in per_sample)
    d.close()


NINE = six.LAYERS + ("change_patterns", "domain_turnover", "spatial_correlation")


def test_all_nine_on_equal_each_alone():
    """all nine summaries on give the integers each gives alone; the eight existing read-outs are unchanged by the
    ninth"""
    model, tree, fp = simulate("tree", six.N_SITES, seed=4)
    cap = six._cap(fp)

    def corr_part(d):
        ns, cnt, n11, edges = d.spatial_correlation_part()
        assert cnt == six.N_SITES
        return ns, n11, edges

    enable = dict(six.ENABLE, change_patterns=lambda d: d.enable_change_patterns(True),
                  domain_turnover=lambda d: d.enable_domain_turnover(six.BATCH),
                  spatial_correlation=lambda d: d.enable_spatial_correlation(65, six.BATCH))
    read = dict(six.READ, change_patterns=lambda d: d.change_patterns(counts=True),
                domain_turnover=lambda d: d.domain_turnover_part(), spatial_correlation=corr_part)

    def dev(layers):
        d = _dev(tree, model, fp, cap)
        for name in layers:
            enable[name](d)
        d.reset()
        return d

    none = dev(())
    plain = six._run(none)
    none.close()
    alone = {}
    for name in NINE:
        d = dev((name,))
        assert six._same_run(six._run(d), plain), name
        alone[name] = read[name](d)
        assert alone[name][0] == six.BATCH and any(np.asarray(x).any() for x in alone[name][1:]), name
        d.close()
    d8 = dev(NINE[:-1])
    assert six._same_run(six._run(d8), plain)
    d9 = dev(NINE[::-1])                             # (switched on against the order of the chain)
    assert six._same_run(six._run(d9), plain)
    for name in NINE:
        assert six._same_readout(read[name](d9), alone[name]), name
    for name in NINE[:-1]:
        assert six._same_readout(read[name](d9), read[name](d8)), name
    assert d9.spatial_correlation_samples() == six.BATCH
    # of the layers that would refuse a batch, the earliest one of the chain is the one reported
    with pytest.raises(EpvError) as e:
        d9.run_mcmc(0, 1, six.SEED, sweep_base=50)
    assert e.value.code == EPV_ERR_STATE and "domain statistics" in str(e.value) and "correlation" not in str(e.value)
    d8.close()
    d9.close()
