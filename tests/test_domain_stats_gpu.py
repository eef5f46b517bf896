"""Domain size spectra counted on the device during run_mcmc (epv_set_domain_stats): the context's unclosed part
-- hist [N, 2, 128], len_sum [N, 2] and every edge record -- and the closed result equal, bit for bit, what numpy
computes from the CPU oracle's paths after every batch sweep (rung B, the same Philox sweeps;
tests/domains_ref.py); counting changes neither J, D, the accept count, the paths, tri_llh nor the plan.  Shapes
the simulated inputs never reach (their longest run is 83 sites) come from synthetic paths: constant rows,
alternating rows, runs of every length around a bin edge and a run longer than two blocks of the runs kernel,
over the whole range and over an unaligned one.  A LocalGroup of three and a ShardedSampler equal one context
after merge and close; the cap, the reset and the lifecycle; a masked leaf.

The synthetic rows: the list of runs laid end to end with alternating states (lengths 1-17, 31-33, 63-65, 127-129 and, for
k = 4 .. 16, 2^k - 1, 2^k, 2^k + 2^(k-2) - 1, 2^k + 2^(k-2)) holds 590 551 sites, three times the n = 3 chunk_sites +
77 = 196 685 of a row, so the list is cut into as many pieces as it needs and every piece is a case of its own:
no length is left out."""
import numpy as np
import pytest

import domains_ref as dr
import orc
from common import simulate
from epievo_amd.host import FlatPaths
from epievo_amd.parallel import LocalGroup, NullComm, ShardedSampler
from epievo_amd.sampler import EPV_ERR_STATE, DeviceSampler, EpvError

pytestmark = pytest.mark.gpu

NO_FUSED = {"EPV_FUSED_PHASE": "0"}
SEED, BASE, BURN_IN, BATCH = 77, 5, 1, 3


def _dev(tree, model, fp, cap):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    return d


def _cap(fp):
    return int(max(16, 2 * fp.counts().max() + 8))


def _oracle_parts(o, tree, burn_in, batch, base, lo=0, cnt=None):
    """the yardstick applied to the oracle's paths after every batch sweep -> dict(part: the summed part,
    closed, per_sample: closed spectra [batch], crossing: runs that hold sites of two 64-site tiles)"""
    for w in range(burn_in):
        o.sweep(base + w)
    total, per_sample, crossing = None, [], 0
    for w in range(batch):
        o.sweep(base + burn_in + w)
        x = dr.node_states(o.paths(), tree)
        x = x[:, lo:x.shape[1] if cnt is None else lo + cnt]
        p = dr.part(x)
        per_sample.append(dr.close(*p)[0])
        crossing += dr.tile_crossing_runs(x)
        total = p if total is None else dr.add_parts(total, p)
    return dict(part=total, closed=dr.close(*total), per_sample=per_sample, crossing=crossing)


def _assert_part(got, want):
    ns, hist, len_sum, edges = got
    assert hist.dtype == len_sum.dtype == edges.dtype == np.uint64
    assert ns == want[2].shape[0] and edges.shape == want[2].shape
    assert np.array_equal(edges, want[2])                      # every edge record of every sample
    assert np.array_equal(hist, want[0]) and np.array_equal(len_sum, want[1])


@pytest.mark.parametrize("cfg,n,env,mode", [
    ("tree", 40000, {}, 3), ("tree", 3001, NO_FUSED, 1), ("bal16", 3000, {}, 4), ("tree", 257, {}, None),
    ("tree", 65, {}, None), ("tree", 3, {}, None)])
def test_part_matches_oracle_and_changes_nothing(monkeypatch, cfg, n, env, mode):
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # read when a context is created
    model, tree, fp = simulate(cfg, n, seed=6)
    cap = _cap(fp)
    N = tree.n_nodes
    on, off = _dev(tree, model, fp, cap), _dev(tree, model, fp, cap)
    assert on.phase_mode() == off.phase_mode() and (mode is None or on.phase_mode() == mode)
    on.enable_domain_stats(BATCH)
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
    want = _oracle_parts(o, tree, BURN_IN, BATCH, BASE)
    assert orc.paths_equal(on.paths(), o.paths())
    assert on.domain_stats_samples() == BATCH
    lay = on.domain_stats_layout()
    assert lay[:4] == (N, 128, 0, n) and lay[4] % 64 == 0 and lay[4] >= 64      # sites 0 and n - 1 included
    _assert_part(on.domain_stats_part(), want["part"])
    ns, hist, len_sum = on.domain_stats()
    assert ns == BATCH and np.array_equal(hist, want["closed"][0]) and np.array_equal(len_sum, want["closed"][1])
    # 3. invariants
    assert (len_sum.sum(axis=1) == BATCH * n).all() and not hist[:, :, 0].any()
    data_hist, data_len = dr.walk(dr.node_states(fp, tree))
    for v in range(1, N):
        if tree.subtree_sizes[v] == 1:                          # an observed leaf: samples x the spectrum of its data
            assert np.array_equal(hist[v], data_hist[v] * np.uint64(BATCH))
            assert np.array_equal(len_sum[v], data_len[v] * np.uint64(BATCH))
    # 4. not vacuous (asserted on the oracle's side)
    if n not in (3, 65):
        internal = [v for v in range(1, N) if tree.subtree_sizes[v] > 1]
        assert any(not np.array_equal(a[v], b[v]) for v in internal
                   for a in want["per_sample"] for b in want["per_sample"])
        assert want["crossing"] >= 1
    assert all(np.array_equal(want["per_sample"][0][0], h[0]) for h in want["per_sample"])   # the root is not resampled
    on.close()
    off.close()


def _laid_lengths():
    ls = list(range(1, 18)) + [31, 32, 33, 63, 64, 65, 127, 128, 129]
    for k in range(4, 17):
        ls += [2 ** k - 1, 2 ** k, 2 ** k + 2 ** (k - 2) - 1, 2 ** k + 2 ** (k - 2)]
    return ls


def _laid_pieces(n):
    """the list of runs cut into rows of at most n sites, each run whole: [[lengths of row 0], ...]"""
    rows, cur, used = [], [], 0
    for l in _laid_lengths():
        assert l <= n
        if used + l > n:
            rows.append(cur)
            cur, used = [], 0
        cur.append(l)
        used += l
    rows.append(cur)
    return rows


def _row_of_runs(lengths, n, first_state=0):
    """runs of the given lengths with alternating states from site 0; what is left of the row goes on alternating
    in runs of 3"""
    x = np.zeros(n, np.uint8)
    at, st = 0, first_state
    for l in lengths:
        x[at:at + l] = st
        at, st = at + l, st ^ 1
    while at < n:
        x[at:at + 3] = st
        at, st = at + 3, st ^ 1
    return x


def _synthetic(tree, n, chunk_sites, laid):
    """FlatPaths whose node rows are: root = one run of 2 chunk_sites + 5 sites from site 40, then short runs;
    node 1 = all 0 (a branch with one jump wherever the root shows 1); node 2 = all 1; node 3 = 0101...;
    node 4 = the runs `laid`.  Nodes 2-4 reach their state with 0, 1 or 2 jumps in turn"""
    B = tree.n_nodes - 1
    assert B == 4 and int(tree.parent_ids[1]) == 0
    root = np.zeros(n, np.uint8)
    root[40:40 + 2 * chunk_sites + 5] = 1
    root[40 + 2 * chunk_sites + 5:] = _row_of_runs([2, 1, 5, 1, 1, 7], n - (40 + 2 * chunk_sites + 5))
    want = np.zeros((B + 1, n), np.uint8)
    want[0] = root
    want[2] = 1
    want[3] = np.arange(n) & 1
    want[4] = _row_of_runs(laid, n)
    init, cnt = np.zeros((B, n), np.uint8), np.zeros((B, n), np.int64)
    init[0], cnt[0] = root, root                               # node 1: back to 0 by one jump
    site = np.arange(n)
    for v in (2, 3, 4):
        k = (site + v) % 3                                     # 0, 1 or 2 jumps
        cnt[v - 1] = k
        init[v - 1] = want[v] ^ (k & 1).astype(np.uint8)
    jumps = []
    T = np.asarray(tree.branches, np.float64)
    for b in range(B):                                         # one jump at T / 2, two at T / 4 and 3 T / 4
        vals = np.stack([np.where(cnt[b] == 1, 0.5, 0.25) * T[b + 1], np.full(n, 0.75 * T[b + 1])], axis=1)
        jumps.append(vals[np.stack([cnt[b] >= 1, cnt[b] == 2], axis=1)])
    off = np.zeros(B * n + 1, np.uint64)
    off[1:] = np.cumsum(cnt.reshape(-1))
    fp = FlatPaths(n, tree.n_nodes, init.reshape(-1), off, np.concatenate(jumps))
    assert np.array_equal(dr.node_states(fp, tree), want)
    return fp, want


def _chunk_sites(tree, model):
    _, _, fp = simulate("tree", 64, seed=1)
    d = _dev(tree, model, fp, 16)
    d.enable_domain_stats(1)
    cs = d.domain_stats_layout()[4]
    d.close()
    return cs


@pytest.mark.parametrize("piece", [0, 1, 2, 3])
def test_shapes_the_simulated_inputs_never_reach(piece):
    model, tree, _ = simulate("tree", 8, seed=6)
    cs = _chunk_sites(tree, model)
    n = 3 * cs + 77
    pieces = _laid_pieces(n)
    assert len(pieces) == 4 and sorted(sum(pieces, [])) == sorted(_laid_lengths())   # chunk_sites = 65 536: four rows
    fp, x = _synthetic(tree, n, cs, pieces[piece])
    d = _dev(tree, model, fp, 16)
    d.enable_domain_stats(2)
    d.reset()
    d.accumulate_domain_stats()
    d.accumulate_domain_stats()
    assert d.domain_stats_layout() == (5, 128, 0, n, cs)
    one = dr.part(x)
    want = dr.add_parts(one, one)
    _assert_part(d.domain_stats_part(), want)
    whole = np.uint64(dr.WHOLE)
    assert (want[2][:, 1:3, :] & whole).all() and not (want[2][:, [0, 3, 4], :] & whole).any()
    closed = d.domain_stats()
    wh, wl = dr.walk(x)
    assert closed[0] == 2 and np.array_equal(closed[1], wh * np.uint64(2)) and np.array_equal(closed[2], wl * np.uint64(2))
    assert closed[1][0, 1, dr.bin_of(2 * cs + 5)] == 2 and closed[1][3, :, 1].sum() == 2 * n
    for l in pieces[piece][1:]:                                # (the row's first run is an edge record; closed, it is binned too)
        assert closed[1][4, :, dr.bin_of(l)].sum() >= 2
    # the same over an unaligned range: tiles that start at site 37, edge records in the middle of runs
    d.set_update_range(37, n - 102)
    with pytest.raises(EpvError) as e:
        d.accumulate_domain_stats()
    assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    d.enable_domain_stats(2)
    d.reset()
    first, cnt = d.domain_stats_layout()[2:4]
    assert (first, cnt) == (37, n - 102 - 37 + 1)
    d.accumulate_domain_stats()
    d.accumulate_domain_stats()
    one = dr.part(x[:, first:first + cnt])
    _assert_part(d.domain_stats_part(), dr.add_parts(one, one))
    assert int(one[2][0, 0, 0]) == dr.record(3, 0) and int(one[2][0, 4, 0]) != int(dr.part(x)[2][0, 4, 0])
    d.close()


@pytest.fixture(scope="module")
def one_context():
    """tree at n = 40 000: one context's part and result, and the oracle's, shared by the group tests"""
    n = 40000
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    d = _dev(tree, model, fp, cap)
    d.enable_domain_stats(BATCH)
    d.reset()
    run = d.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    part, closed = d.domain_stats_part(), d.domain_stats()
    d.close()
    return model, tree, fp, cap, n, run, part, closed


def test_local_group_of_three_equals_one_context(one_context):
    model, tree, fp, cap, n, (J1, D1, a1), part, closed = one_context
    g = LocalGroup(0, 3)
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    assert len(g.subs) == 3
    g.enable_domain_stats(BATCH)
    with pytest.raises(RuntimeError, match="reset\\(\\) the group"):
        g.accumulate_domain_stats()
    g.reset()
    J3, D3, a3 = g.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert a3 == a1 and np.array_equal(J3, J1) and np.array_equal(D3, D1)
    assert g.domain_stats_samples() == BATCH and g.domain_stats_layout()[:4] == (tree.n_nodes, 128, 0, n)
    shard_parts = [s.domain_stats_part() for s in g.subs]
    assert sum(s.domain_stats_layout()[3] for s in g.subs) == n
    # runs cross the cuts: the merge closes runs that no shard could close
    assert sum(int(p[1].sum()) for p in shard_parts) < int(part[1].sum())
    got = g.domain_stats_part()
    _assert_part(got, part[1:])
    ns, hist, len_sum = g.domain_stats()
    assert ns == BATCH and np.array_equal(hist, closed[1]) and np.array_equal(len_sum, closed[2])
    g.reset_domain_stats()
    assert g.domain_stats_samples() == 0 and not g.domain_stats()[1].any()
    g.close()


@pytest.mark.parametrize("k", [1, 3])
def test_sharded_sampler_equals_one_context(one_context, k):
    model, tree, fp, cap, n, _, part, closed = one_context
    ss = ShardedSampler(NullComm(), 0, (lambda dev: LocalGroup(dev, 3, 10)) if k > 1 else None)
    ss.setup(model, tree, fp, [0, n], capacity=cap, sweeps_per_refresh=10)
    assert len(getattr(ss.dev, "subs", [ss.dev])) == k
    ss.enable_domain_stats(BATCH)
    ss.reset()
    ss.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert ss.domain_stats_samples() == BATCH
    _assert_part(ss.domain_stats_part(), part[1:])
    ns, hist, len_sum = ss.domain_stats()
    assert ns == BATCH and np.array_equal(hist, closed[1]) and np.array_equal(len_sum, closed[2])
    ss.reset_domain_stats()
    assert not ss.domain_stats()[1].any()
    ss.dev.close()


def test_lifecycle_and_cap():
    n = 3001
    model, tree, fp = simulate("tree", n, seed=6)
    d = _dev(tree, model, fp, _cap(fp))
    # off: nothing to read, nothing to add to, nothing counted
    for call in (d.domain_stats, d.domain_stats_part, d.accumulate_domain_stats, d.reset_domain_stats):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and "epv_set_domain_stats first" in str(e.value)
    assert d.domain_stats_samples() == 0 and d.domain_stats_layout() == (0, 0, 0, 0, 0)
    d.reset()
    d.run_mcmc(0, 1, 5)
    assert d.domain_stats_samples() == 0
    with pytest.raises(EpvError):
        d.enable_domain_stats(2 ** 21 + 1)
    d.enable_domain_stats(2)
    # before the first sample a new site range lays the part out again
    d.set_update_range(10, 2000)
    assert d.domain_stats_layout()[:4] == (5, 128, 10, 1991)
    d.set_update_range(1, n - 2)
    d.reset()
    assert d.domain_stats_layout()[:4] == (5, 128, 0, n)
    # a run whose batch would pass max_samples is refused before its first sweep
    paths = d.paths()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(1, 3, 5)
    assert e.value.code == EPV_ERR_STATE and "samples" in str(e.value)
    assert d.domain_stats_samples() == 0 and orc.paths_equal(d.paths(), paths)
    d.run_mcmc(0, 2, 5)
    assert d.domain_stats_samples() == 2
    x = dr.node_states(d.paths(), tree)
    ns, hist, len_sum, edges = d.domain_stats_part()
    assert np.array_equal(edges[1], dr.part(x)[2][0])          # the last sample is the resident paths'
    paths = d.paths()
    for call in (d.accumulate_domain_stats, lambda: d.run_mcmc(0, 1, 5, sweep_base=2)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE
    assert d.domain_stats_samples() == 2 and orc.paths_equal(d.paths(), paths)
    assert np.array_equal(d.domain_stats_part()[1], hist)
    # kept over reset, set_model and scale_jump_times; a changed range after a sample is an error
    d.reset()
    d.set_model(model)
    d.scale_jump_times(tree.branches * 2.0)
    d.reset()
    assert d.domain_stats_samples() == 2 and np.array_equal(d.domain_stats_part()[1], hist)
    d.reset_domain_stats()
    assert d.domain_stats_samples() == 0
    ns, hist0, len0, edges0 = d.domain_stats_part()
    assert ns == 0 and not hist0.any() and not len0.any() and edges0.shape == (0, 5, 2)
    d.run_mcmc(0, 1, 5, sweep_base=2)
    assert d.domain_stats_samples() == 1
    d.set_update_range(10, 2000)
    d.reset()
    for call in (d.accumulate_domain_stats, lambda: d.run_mcmc(0, 1, 5, sweep_base=3)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    assert d.domain_stats_samples() == 1
    d.enable_domain_stats(0)
    with pytest.raises(EpvError):
        d.domain_stats()
    assert d.domain_stats_layout() == (0, 0, 0, 0, 0)
    d.run_mcmc(0, 1, 5, sweep_base=3)                          # off again: runs, counts nothing
    assert d.domain_stats_samples() == 0
    d.close()


def test_masked_leaf_has_a_spectrum_of_its_own():
    n, batch = 601, 8
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    leaves = [b for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1]
    leaf = max(leaves, key=lambda b: tree.branches[b])
    m = np.zeros((tree.n_nodes - 1, n), np.uint8)
    m[leaf - 1, [1, 31, 32, 33, 63, 64, 65, n - 2]] = 1
    m[leaf - 1, 200:260] = 1
    d = _dev(tree, model, fp, cap)
    d.set_unobserved(m)
    d.enable_domain_stats(batch)
    d.reset()
    d.run_mcmc(0, batch, 41)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=41)
    o.set_unobserved(m)
    o.reset()
    want = _oracle_parts(o, tree, 0, batch, 0)
    assert orc.paths_equal(d.paths(), o.paths())
    _assert_part(d.domain_stats_part(), want["part"])
    assert any(not np.array_equal(want["per_sample"][0][leaf], h[leaf]) for h in want["per_sample"])   # it varies
    for v in leaves:
        if v != leaf:
            assert all(np.array_equal(want["per_sample"][0][v], h[v]) for h in want["per_sample"])
    d.close()
