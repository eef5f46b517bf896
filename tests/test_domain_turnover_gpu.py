"""Domain turnover counted on the device during run_mcmc (epv_set_domain_turnover): the context's unclosed part --
hist [R, 2, 2, 128], len_sum [R, 2, 2] and every edge record -- and the closed result equal, bit for bit, what numpy
computes from the CPU oracle's paths after every batch sweep (rung B, the same Philox sweeps;
tests/turnover_ref.py); counting changes neither J, D, the accept count, the paths, tri_llh nor the plan.  With the
domain size spectra on in the same run, a branch's end row summed over kept is the domain part of its child node
and its start row that of the parent node.  Shapes the simulated inputs never reach (their longest turned-over run
is 8 sites) come from synthetic meta words on the single branch: runs of every length around a word and a bin edge,
kept and turned over, the kept site first, last, in the middle and on bit 0 and bit 63 of a word; a run across
both chunk boundaries of the runs kernel whose single kept site lies in the first chunk, more than 256 words
before the second boundary, or nowhere; constant rows; an unaligned range.  A LocalGroup of three and a
ShardedSampler equal one context after merge and close; the cap, the reset and the lifecycle; a masked leaf and a
sampled root; all eight summaries on give what each gives alone."""
import numpy as np
import pytest

import orc
import test_summaries_together_gpu as six
import turnover_ref as tr
from common import _tmp, ref_test_model, simulate
from epievo_amd import host
from epievo_amd.host import FlatPaths
from epievo_amd.parallel import LocalGroup, NullComm, ShardedSampler
from epievo_amd.sampler import EPV_ERR_STATE, DeviceSampler, EpvError

pytestmark = pytest.mark.gpu

NO_FUSED = {"EPV_FUSED_PHASE": "0"}
SEED, BASE, BURN_IN, BATCH = 77, 5, 1, 3
OFF_TEXT = "domain turnover is off: epv_set_domain_turnover first"
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


def _oracle_parts(o, burn_in, batch, base, lo=0, cnt=None):
    """the yardstick applied to the oracle's paths after every batch sweep -> (the summed part, the closed result of
    every sample)"""
    for w in range(burn_in):
        o.sweep(base + w)
    total, per_sample = None, []
    for w in range(batch):
        o.sweep(base + burn_in + w)
        x = tr.rows(o.paths())
        x = x[:, lo:x.shape[1] if cnt is None else lo + cnt]
        p = tr.part(x)
        per_sample.append(tr.close(*p)[0])
        total = p if total is None else tr.add_parts(total, p)
    return total, per_sample


def _assert_part(got, want):
    ns, hist, len_sum, edges = got
    assert hist.dtype == len_sum.dtype == edges.dtype == np.uint64
    assert ns == want[2].shape[0] and edges.shape == want[2].shape
    assert np.array_equal(edges, want[2])                      # every edge record of every sample
    assert np.array_equal(hist, want[0]) and np.array_equal(len_sum, want[1])


CASES = [("tree", 40000, {}, 3), ("tree", 3001, NO_FUSED, 1), ("tree", 257, {}, None), ("tree", 65, {}, None),
         ("tree", 3, {}, None), ("pair", 4000, {}, None), ("bal16", 3000, {}, 4), ("cat5", 3000, {}, None)]


@pytest.mark.parametrize("cfg,n,env,mode", CASES, ids=["%s-%d" % c[:2] for c in CASES])
def test_part_matches_oracle_and_changes_nothing(monkeypatch, cfg, n, env, mode):
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # read when a context is created
    model, tree, fp = _inputs(cfg, n)
    cap = _cap(fp)
    B = tree.n_nodes - 1
    on, off = _dev(tree, model, fp, cap), _dev(tree, model, fp, cap)
    assert on.phase_mode() == off.phase_mode() and (mode is None or on.phase_mode() == mode)
    on.enable_domain_turnover(BATCH)
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
    want, per_sample = _oracle_parts(o, BURN_IN, BATCH, BASE)
    assert orc.paths_equal(on.paths(), o.paths())
    assert on.domain_turnover_samples() == BATCH
    lay = on.domain_turnover_layout()
    assert lay[:4] == (2 * B, 128, 0, n) and lay[4] % 64 == 0 and lay[4] >= 64      # sites 0 and n - 1 included
    got = on.domain_turnover_part()
    _assert_part(got, want)
    ns, hist, len_sum = on.domain_turnover()
    closed = tr.close(*want)
    assert ns == BATCH and np.array_equal(hist, closed[0]) and np.array_equal(len_sum, closed[1])
    # 3. invariants, and the domain size spectra of the same run
    assert (len_sum.sum(axis=(1, 2)) == BATCH * n).all() and not hist[:, :, :, 0].any()
    dns, dhist, dlen, dedges = on.domain_stats_part()
    assert dns == BATCH
    unkept = ~np.uint64(tr.KEPT)
    for b in range(B):
        v, p = b + 1, int(tree.parent_ids[b + 1])
        for row, node in ((2 * b + 1, v), (2 * b, p)):
            assert np.array_equal(got[1][row].sum(axis=1), dhist[node])
            assert np.array_equal(got[2][row].sum(axis=1), dlen[node])
            assert np.array_equal(got[3][:, row] & unkept, dedges[:, node])
    # 4. not vacuous (asserted on the oracle's side)
    if n >= 3000:
        assert all(c > 0 for c in tr.turned_over_counts(closed[0])), tr.turned_over_counts(closed[0])
        if B > 1:                         # (on the single branch both ends are fixed: only jump times move)
            assert any(not np.array_equal(per_sample[0], h) for h in per_sample[1:])   # the samples differ
    on.close()
    off.close()


# ---- synthetic meta words on the single branch
LENGTHS = list(range(1, 18)) + [31, 32, 33, 63, 64, 65, 127, 128, 129]
VARIANTS = ("over", "first", "last", "middle", "bit0", "bit63")


def _laid():
    """-> (start row a, change bits c, [(length, variant, first site)]): runs of every length and variant laid end to
    end with alternating states; a run changes at every site but its kept one.  bit0 / bit63: a filler run before it
    puts the run's first (last) site on bit 0 (bit 63) of a word of a range that starts at site 0, and that site is
    the kept one"""
    a, c, runs = [], [], []
    state = 0

    def put(length, kept_at):
        nonlocal state
        a.extend([state] * length)
        c.extend([0 if i == kept_at else 1 for i in range(length)])
        state ^= 1

    for L in LENGTHS:
        for var in VARIANTS:
            if var == "bit0" and len(a) % 64:
                put(64 - len(a) % 64, None)
            if var == "bit63" and (len(a) + L) % 64:
                put(64 - (len(a) + L) % 64, None)
            runs.append((L, var, len(a)))
            put(L, {"over": None, "first": 0, "last": L - 1, "middle": L // 2, "bit0": 0, "bit63": L - 1}[var])
    put(3, 1)
    return np.array(a, np.uint8), np.array(c, np.uint8), runs


def _pair_paths(tree, a, c):
    """FlatPaths of the single branch with init state a and c + 0 or 2 jumps per site (so that k is not c itself)"""
    n = len(a)
    k = c.astype(np.int64) + 2 * (np.arange(n) % 3 == 0)
    T = float(tree.branches[1])
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(k)
    jumps = np.concatenate([T * (np.arange(kk) + 1.0) / (kk + 1.0) for kk in k]) if k.sum() else np.zeros(0)
    fp = FlatPaths(n, 2, a.astype(np.uint8), off, jumps)
    x = tr.rows(fp)
    assert np.array_equal(x[0], a) and np.array_equal(x[1], a ^ c)
    return fp, x


def _take_two(tree, model, fp):
    d = _dev(tree, model, fp, 16)
    d.enable_domain_turnover(2)
    d.reset()
    d.accumulate_domain_turnover()
    d.accumulate_domain_turnover()
    return d


def test_runs_around_word_and_bin_edges_kept_and_turned_over():
    model, tree, _ = simulate("pair", 8, seed=6)
    a, c, runs = _laid()
    n = len(a)
    fp, x = _pair_paths(tree, a, c)
    # the layout is what it claims, by the per-site walk alone
    wh, wl = tr.brute([a.tolist()], [fp.counts().tolist()])
    for L, var, at in runs:
        assert (x[0, at:at + L] == x[0, at]).all() and (at == 0 or x[0, at - 1] != x[0, at]) and x[0, at + L] != x[0, at]
        kept = x[0, at:at + L] == x[1, at:at + L]
        assert kept.sum() == (0 if var == "over" else 1)
        if var == "bit0":
            assert at % 64 == 0 and kept[0]
        if var == "bit63":
            assert (at + L - 1) % 64 == 63 and kept[-1]
    for L in LENGTHS:
        assert wh[0, :, 0, tr.bin_of(L)].sum() >= 1 and wh[0, :, 1, tr.bin_of(L)].sum() >= 5
    d = _take_two(tree, model, fp)
    assert d.domain_turnover_layout()[:4] == (2, 128, 0, n)
    one = tr.part(x)
    _assert_part(d.domain_turnover_part(), tr.add_parts(one, one))
    closed = d.domain_turnover()
    assert closed[0] == 2 and np.array_equal(closed[1], wh * np.uint64(2)) and np.array_equal(closed[2], wl * np.uint64(2))
    # the same over an unaligned range: tiles that start at site 37, edge records in the middle of runs
    d.set_update_range(37, n - 102)
    with pytest.raises(EpvError) as e:
        d.accumulate_domain_turnover()
    assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    d.enable_domain_turnover(2)
    d.reset()
    first, cnt = d.domain_turnover_layout()[2:4]
    assert (first, cnt) == (37, n - 102 - 37 + 1)
    d.accumulate_domain_turnover()
    d.accumulate_domain_turnover()
    one = tr.part(x[:, first:first + cnt])
    _assert_part(d.domain_turnover_part(), tr.add_parts(one, one))
    assert int(one[2][0, 0, 0]) != int(tr.part(x)[2][0, 0, 0])
    d.close()


def _chunk_sites(tree, model):
    d = _dev(tree, model, simulate("pair", 64, seed=1)[2], 16)
    d.enable_domain_turnover(1)
    cs = d.domain_turnover_layout()[4]
    d.close()
    return cs


@pytest.mark.parametrize("kept_at", ["first_chunk", "far_before_second_boundary", "nowhere"])
def test_a_run_across_both_chunk_boundaries(kept_at):
    model, tree, _ = simulate("pair", 8, seed=6)
    cs = _chunk_sites(tree, model)
    n = 2 * cs + 5
    a = np.zeros(n, np.uint8)
    a[40:n - 2] = 1                                            # one run over both boundaries, cs and 2 cs
    c = np.zeros(n, np.uint8)
    c[40:n - 2] = 1
    site = {"first_chunk": 1000, "far_before_second_boundary": cs + 64 * 300 + 17, "nowhere": None}[kept_at]
    if site is not None:
        assert 40 <= site and (2 * cs - site) // 64 > 256      # (the look-back of the last chunk walks more than one step)
        c[site] = 0
    fp, x = _pair_paths(tree, a, c)
    d = _take_two(tree, model, fp)
    assert d.domain_turnover_layout() == (2, 128, 0, n, cs)
    one = tr.part(x)
    assert int(one[2][0, 0, 1]) == tr.record(2, 0, True) and int(one[2][0, 0, 0]) == tr.record(40, 0, True)
    assert one[0][0, 1, int(site is not None), tr.bin_of(n - 42)] == 1 and one[0][0].sum() == 1
    _assert_part(d.domain_turnover_part(), tr.add_parts(one, one))
    ns, hist, len_sum = d.domain_turnover()
    assert ns == 2 and hist[0, 1, int(site is not None), tr.bin_of(n - 42)] == 2
    assert (len_sum.sum(axis=(1, 2)) == 2 * n).all()
    d.close()


@pytest.mark.parametrize("state,change,n_chunks", [(0, "none", 0), (1, "all", 0), (1, "all", 2), (0, "all_but_one", 2)])
def test_constant_rows(state, change, n_chunks):
    model, tree, _ = simulate("pair", 8, seed=6)
    n = n_chunks * _chunk_sites(tree, model) + 5 if n_chunks else 300
    a = np.full(n, state, np.uint8)
    c = np.zeros(n, np.uint8) if change == "none" else np.ones(n, np.uint8)
    if change == "all_but_one":
        c[7] = 0                                               # the end row has two ends; the start row is whole and kept
    fp, x = _pair_paths(tree, a, c)
    d = _take_two(tree, model, fp)
    one = tr.part(x)
    assert int(one[2][0, 0, 0]) == tr.record(n, state, change != "all", True)
    _assert_part(d.domain_turnover_part(), tr.add_parts(one, one))
    ns, hist, len_sum = d.domain_turnover()
    assert hist[0, state, int(change != "all"), tr.bin_of(n)] == 2 and hist[0].sum() == 2
    d.close()


# ---- groups
@pytest.fixture(scope="module")
def one_context():
    """tree at n = 3301: one context's part and result, shared by the group tests"""
    n = 3301
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    d = _dev(tree, model, fp, cap)
    d.enable_domain_turnover(BATCH)
    d.reset()
    run = d.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    part, closed = d.domain_turnover_part(), d.domain_turnover()
    d.close()
    return model, tree, fp, cap, n, run, part, closed


def test_local_group_of_three_equals_one_context(one_context):
    model, tree, fp, cap, n, (J1, D1, a1), part, closed = one_context
    g = LocalGroup(0, 3, sweeps_per_refresh=10)          # (halos of 256 sites: three shards fit 3301 sites)
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    assert len(g.subs) == 3
    g.enable_domain_turnover(BATCH)
    with pytest.raises(RuntimeError, match="reset\\(\\) the group"):
        g.accumulate_domain_turnover()
    g.reset()
    J3, D3, a3 = g.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert a3 == a1 and np.array_equal(J3, J1) and np.array_equal(D3, D1)
    R = 2 * (tree.n_nodes - 1)
    assert g.domain_turnover_samples() == BATCH and g.domain_turnover_layout()[:4] == (R, 128, 0, n)
    shard_parts = [s.domain_turnover_part() for s in g.subs]
    assert sum(s.domain_turnover_layout()[3] for s in g.subs) == n
    # runs cross the cuts: the merge closes runs that no shard could close
    assert sum(int(p[1].sum()) for p in shard_parts) < int(part[1].sum())
    _assert_part(g.domain_turnover_part(), part[1:])
    ns, hist, len_sum = g.domain_turnover()
    assert ns == BATCH and np.array_equal(hist, closed[1]) and np.array_equal(len_sum, closed[2])
    g.reset_domain_turnover()
    assert g.domain_turnover_samples() == 0 and not g.domain_turnover()[1].any()
    g.close()


@pytest.mark.parametrize("k", [1, 3])
def test_sharded_sampler_equals_one_context(one_context, k):
    model, tree, fp, cap, n, _, part, closed = one_context
    ss = ShardedSampler(NullComm(), 0, (lambda dev: LocalGroup(dev, 3, 10)) if k > 1 else None)
    ss.setup(model, tree, fp, [0, n], capacity=cap, sweeps_per_refresh=10)
    assert len(getattr(ss.dev, "subs", [ss.dev])) == k
    ss.enable_domain_turnover(BATCH)
    ss.reset()
    ss.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert ss.domain_turnover_samples() == BATCH
    _assert_part(ss.domain_turnover_part(), part[1:])
    ns, hist, len_sum = ss.domain_turnover()
    assert ns == BATCH and np.array_equal(hist, closed[1]) and np.array_equal(len_sum, closed[2])
    ss.reset_domain_turnover()
    assert not ss.domain_turnover()[1].any()
    ss.dev.close()


def test_lifecycle_and_cap():
    n = 3001
    model, tree, fp = simulate("tree", n, seed=6)
    d = _dev(tree, model, fp, _cap(fp))
    # off: nothing to read, nothing to add to, nothing counted
    for call in (d.domain_turnover, d.domain_turnover_part, d.accumulate_domain_turnover, d.reset_domain_turnover):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and OFF_TEXT in str(e.value)
    assert d.domain_turnover_samples() == 0 and d.domain_turnover_layout() == (0, 0, 0, 0, 0)
    d.reset()
    d.run_mcmc(0, 1, 5)
    assert d.domain_turnover_samples() == 0
    with pytest.raises(EpvError):
        d.enable_domain_turnover(2 ** 21 + 1)
    d.enable_domain_turnover(2)
    # before the first sample a new site range lays the part out again
    d.set_update_range(10, 2000)
    assert d.domain_turnover_layout()[:4] == (8, 128, 10, 1991)
    d.set_update_range(1, n - 2)
    d.reset()
    assert d.domain_turnover_layout()[:4] == (8, 128, 0, n)
    # a run whose batch would pass max_samples is refused before its first sweep
    paths = d.paths()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(1, 3, 5)
    assert e.value.code == EPV_ERR_STATE and "samples" in str(e.value) and "domain turnover" in str(e.value)
    assert d.domain_turnover_samples() == 0 and orc.paths_equal(d.paths(), paths)
    d.run_mcmc(0, 2, 5)
    assert d.domain_turnover_samples() == 2
    ns, hist, len_sum, edges = d.domain_turnover_part()
    assert np.array_equal(edges[1], tr.part(tr.rows(d.paths()))[2][0])   # the last sample is the resident paths'
    paths = d.paths()
    for call in (d.accumulate_domain_turnover, lambda: d.run_mcmc(0, 1, 5, sweep_base=2)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE
    assert d.domain_turnover_samples() == 2 and orc.paths_equal(d.paths(), paths)
    assert np.array_equal(d.domain_turnover_part()[1], hist)
    # kept over reset, set_model and scale_jump_times; a changed range after a sample is an error
    d.reset()
    d.set_model(model)
    d.scale_jump_times(tree.branches * 2.0)
    d.reset()
    assert d.domain_turnover_samples() == 2 and np.array_equal(d.domain_turnover_part()[1], hist)
    d.reset_domain_turnover()
    assert d.domain_turnover_samples() == 0
    ns, hist0, len0, edges0 = d.domain_turnover_part()
    assert ns == 0 and not hist0.any() and not len0.any() and edges0.shape == (0, 8, 2)
    d.run_mcmc(0, 1, 5, sweep_base=2)
    assert d.domain_turnover_samples() == 1
    d.set_update_range(10, 2000)
    d.reset()
    for call in (d.accumulate_domain_turnover, lambda: d.run_mcmc(0, 1, 5, sweep_base=3)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    assert d.domain_turnover_samples() == 1
    d.enable_domain_turnover(0)
    with pytest.raises(EpvError):
        d.domain_turnover()
    assert d.domain_turnover_layout() == (0, 0, 0, 0, 0)
    d.run_mcmc(0, 1, 5, sweep_base=3)                          # off again: runs, counts nothing
    assert d.domain_turnover_samples() == 0
    d.close()


def test_masked_leaf_turns_over():
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
    d.enable_domain_turnover(batch)
    d.reset()
    d.run_mcmc(0, batch, 41)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=41)
    o.set_unobserved(m)
    o.reset()
    want, per_sample = _oracle_parts(o, 0, batch, 0)
    assert orc.paths_equal(d.paths(), o.paths())
    _assert_part(d.domain_turnover_part(), want)
    end_row = 2 * (leaf - 1) + 1
    assert any(not np.array_equal(per_sample[0][end_row].sum(axis=1), h[end_row].sum(axis=1)) for h in per_sample)
    for v in leaves:                                           # an observed leaf's end row has the runs of its data
        if v != leaf:
            assert all(np.array_equal(per_sample[0][2 * v - 1].sum(axis=1), h[2 * v - 1].sum(axis=1)) for h in per_sample)
    d.close()


def test_sampled_root():
    """set_options(sample_root=True): the root state moves, so the start rows of the branches below it do"""
    n = 1000
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    d = _dev(tree, model, fp, cap)
    d.set_options(sample_root=True)
    d.enable_domain_turnover(4)
    d.reset()
    d.run_mcmc(1, 4, 23, sweep_base=2)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=23)
    o.set_sample_root(True)
    o.reset()
    want, per_sample = _oracle_parts(o, 1, 4, 2)
    assert orc.paths_equal(d.paths(), o.paths())
    root0 = fp.init.reshape(tree.n_nodes - 1, n)[0]
    assert (o.paths().init.reshape(tree.n_nodes - 1, n)[0] != root0).any()        # the root did move
    _assert_part(d.domain_turnover_part(), want)
    assert any(not np.array_equal(per_sample[0][0].sum(axis=1), h[0].sum(axis=1)) for h in per_sample)
    d.close()


EIGHT = six.LAYERS + ("change_patterns", "domain_turnover")


def test_all_eight_on_equal_each_alone():
    """all eight summaries on give the integers each gives alone; the seven existing read-outs are unchanged by the
    eighth"""
    model, tree, fp = simulate("tree", six.N_SITES, seed=4)
    cap = six._cap(fp)
    enable = dict(six.ENABLE, change_patterns=lambda d: d.enable_change_patterns(True),
                  domain_turnover=lambda d: d.enable_domain_turnover(six.BATCH))
    read = dict(six.READ, change_patterns=lambda d: d.change_patterns(counts=True),
                domain_turnover=lambda d: d.domain_turnover_part())

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
    for name in EIGHT:
        d = dev((name,))
        assert six._same_run(six._run(d), plain), name
        alone[name] = read[name](d)
        assert alone[name][0] == six.BATCH and any(np.asarray(x).any() for x in alone[name][1:]), name
        d.close()
    d7 = dev(EIGHT[:-1])
    assert six._same_run(six._run(d7), plain)
    d8 = dev(EIGHT[::-1])                            # (switched on against the order of the chain)
    assert six._same_run(six._run(d8), plain)
    for name in EIGHT:
        assert six._same_readout(read[name](d8), alone[name]), name
    for name in EIGHT[:-1]:
        assert six._same_readout(read[name](d8), read[name](d7)), name
    assert d8.domain_turnover_samples() == six.BATCH
    # of two layers that would both refuse a batch, the earlier one of the chain is the one reported
    with pytest.raises(EpvError) as e:
        d8.run_mcmc(0, 1, six.SEED, sweep_base=50)
    assert e.value.code == EPV_ERR_STATE and "domain statistics" in str(e.value) and "turnover" not in str(e.value)
    d7.close()
    d8.close()
