"""Domain maps counted on the device during run_mcmc (epv_set_domain_maps): the context's unmerged part -- counts
[N, K, sites] and every edge word of every sample -- equals, bit for bit, what numpy computes from the CPU oracle's
paths after every batch sweep (rung B, the same Philox sweeps; tests/domain_maps_ref.py), for both states; counting
changes neither J, D, the accept count, the paths, tri_llh nor the plan.  With the branch events and the domain size
spectra on in the same run: the size-1 row is the marginal of the node state (end1, or samples - end1), and the sum of
a row of a size up to 16 is what the closed spectra leave after the shorter runs.  What simulated inputs do not pin
comes from synthetic meta words on the single branch: runs of L - 1, L and L + 1 sites for L in {2, 64, 65, 1024} on
the first and the last site of the stretch, across a word boundary, across the boundary of a thread's two words
and across a chunk boundary of the membership kernel; a run longer than two chunks; constant and 0101.. rows; all
of them over the whole range and over an unaligned one.  A LocalGroup of three (one shard of exactly E sites) and a
ShardedSampler equal one context; a stretch shorter than E is refused before any sweep; the cap, the reset and the
lifecycle; a masked leaf; all eleven layers on give what each gives alone."""
import numpy as np
import pytest

import domain_maps_ref as mr
import orc
from common import simulate
from epievo_amd import host
from epievo_amd.parallel import LocalGroup, NullComm, ShardedSampler
from epievo_amd.sampler import EPV_ERR_ARG, EPV_ERR_STATE, DeviceSampler, EpvError
from test_spatial_correlation_gpu import _cap, _dev, _pair_paths

pytestmark = pytest.mark.gpu

NO_FUSED = {"EPV_FUSED_PHASE": "0"}
SEED, BASE, BURN_IN, BATCH = 77, 5, 1, 3
OFF_TEXT = "domain maps are off: epv_set_domain_maps first"
OFF_LAYOUT = (0, (), 0, 0, 0, 0)


def _oracle_parts(o, tree, sizes, state, burn_in, batch, base, lo=0, cnt=None):
    """the yardstick applied to the oracle's paths after every batch sweep -> (the summed part, every sample's part)"""
    for w in range(burn_in):
        o.sweep(base + w)
    total, per_sample = None, []
    for w in range(batch):
        o.sweep(base + burn_in + w)
        x = mr.rows(o.paths(), tree, state)
        x = x[:, lo:x.shape[1] if cnt is None else lo + cnt]
        p = mr.part(x, sizes)
        per_sample.append(p)
        total = p if total is None else mr.add_parts(total, p)
    return total, per_sample


def _assert_part(got, want):
    ns, cnt, counts, edges = got
    assert counts.dtype == np.uint32 and edges.dtype == np.uint64
    assert ns == want[2].shape[0] and cnt == want[0] and edges.shape == want[2].shape and counts.shape == want[1].shape
    assert np.array_equal(edges, want[2])                      # every edge word of every sample
    assert np.array_equal(counts, want[1])


def assert_not_vacuous(want, tree, n, sizes, samples):
    """on the oracle's side: at both sizes above 1 some internal node has a cell strictly between 0 and the samples,
    and some cell of the largest size is below the cell of the smallest"""
    if n < 257:
        return
    counts = want[1].astype(np.int64)
    internal = [v for v in range(tree.n_nodes) if tree.subtree_sizes[v] > 1]
    for k, L in enumerate(sizes):
        if L > 1:
            assert ((counts[internal, k] > 0) & (counts[internal, k] < samples)).any(), (n, L)
    assert (counts[:, 2] < counts[:, 0]).any()


# sizes (1, 5, 20) but at n = 257: there no internal node of the oracle's three samples has a cell of size 20 strictly
# between 0 and 3 for state 1 (checked on the oracle alone), so that shape takes (2, 5, 8), where every size has one
# for both states
CASES = [("tree", 40000, (1, 5, 20), {}, 3), ("tree", 3001, (1, 5, 20), NO_FUSED, 1), ("tree", 257, (2, 5, 8), {}, None),
         ("tree", 65, (1, 5, 20), {}, None), ("bal16", 3000, (1, 5, 20), {}, 4), ("tree", 3, (1, 2), {}, None)]


@pytest.mark.parametrize("state", [1, 0])
@pytest.mark.parametrize("cfg,n,sizes,env,mode", CASES, ids=["%s-%d" % c[:2] for c in CASES])
def test_part_matches_oracle_and_changes_nothing(monkeypatch, cfg, n, sizes, env, mode, state):
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # read when a context is created
    model, tree, fp = simulate(cfg, n, seed=6)
    cap = _cap(fp)
    N = tree.n_nodes
    on, off = _dev(tree, model, fp, cap), _dev(tree, model, fp, cap)
    assert on.phase_mode() == off.phase_mode() and (mode is None or on.phase_mode() == mode)
    on.enable_domain_maps(sizes, state, BATCH)
    on.enable_branch_events(True)         # (for the identities that tie the layers together)
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
    # 2. the part, bit for bit
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=SEED)
    o.reset()
    want, per_sample = _oracle_parts(o, tree, sizes, state, BURN_IN, BATCH, BASE)
    assert orc.paths_equal(on.paths(), o.paths())
    assert on.domain_maps_samples() == BATCH
    lay = on.domain_maps_layout()
    assert lay[:5] == (N, tuple(sizes), state, 0, n) and lay[5] % 64 == 0 and lay[5] >= 64   # sites 0 and n - 1 included
    got = on.domain_maps_part()
    _assert_part(got, want)
    ns, maps = on.domain_maps(counts=True)
    assert ns == BATCH and np.array_equal(maps, want[1])
    ns, freq = on.domain_maps()
    assert freq.dtype == np.float64 and np.array_equal(freq, want[1] / float(BATCH))
    # 3. invariants, and the other layers of the same run
    c = got[2].astype(np.int64)
    assert (c[:, 1:] <= c[:, :-1]).all() and (c <= BATCH).all()
    bns, planes = on.branch_events(counts=True)
    end1 = planes[0].astype(np.int64)                                      # [B, sites], branch b ends in node b + 1
    assert bns == BATCH
    if sizes[0] == 1:
        assert np.array_equal(c[1:, 0], end1 if state == 1 else BATCH - end1)
    dns, hist, len_sum = on.domain_stats()
    assert dns == BATCH
    for k, L in enumerate(sizes):
        if L <= 16:
            shorter = (np.arange(L)[None] * hist[:, state, :L].astype(np.int64)).sum(axis=1)
            assert np.array_equal(c[:, k].sum(axis=1), len_sum[:, state].astype(np.int64) - shorter), L
    # 4. not vacuous (asserted on the oracle's side)
    if len(sizes) == 3:
        assert_not_vacuous(want, tree, n, sizes, BATCH)
    if n >= 3000:
        for i in range(BATCH):
            for j in range(i):
                assert not np.array_equal(per_sample[i][1], per_sample[j][1])   # the samples differ
    on.close()
    off.close()


# ---- synthetic meta words on the single branch
def _take(dev, sizes, state, times=2):
    dev.enable_domain_maps(sizes, state, times)
    dev.reset()
    for _ in range(times):
        dev.accumulate_domain_maps()


def _times(p, k):
    out = p
    for _ in range(k - 1):
        out = mr.add_parts(out, p)
    return out


@pytest.fixture(scope="module")
def pair_setup():
    model, tree, _ = simulate("pair", 8, seed=6)
    d = _dev(tree, model, simulate("pair", 64, seed=1)[2], 16)
    d.enable_domain_maps((1,), 1, 1)
    cs = d.domain_maps_layout()[5]
    d.close()
    assert cs % 64 == 0 and cs >= 4096        # (the runs placed below do not collide)
    return model, tree, cs


def _check_whole_and_unaligned(model, tree, fp, x, sizes, lo, hi):
    """both states, over the whole range and over the sites lo .. hi"""
    n = x.shape[1]
    dev = _dev(tree, model, fp, 16)
    for state in (1, 0):
        rows = (x[:2] == state).astype(np.uint8)
        _take(dev, sizes, state)
        assert dev.domain_maps_layout()[:5] == (2, tuple(sizes), state, 0, n)
        _assert_part(dev.domain_maps_part(), _times(mr.part(rows, sizes), 2))
    dev.set_update_range(lo, hi)
    with pytest.raises(EpvError) as e:
        dev.accumulate_domain_maps()
    assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    for state in (1, 0):
        rows = (x[:2, lo:hi + 1] == state).astype(np.uint8)
        _take(dev, sizes, state)
        assert dev.domain_maps_layout()[3:5] == (lo, hi - lo + 1)
        _assert_part(dev.domain_maps_part(), _times(mr.part(rows, sizes), 2))
    dev.close()


@pytest.mark.parametrize("r_off", [-1, 0, 1])
@pytest.mark.parametrize("L", [2, 64, 65, 1024])
def test_runs_around_every_size_on_every_boundary(pair_setup, L, r_off):
    """node 0 holds runs of r = L + r_off ones: on the first site, across a word boundary, across the boundary of a
    thread's two words in the first and in the second chunk, across the boundary of the two chunks, and on the last
    site (in a third chunk, which is not full); and one that begins on the first site of the unaligned stretch and one
    that ends on its last site (the stretch begins inside a word and its length is no multiple of 64).  Node 1 is
    random.  A run counts if and only if r >= L"""
    model, tree, cs = pair_setup
    r = L + r_off
    words = cs // 64
    H = (L - 1 + 63) // 64 + 1                    # the halo of the membership kernel, in words
    n = 2 * cs + 2205
    half = (r + 1) // 2
    marks = [64 * 100, 64 * (256 - H), cs, cs + 64 * (256 - H)]      # (a thread holds slots t and t + 256 of the stage)
    assert words == 256
    lo, hi = 64 * 40 + 37, cs + 64 * 60 + 3       # the unaligned stretch
    assert lo % 64 and (hi - lo + 1) % 64
    starts = [0, lo] + [m - half for m in marks] + [hi - r + 1, n - r]
    a = np.zeros(n, np.uint8)
    for st in starts:
        assert not a[max(st - 1, 0):st + r + 1].any()               # the runs stay apart
        a[st:st + r] = 1
    rng = np.random.default_rng(L + r_off)
    c = (rng.random(n) < 0.2).astype(np.uint8)
    fp, x = _pair_paths(tree, a, c)
    one = mr.part(x[:2], (L,))
    assert int(one[1][0, 0].sum()) == (len(starts) * r if r >= L else 0)
    # in the stretch: whole runs on its first and on its last site, and three whole runs between them
    cut = mr.part(x[:2, lo:hi + 1], (L,))[1][0, 0]
    assert int(cut.sum()) == (5 * r if r >= L else 0) and cut[0] == cut[-1] == (1 if r >= L else 0)
    _check_whole_and_unaligned(model, tree, fp, x, (L,), lo, hi)


def test_a_run_longer_than_two_chunks_and_four_sizes(pair_setup):
    model, tree, cs = pair_setup
    n = 3 * cs + 100
    a = np.zeros(n, np.uint8)
    a[50:50 + 2 * cs + 300] = 1
    a[n - 999:] = 1                                # one site short of the largest size
    rng = np.random.default_rng(2)
    c = (rng.random(n) < 0.01).astype(np.uint8)
    fp, x = _pair_paths(tree, a, c)
    sizes = (5, 20, 100, 1000)
    one = mr.part(x[:2], sizes)
    assert one[1][0, 3].sum() == 2 * cs + 300 and one[1][0, 2].sum() == 2 * cs + 300 + 999
    _check_whole_and_unaligned(model, tree, fp, x, sizes, 101, n - 3)


@pytest.mark.parametrize("sizes", [(1,), (1, 2, 64, 1024), (2,)], ids=str)
def test_constant_and_alternating_rows(pair_setup, sizes):
    """node 0 all ones, node 1 0101..: every cell of node 0 counts at every size, node 1 only at size 1; and the
    complement for state 0.  With L_K = 1 there are no records.  Over the whole range and over an unaligned one"""
    model, tree, cs = pair_setup
    n = cs + 2300
    a, c = np.ones(n, np.uint8), (np.arange(n) & 1).astype(np.uint8)
    fp, x = _pair_paths(tree, a, c)
    E = mr.edge_bits(sizes)
    for state in (1, 0):                           # what the yardstick says of these rows
        cnt, counts, edges = mr.part((x[:2] == state).astype(np.uint8), sizes)
        assert cnt == n and edges.shape == (1, 2, 2, (E + 63) // 64)
        assert (counts[0] == (1 if state == 1 else 0)).all()
        for k, L in enumerate(sizes):
            assert np.array_equal(counts[1, k], (x[1] == state) if L == 1 else np.zeros(n))
    _check_whole_and_unaligned(model, tree, fp, x, sizes, 37, n - 70)


# ---- groups
# E = 1024: the first shard of a LocalGroup of three over 3400 sites holds exactly E.  State 0: at these inputs runs of
# zeros of five and more sites cross both cuts of the group (runs of ones happen to begin on them)
SIZES_GROUP, STATE_GROUP = (1, 5, 513), 0


@pytest.fixture(scope="module")
def one_context():
    n = 3400
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    d = _dev(tree, model, fp, cap)
    d.enable_domain_maps(SIZES_GROUP, STATE_GROUP, BATCH)
    d.reset()
    run = d.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    part = d.domain_maps_part()
    d.close()
    return model, tree, fp, cap, n, run, part


def test_local_group_of_three_equals_one_context(one_context):
    model, tree, fp, cap, n, (J1, D1, a1), part = one_context
    g = LocalGroup(0, 3, sweeps_per_refresh=10)          # (halos of 256 sites: three shards fit 3400 sites)
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    assert len(g.subs) == 3
    g.enable_domain_maps(SIZES_GROUP, STATE_GROUP, BATCH)
    with pytest.raises(RuntimeError, match="reset\\(\\) the group"):
        g.accumulate_domain_maps()
    g.reset()
    J3, D3, a3 = g.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert a3 == a1 and np.array_equal(J3, J1) and np.array_equal(D3, D1)
    assert g.domain_maps_samples() == BATCH and g.domain_maps_layout()[:5] == (tree.n_nodes, SIZES_GROUP, STATE_GROUP, 0, n)
    shard_parts = [s.domain_maps_part() for s in g.subs]
    assert [p[1] for p in shard_parts] == [1024, 1280, 1096]   # one shard of exactly E sites
    # runs cross the cuts: the merge counts memberships that no shard could see
    assert sum(int(p[2][:, 1].sum()) for p in shard_parts) < int(part[2][:, 1].sum())
    assert sum(int(p[2][:, 0].sum()) for p in shard_parts) == int(part[2][:, 0].sum())
    _assert_part(g.domain_maps_part(), part[1:])
    assert np.array_equal(g.domain_maps(counts=True)[1], part[2])
    g.reset_domain_maps()
    assert g.domain_maps_samples() == 0 and not g.domain_maps(counts=True)[1].any()
    g.close()


@pytest.mark.parametrize("k", [1, 3])
def test_sharded_sampler_equals_one_context(one_context, k):
    model, tree, fp, cap, n, _, part = one_context
    ss = ShardedSampler(NullComm(), 0, (lambda dev: LocalGroup(dev, 3, 10)) if k > 1 else None)
    ss.setup(model, tree, fp, [0, n], capacity=cap, sweeps_per_refresh=10)
    assert len(getattr(ss.dev, "subs", [ss.dev])) == k
    ss.enable_domain_maps(SIZES_GROUP, STATE_GROUP, BATCH)
    ss.reset()
    ss.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert ss.domain_maps_samples() == BATCH
    _assert_part(ss.domain_maps_part(), part[1:])
    assert np.array_equal(ss.domain_maps(counts=True)[1], part[2])
    ss.reset_domain_maps()
    assert not ss.domain_maps(counts=True)[1].any()
    ss.dev.close()


def test_a_stretch_shorter_than_an_edge_record_is_refused_before_any_sweep():
    """tree at n = 3301 in three shards of 1024, 1280 and 997 sites with L_K = 513 (E = 1024); and one context whose
    stretch is shorter than E"""
    n = 3301
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    g = LocalGroup(0, 3, sweeps_per_refresh=10)
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    assert len(g.subs) == 3
    g.enable_domain_maps((513,), 1, BATCH)
    g.reset()
    before = g.paths()
    with pytest.raises(EpvError) as e:
        g.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert e.value.code == EPV_ERR_ARG and "997 sites" in str(e.value) and "1024" in str(e.value)
    assert orc.paths_equal(g.paths(), before)                  # no shard swept
    assert all(s.domain_maps_samples() == 0 for s in g.subs)
    g.close()
    d = _dev(tree, model, fp, cap)
    d.set_update_range(100, 199)
    with pytest.raises(EpvError) as e:
        d.enable_domain_maps((52,), 1, 1)
    assert e.value.code == EPV_ERR_ARG and "100 sites" in str(e.value) and "102" in str(e.value)
    assert d.domain_maps_layout() == OFF_LAYOUT                # the layer is off
    d.enable_domain_maps((51,), 1, 1)                          # exactly E sites are taken
    d.set_update_range(100, 198)                               # a range that shrinks below E before a sample
    d.reset()
    paths = d.paths()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(1, 1, 5)
    assert e.value.code == EPV_ERR_ARG and "99 sites" in str(e.value) and orc.paths_equal(d.paths(), paths)
    d.close()


def test_lifecycle_and_cap():
    n, sizes = 3001, (1, 5, 20)
    model, tree, fp = simulate("tree", n, seed=6)
    N, EW = tree.n_nodes, 1
    d = _dev(tree, model, fp, _cap(fp))
    # off: nothing to read, nothing to add to, nothing counted
    for call in (d.domain_maps, d.domain_maps_part, d.accumulate_domain_maps, d.reset_domain_maps):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and OFF_TEXT in str(e.value)
    assert d.domain_maps_samples() == 0 and d.domain_maps_layout() == OFF_LAYOUT
    d.reset()
    d.run_mcmc(0, 1, 5)
    assert d.domain_maps_samples() == 0
    for bad in (((5, 5), 1, 2), ((5, 3), 1, 2), ((0, 3), 1, 2), ((1025,), 1, 2), ((1, 2, 3, 4, 5), 1, 2)):
        with pytest.raises(ValueError):
            d.enable_domain_maps(*bad)
    for bad in ((sizes, 1, 2 ** 21 + 1), (sizes, 1, 0)):
        with pytest.raises(EpvError) as e:
            d.enable_domain_maps(*bad)
        assert e.value.code == EPV_ERR_ARG
    with pytest.raises(ValueError):
        d.enable_domain_maps(sizes, 2, 2)
    # the C entry point refuses what the Python layer refuses
    import ctypes as C
    for bad in ((5, 5), (5, 3), (0, 3), (1025,), (1, 2, 3, 4, 5)):
        z = np.array(bad, np.uint32)
        assert d.L.epv_set_domain_maps(d.h, len(z), z.ctypes.data_as(C.POINTER(C.c_uint32)), 1, 2) == EPV_ERR_ARG
    assert d.L.epv_set_domain_maps(d.h, 1, np.array([3], np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), 2, 2) == EPV_ERR_ARG
    assert d.domain_maps_layout() == OFF_LAYOUT
    d.enable_domain_maps(sizes, 1, 2)
    # before the first sample a new site range lays the part out again
    d.set_update_range(10, 2000)
    assert d.domain_maps_layout()[:5] == (N, sizes, 1, 10, 1991)
    d.set_update_range(1, n - 2)
    d.reset()
    assert d.domain_maps_layout()[:5] == (N, sizes, 1, 0, n)
    # a run whose batch would pass max_samples is refused before its first sweep
    paths = d.paths()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(1, 3, 5)
    assert e.value.code == EPV_ERR_STATE and "samples" in str(e.value) and "domain maps" in str(e.value)
    assert d.domain_maps_samples() == 0 and orc.paths_equal(d.paths(), paths)
    d.run_mcmc(0, 2, 5)
    assert d.domain_maps_samples() == 2
    ns, cnt, counts, edges = d.domain_maps_part()
    last = mr.part(mr.rows(d.paths(), tree, 1), sizes)
    assert np.array_equal(edges[1], last[2][0])                # the last sample is the resident paths'
    paths = d.paths()
    for call in (d.accumulate_domain_maps, lambda: d.run_mcmc(0, 1, 5, sweep_base=2)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE
    assert d.domain_maps_samples() == 2 and orc.paths_equal(d.paths(), paths)
    assert np.array_equal(d.domain_maps_part()[2], counts)
    # kept over reset, set_model and scale_jump_times; a changed range after a sample is an error
    d.reset()
    d.set_model(model)
    d.scale_jump_times(tree.branches * 2.0)
    d.reset()
    assert d.domain_maps_samples() == 2 and np.array_equal(d.domain_maps_part()[2], counts)
    d.reset_domain_maps()
    assert d.domain_maps_samples() == 0
    ns, cnt, c0, edges0 = d.domain_maps_part()
    assert ns == 0 and cnt == n and not c0.any() and edges0.shape == (0, N, 2, EW)
    d.run_mcmc(0, 1, 5, sweep_base=2)
    assert d.domain_maps_samples() == 1 and d.domain_maps_part()[2].any()
    d.set_update_range(10, 2000)
    d.reset()
    for call in (d.accumulate_domain_maps, lambda: d.run_mcmc(0, 1, 5, sweep_base=3)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    assert d.domain_maps_samples() == 1
    d.enable_domain_maps(())                                   # switching off
    with pytest.raises(EpvError):
        d.domain_maps()
    assert d.domain_maps_layout() == OFF_LAYOUT
    d.run_mcmc(0, 1, 5, sweep_base=3)                          # off again: runs, counts nothing
    assert d.domain_maps_samples() == 0
    d.close()


def test_masked_leaf():
    n, batch, sizes = 601, 8, (1, 3, 8)
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
    d.enable_domain_maps(sizes, 1, batch)
    d.reset()
    d.run_mcmc(0, batch, 41)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=41)
    o.set_unobserved(m)
    o.reset()
    want, per_sample = _oracle_parts(o, tree, sizes, 1, 0, batch, 0)
    assert orc.paths_equal(d.paths(), o.paths())
    _assert_part(d.domain_maps_part(), want)
    assert any(not np.array_equal(per_sample[0][1][leaf], p[1][leaf]) for p in per_sample)   # the masked leaf's map moves
    c = want[1][leaf].astype(np.int64)
    assert ((c > 0) & (c < batch)).any()
    for v in leaves:                                           # an observed leaf's map is its data's
        if v != leaf:
            assert all(np.array_equal(per_sample[0][1][v], p[1][v]) for p in per_sample)
    d.close()


def test_all_eleven_layers_together():
    """every layer on at once gives what it gives alone, the eleventh included; the ten existing read-outs are what
    they are without it"""
    n = 1201
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    enable = {
        "path_average": (7,), "branch_events": (), "window_stats": (100,), "epoch_stats": (3,), "lineage_origins": (),
        "domain_stats": (8,), "change_patterns": (), "domain_turnover": (8,), "spatial_correlation": (5, 8),
        "mixing": (4,), "domain_maps": ((1, 5, 20), 1, 8)}
    read = {
        "path_average": lambda d: d.path_average(counts=True), "branch_events": lambda d: d.branch_events(counts=True),
        "window_stats": lambda d: d.window_stats(counts=True), "epoch_stats": lambda d: d.epoch_raw(),
        "lineage_origins": lambda d: d.lineage_origins(counts=True), "domain_stats": lambda d: d.domain_stats_part(),
        "change_patterns": lambda d: d.change_patterns(counts=True), "domain_turnover": lambda d: d.domain_turnover_part(),
        "spatial_correlation": lambda d: d.spatial_correlation_part(), "mixing": lambda d: d.mixing(counts=True),
        "domain_maps": lambda d: d.domain_maps_part()}

    def run(stems):
        d = _dev(tree, model, fp, cap)
        for stem in stems:
            getattr(d, "enable_" + stem)(*enable[stem])
        d.reset()
        out = [d.run_mcmc(BURN_IN, 4, SEED, sweep_base=c * 5) for c in range(2)]
        res = {stem: read[stem](d) for stem in stems}
        d.close()
        return out, res

    def same(a, b):
        return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))

    out_all, together = run(list(enable)[::-1])            # (switched on against the order of the chain)
    out_ten, ten = run(list(enable)[:-1])
    out_none, _ = run([])
    for stem in enable:
        out, alone = run([stem])
        for (J, D, a), (Ja, Da, aa), (Jn, Dn, an) in zip(out, out_all, out_none):
            assert a == aa == an and np.array_equal(J, Ja) and np.array_equal(D, Da) and np.array_equal(J, Jn)
        assert same(alone[stem], together[stem]), stem
        if stem != "domain_maps":
            assert same(ten[stem], together[stem]), stem
    assert together["domain_maps"][0] == 8 and together["domain_maps"][2].any()
    assert [a for _, _, a in out_ten] == [a for _, _, a in out_all]
