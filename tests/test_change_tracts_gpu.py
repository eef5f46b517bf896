"""Change tracts counted on the device during run_mcmc (epv_set_change_tracts): the context's unclosed part -- hist
[B, 27, 128], len_sum [B, 27] and every edge record -- and the closed result equal, bit for bit, what numpy computes
from the CPU oracle's paths after every batch sweep (rung B, the same Philox sweeps; tests/tracts_ref.py); counting
changes neither J, D, the accept count, the paths, tri_llh nor the plan.  With the branch events on in the same run,
a branch's len_sum over the classes is its net gains plus its net losses over the sites.  Shapes the simulated
inputs never reach (their longest tract is 15 sites, none at a genome end) come from synthetic meta words on the
single branch: tracts of every length around a word and a bin edge in each direction and between each pair of
flanks; mixed tracts whose single opposite site is first, last, in the middle and on bit 0 and bit 63 of a word;
tracts at the first and the last site; a tract across both chunk boundaries of the tract kernel whose start, and
whose only opposite site, lie more than 256 words before the second boundary; dense random rows with a tract
across a chunk boundary; all-changed and unchanged rows; an unaligned range.  A LocalGroup of three and a ShardedSampler equal one context after merge and close; the cap, the
reset and the lifecycle; a masked leaf and a sampled root; all twelve layers on give what each gives alone."""
import numpy as np
import pytest

import orc
import tracts_ref as xr
from common import _tmp, ref_test_model, simulate
from epievo_amd import host
from epievo_amd.host import FlatPaths
from epievo_amd.parallel import LocalGroup, NullComm, ShardedSampler
from epievo_amd.sampler import EPV_ERR_STATE, DeviceSampler, EpvError

pytestmark = pytest.mark.gpu

NO_FUSED = {"EPV_FUSED_PHASE": "0"}
SEED, BASE, BURN_IN, BATCH = 77, 5, 1, 3
OFF_TEXT = "change tracts are off: epv_set_change_tracts first"
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


def _oracle_parts(o, burn_in, batch, base):
    """the yardstick applied to the oracle's paths after every batch sweep -> (the summed part, the closed result of
    every sample)"""
    for w in range(burn_in):
        o.sweep(base + w)
    total, per_sample = None, []
    for w in range(batch):
        o.sweep(base + burn_in + w)
        p = xr.part(xr.rows(o.paths()))
        per_sample.append(xr.close(*p)[0])
        total = p if total is None else xr.add_parts(total, p)
    return total, per_sample


def _assert_part(got, want):
    ns, hist, len_sum, edges = got
    assert hist.dtype == len_sum.dtype == edges.dtype == np.uint64
    assert ns == want[2].shape[0] and edges.shape == want[2].shape
    assert np.array_equal(edges, want[2]), [(hex(int(a)), hex(int(b))) for a, b in zip(edges.ravel(), want[2].ravel()) if a != b][:4]
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
    on.enable_change_tracts(BATCH)
    on.enable_branch_events(True)         # (for the cross-check that ties the two together)
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
    assert on.change_tracts_samples() == BATCH
    lay = on.change_tracts_layout()
    assert lay[:5] == (B, 27, 128, 0, n) and lay[5] % 64 == 0 and lay[5] >= 64      # sites 0 and n - 1 included
    _assert_part(on.change_tracts_part(), want)
    ns, hist, len_sum = on.change_tracts()
    closed = xr.close(*want)
    assert ns == BATCH and np.array_equal(hist, closed[0]) and np.array_equal(len_sum, closed[1])
    # 3. the branch events of the same run: a branch's tracts hold its net gains and net losses, every site once
    ens, ev = on.branch_events(counts=True)
    assert ens == BATCH and not hist[:, :, 0].any()
    assert np.array_equal(len_sum.sum(axis=1), (ev[1].astype(np.uint64) + ev[2]).sum(axis=1))
    # 4. not vacuous (asserted on the oracle's side)
    if n >= 3000:
        counts = xr.pure_counts(closed[0])
        assert all(counts[d, l, r] > 0 for d in (0, 1) for l in (0, 1) for r in (0, 1)), counts
        if B > 1:                         # (on the single branch both ends are fixed: only jump times move)
            assert any(not np.array_equal(per_sample[0], h) for h in per_sample[1:])   # the samples differ
    on.close()
    off.close()


# ---- synthetic meta words on the single branch
LENGTHS = list(range(1, 18)) + [31, 32, 33, 63, 64, 65, 127, 128, 129]
OPPOSITE = ("first", "last", "middle", "bit0", "bit63")


def _laid():
    """-> (start row a, change bits c, [(length, direction, left, right, variant, first site)]): a tract at site 0,
    then tracts of every length, direction and pair of flanks, each between an unchanged site of either state, then
    mixed tracts with a single opposite site, then a tract at the last site.  bit0 / bit63: unchanged filler sites put
    the tract's first (last) site, the opposite one, on bit 0 (bit 63) of a word of a range that starts at site 0"""
    a, c, tracts = [], [], []

    def still(y, count=1):
        a.extend([y] * count)
        c.extend([0] * count)

    def tract(L, direction, opposite_at=None):             # a gained site starts at 0, a lost one at 1
        a.extend([(direction if i != opposite_at else 1 - direction) for i in range(L)])
        c.extend([1] * L)

    tract(5, 0)                                            # sites 0-4 gained: left flank none
    for L in LENGTHS:
        for direction in (0, 1):
            for left in (0, 1):
                for right in (0, 1):
                    still(left)
                    tracts.append((L, direction, left, right, "pure", len(a)))
                    tract(L, direction)
                    still(right)
    for L in LENGTHS[1:]:
        for direction in (0, 1):
            for var in OPPOSITE:
                left, right = L & 1, (L >> 1) & 1
                still(left)
                if var == "bit0" and len(a) % 64:
                    still(left, 64 - len(a) % 64)
                if var == "bit63" and (len(a) + L) % 64:
                    still(left, 64 - (len(a) + L) % 64)
                tracts.append((L, direction, left, right, var, len(a)))
                tract(L, direction, {"first": 0, "last": L - 1, "middle": L // 2, "bit0": 0, "bit63": L - 1}[var])
                still(right)
    still(1, 3)
    tract(7, 1)                                            # the last 7 sites lost: right flank none
    return np.array(a, np.uint8), np.array(c, np.uint8), tracts


def _pair_paths(tree, a, c):
    """FlatPaths of the single branch with init state a and c + 0 or 2 jumps per site (so that k is not c itself)"""
    n = len(a)
    k = c.astype(np.int64) + 2 * (np.arange(n) % 3 == 0)
    T = float(tree.branches[1])
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(k)
    jumps = np.concatenate([T * (np.arange(kk) + 1.0) / (kk + 1.0) for kk in k]) if k.sum() else np.zeros(0)
    fp = FlatPaths(n, 2, a.astype(np.uint8), off, jumps)
    x = xr.rows(fp)
    assert np.array_equal(x[0], a) and np.array_equal(x[1], a ^ c)
    return fp, x


def _take_two(tree, model, fp):
    d = _dev(tree, model, fp, 16)
    d.enable_change_tracts(2)
    d.reset()
    d.accumulate_change_tracts()
    d.accumulate_change_tracts()
    return d


def test_tracts_around_word_and_bin_edges_in_every_class():
    model, tree, _ = simulate("pair", 8, seed=6)
    a, c, tracts = _laid()
    n = len(a)
    fp, x = _pair_paths(tree, a, c)
    y = x[1]
    # the layout is what it claims, by the per-site walk alone
    wh, wl = xr.brute([a.tolist()], [fp.counts().tolist()])
    for L, direction, left, right, var, at in tracts:
        assert c[at:at + L].all() and not c[at - 1] and not c[at + L] and (y[at - 1], y[at + L]) == (left, right)
        opposite = y[at:at + L] == direction
        assert opposite.sum() == (0 if var == "pure" else 1)
        if var == "bit0":
            assert at % 64 == 0 and opposite[0]
        if var == "bit63":
            assert (at + L - 1) % 64 == 63 and opposite[-1]
    for L in LENGTHS:
        for k in range(8):                                 # every pure class at every length
            assert wh[0, xr.cls_of(k >> 2, (k >> 1) & 1, k & 1), xr.bin_of(L)] >= 1
        if L > 1:
            assert wh[0, 18:, xr.bin_of(L)].sum() >= 10    # the mixed ones
    assert wh[0, xr.cls_of(0, 2, 0), 5] == 1 and wh[0, xr.cls_of(1, 1, 2), 7] == 1 and wh[0, :, 0].sum() == 0
    d = _take_two(tree, model, fp)
    assert d.change_tracts_layout()[:5] == (1, 27, 128, 0, n)
    one = xr.part(x)
    assert int(one[2][0, 0, 0]) == xr.record(5, 1, gain=1, flank=int(y[5]))
    assert int(one[2][0, 0, 1]) == xr.record(7, 0, loss=1, flank=1)
    _assert_part(d.change_tracts_part(), xr.add_parts(one, one))
    closed = d.change_tracts()
    assert closed[0] == 2 and np.array_equal(closed[1], wh * np.uint64(2)) and np.array_equal(closed[2], wl * np.uint64(2))
    # the same over an unaligned range: tiles that start in the middle of a word, both cuts inside tracts
    lo = next(s for s in range(37, n) if c[s - 1] and c[s])
    assert lo % 64 and c[n - 5] and c[n - 4]
    d.set_update_range(lo, n - 5)
    with pytest.raises(EpvError) as e:
        d.accumulate_change_tracts()
    assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    d.enable_change_tracts(2)
    d.reset()
    first, cnt = d.change_tracts_layout()[3:5]
    assert (first, cnt) == (lo, n - 5 - lo + 1)
    d.accumulate_change_tracts()
    d.accumulate_change_tracts()
    one = xr.part(x[:, first:first + cnt])
    _assert_part(d.change_tracts_part(), xr.add_parts(one, one))
    d.close()


def _chunk_sites(tree, model):
    d = _dev(tree, model, simulate("pair", 64, seed=1)[2], 16)
    d.enable_change_tracts(1)
    cs = d.change_tracts_layout()[5]
    d.close()
    return cs


@pytest.mark.parametrize("opposite_at", ["first_chunk", "far_before_second_boundary", "nowhere"])
def test_a_tract_across_both_chunk_boundaries(opposite_at):
    model, tree, _ = simulate("pair", 8, seed=6)
    cs = _chunk_sites(tree, model)
    n = 2 * cs + 5
    a = np.zeros(n, np.uint8)                                  # gains, between a flank of 1 and a flank of 0
    a[39] = 1
    c = np.zeros(n, np.uint8)
    c[40:n - 2] = 1                                            # one tract over both boundaries, cs and 2 cs
    assert (2 * cs - 40) // 64 > 256                           # (the look-back of the last chunk walks more than one step)
    site = {"first_chunk": 1000, "far_before_second_boundary": cs + 64 * 300 + 17, "nowhere": None}[opposite_at]
    if site is not None:
        assert (2 * cs - site) // 64 > 256
        a[site] = 1                                            # the one lost site
    fp, x = _pair_paths(tree, a, c)
    d = _take_two(tree, model, fp)
    assert d.change_tracts_layout() == (1, 27, 128, 0, n, cs)
    one = xr.part(x)
    k = xr.cls_of(2 if site is not None else 0, 1, 0)
    assert [int(e) for e in one[2][0, 0]] == [xr.record(0, 0), xr.record(0, 0)]
    assert one[0][0, k, xr.bin_of(n - 42)] == 1 and one[0].sum() == 1 and one[1][0, k] == n - 42
    _assert_part(d.change_tracts_part(), xr.add_parts(one, one))
    ns, hist, len_sum = d.change_tracts()
    assert ns == 2 and hist[0, k, xr.bin_of(n - 42)] == 2 and len_sum.sum() == 2 * (n - 42)
    d.close()


@pytest.mark.parametrize("density", [0.5, 0.97])
def test_dense_random_tracts_across_a_chunk_boundary(density):
    """many short tracts in the words the look-back reads, and one that crosses the boundary: the carried start is
    the last of many, and only the sites behind it count for its direction"""
    model, tree, _ = simulate("pair", 8, seed=6)
    cs = _chunk_sites(tree, model)
    n = cs + 3000
    rng = np.random.default_rng(11)
    a = rng.integers(0, 2, n).astype(np.uint8)
    c = (rng.random(n) < density).astype(np.uint8)
    c[cs - 70:cs + 70] = 1                                     # across the boundary, from more than a word before it
    c[cs - 71] = c[cs + 70] = 0
    a[cs - 200:cs - 71] = 1                                    # losses before the tract, none of them its own
    a[cs - 70:cs + 70] = 0                                     # a pure gain
    fp, x = _pair_paths(tree, a, c)
    d = _take_two(tree, model, fp)
    one = xr.part(x)
    k = xr.cls_of(0, 1, int(a[cs + 70]))                       # the crossing tract: a pure gain of 140 sites behind a 1
    assert one[0][0, k, xr.bin_of(140)] >= 1 and c[cs - 200:cs - 71].any()
    _assert_part(d.change_tracts_part(), xr.add_parts(one, one))
    wh, wl = xr.brute([a.tolist()], [fp.counts().tolist()])
    closed = d.change_tracts()
    assert np.array_equal(closed[1], wh * np.uint64(2)) and np.array_equal(closed[2], wl * np.uint64(2))
    d.close()


@pytest.mark.parametrize("state,change,n_chunks", [(0, "none", 0), (1, "all", 0), (1, "all", 2), (0, "all_but_one", 2)])
def test_all_changed_and_unchanged_rows(state, change, n_chunks):
    model, tree, _ = simulate("pair", 8, seed=6)
    n = n_chunks * _chunk_sites(tree, model) + 5 if n_chunks else 300
    a = np.full(n, state, np.uint8)
    c = np.zeros(n, np.uint8) if change == "none" else np.ones(n, np.uint8)
    if change == "all_but_one":
        c[n - 3] = 0                                           # two tracts, each open at one end of the genome
    if change != "none":
        a[5] ^= 1                                              # both directions: the bits come from the first chunk
    fp, x = _pair_paths(tree, a, c)
    d = _take_two(tree, model, fp)
    one = xr.part(x)
    y0, yl = int(x[1, 0]), int(x[1, -1])
    want = {"none": [xr.record(0, y0), xr.record(0, yl)],
            "all": [xr.record(n, y0, 1, 1, 0, True), xr.record(n, yl, 1, 1, 0, True)],
            "all_but_one": [xr.record(n - 3, y0, 1, 1, state), xr.record(2, yl, state == 0, state == 1, state)]}[change]
    assert [int(e) for e in one[2][0, 0]] == want and not one[0].any()
    _assert_part(d.change_tracts_part(), xr.add_parts(one, one))
    ns, hist, len_sum = d.change_tracts()
    assert ns == 2 and len_sum.sum() == 2 * int(c.sum())
    if change == "all":
        assert hist[0, 26, xr.bin_of(n)] == 2 and hist.sum() == 2
    d.close()


# ---- groups
@pytest.fixture(scope="module")
def one_context():
    """tree at n = 3301: one context's part and result, shared by the group tests"""
    n = 3301
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    d = _dev(tree, model, fp, cap)
    d.enable_change_tracts(BATCH)
    d.reset()
    run = d.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    part, closed = d.change_tracts_part(), d.change_tracts()
    d.close()
    return model, tree, fp, cap, n, run, part, closed


def test_local_group_of_three_equals_one_context(one_context):
    model, tree, fp, cap, n, (J1, D1, a1), part, closed = one_context
    g = LocalGroup(0, 3, sweeps_per_refresh=10)          # (halos of 256 sites: three shards fit 3301 sites)
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    assert len(g.subs) == 3
    g.enable_change_tracts(BATCH)
    with pytest.raises(RuntimeError, match="reset\\(\\) the group before taking a change-tract sample"):
        g.accumulate_change_tracts()
    g.reset()
    J3, D3, a3 = g.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert a3 == a1 and np.array_equal(J3, J1) and np.array_equal(D3, D1)
    B = tree.n_nodes - 1
    assert g.change_tracts_samples() == BATCH and g.change_tracts_layout()[:5] == (B, 27, 128, 0, n)
    assert sum(s.change_tracts_layout()[4] for s in g.subs) == n
    _assert_part(g.change_tracts_part(), part[1:])
    ns, hist, len_sum = g.change_tracts()
    assert ns == BATCH and np.array_equal(hist, closed[1]) and np.array_equal(len_sum, closed[2])
    g.reset_change_tracts()
    assert g.change_tracts_samples() == 0 and not g.change_tracts()[1].any()
    g.close()


@pytest.mark.parametrize("k", [1, 3])
def test_sharded_sampler_equals_one_context(one_context, k):
    model, tree, fp, cap, n, _, part, closed = one_context
    ss = ShardedSampler(NullComm(), 0, (lambda dev: LocalGroup(dev, 3, 10)) if k > 1 else None)
    ss.setup(model, tree, fp, [0, n], capacity=cap, sweeps_per_refresh=10)
    assert len(getattr(ss.dev, "subs", [ss.dev])) == k
    ss.enable_change_tracts(BATCH)
    ss.reset()
    ss.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=BASE)
    assert ss.change_tracts_samples() == BATCH
    _assert_part(ss.change_tracts_part(), part[1:])
    ns, hist, len_sum = ss.change_tracts()
    assert ns == BATCH and np.array_equal(hist, closed[1]) and np.array_equal(len_sum, closed[2])
    ss.reset_change_tracts()
    assert not ss.change_tracts()[1].any()
    ss.dev.close()


def test_lifecycle_and_cap():
    n = 3001
    model, tree, fp = simulate("tree", n, seed=6)
    d = _dev(tree, model, fp, _cap(fp))
    # off: nothing to read, nothing to add to, nothing counted
    for call in (d.change_tracts, d.change_tracts_part, d.accumulate_change_tracts, d.reset_change_tracts):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and OFF_TEXT in str(e.value)
    assert d.change_tracts_samples() == 0 and d.change_tracts_layout() == (0, 0, 0, 0, 0, 0)
    d.reset()
    d.run_mcmc(0, 1, 5)
    assert d.change_tracts_samples() == 0
    with pytest.raises(EpvError):
        d.enable_change_tracts(2 ** 21 + 1)
    d.enable_change_tracts(2)
    # before the first sample a new site range lays the part out again
    d.set_update_range(10, 2000)
    assert d.change_tracts_layout()[:5] == (4, 27, 128, 10, 1991)
    d.set_update_range(1, n - 2)
    d.reset()
    assert d.change_tracts_layout()[:5] == (4, 27, 128, 0, n)
    # a run whose batch would pass max_samples is refused before its first sweep
    paths = d.paths()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(1, 3, 5)
    assert e.value.code == EPV_ERR_STATE and "samples" in str(e.value) and "change tracts" in str(e.value)
    assert d.change_tracts_samples() == 0 and orc.paths_equal(d.paths(), paths)
    d.run_mcmc(0, 2, 5)
    assert d.change_tracts_samples() == 2
    ns, hist, len_sum, edges = d.change_tracts_part()
    assert np.array_equal(edges[1], xr.part(xr.rows(d.paths()))[2][0])   # the last sample is the resident paths'
    paths = d.paths()
    for call in (d.accumulate_change_tracts, lambda: d.run_mcmc(0, 1, 5, sweep_base=2)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE
    assert d.change_tracts_samples() == 2 and orc.paths_equal(d.paths(), paths)
    assert np.array_equal(d.change_tracts_part()[1], hist)
    # kept over reset, set_model and scale_jump_times; a changed range after a sample is an error
    d.reset()
    d.set_model(model)
    d.scale_jump_times(tree.branches * 2.0)
    d.reset()
    assert d.change_tracts_samples() == 2 and np.array_equal(d.change_tracts_part()[1], hist)
    d.reset_change_tracts()
    assert d.change_tracts_samples() == 0
    ns, hist0, len0, edges0 = d.change_tracts_part()
    assert ns == 0 and not hist0.any() and not len0.any() and edges0.shape == (0, 4, 2)
    d.run_mcmc(0, 1, 5, sweep_base=2)
    assert d.change_tracts_samples() == 1
    d.set_update_range(10, 2000)
    d.reset()
    for call in (d.accumulate_change_tracts, lambda: d.run_mcmc(0, 1, 5, sweep_base=3)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    assert d.change_tracts_samples() == 1
    d.enable_change_tracts(0)
    with pytest.raises(EpvError):
        d.change_tracts()
    assert d.change_tracts_layout() == (0, 0, 0, 0, 0, 0)
    d.run_mcmc(0, 1, 5, sweep_base=3)                          # off again: runs, counts nothing
    assert d.change_tracts_samples() == 0
    d.close()


def test_masked_leaf_changes_its_tracts():
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
    d.enable_change_tracts(batch)
    d.reset()
    d.run_mcmc(0, batch, 41)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=41)
    o.set_unobserved(m)
    o.reset()
    want, per_sample = _oracle_parts(o, 0, batch, 0)
    assert orc.paths_equal(d.paths(), o.paths())
    _assert_part(d.change_tracts_part(), want)
    assert any(not np.array_equal(per_sample[0][leaf - 1], h[leaf - 1]) for h in per_sample)
    d.close()


def test_sampled_root():
    """set_options(sample_root=True): the root state moves, so the changes of the branches below it do"""
    n = 1000
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    d = _dev(tree, model, fp, cap)
    d.set_options(sample_root=True)
    d.enable_change_tracts(4)
    d.reset()
    d.run_mcmc(1, 4, 23, sweep_base=2)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=23)
    o.set_sample_root(True)
    o.reset()
    want, per_sample = _oracle_parts(o, 1, 4, 2)
    assert orc.paths_equal(d.paths(), o.paths())
    root0 = fp.init.reshape(tree.n_nodes - 1, n)[0]
    assert (o.paths().init.reshape(tree.n_nodes - 1, n)[0] != root0).any()        # the root did move
    _assert_part(d.change_tracts_part(), want)
    assert any(not np.array_equal(per_sample[0][0], h[0]) for h in per_sample)
    d.close()


def test_all_twelve_layers_together():
    """every layer on at once gives what it gives alone, the twelfth included; the eleven existing read-outs are what
    they are without it"""
    n = 1201
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    enable = {
        "path_average": (7,), "branch_events": (), "window_stats": (100,), "epoch_stats": (3,), "lineage_origins": (),
        "domain_stats": (8,), "change_patterns": (), "domain_turnover": (8,), "spatial_correlation": (5, 8),
        "mixing": (4,), "domain_maps": ((1, 5, 20), 1, 8), "change_tracts": (8,)}
    read = {
        "path_average": lambda d: d.path_average(counts=True), "branch_events": lambda d: d.branch_events(counts=True),
        "window_stats": lambda d: d.window_stats(counts=True), "epoch_stats": lambda d: d.epoch_raw(),
        "lineage_origins": lambda d: d.lineage_origins(counts=True), "domain_stats": lambda d: d.domain_stats_part(),
        "change_patterns": lambda d: d.change_patterns(counts=True), "domain_turnover": lambda d: d.domain_turnover_part(),
        "spatial_correlation": lambda d: d.spatial_correlation_part(), "mixing": lambda d: d.mixing(counts=True),
        "domain_maps": lambda d: d.domain_maps_part(), "change_tracts": lambda d: d.change_tracts_part()}
    from epievo_amd.summaries import CHAIN
    assert list(enable) == [s.stem for s in CHAIN]

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
    out_eleven, eleven = run(list(enable)[:-1])
    out_none, _ = run([])
    out, alone = run(["change_tracts"])
    for (J, D, a), (Ja, Da, aa), (Jn, Dn, an), (Je, De, ae) in zip(out, out_all, out_none, out_eleven):
        assert a == aa == an == ae and np.array_equal(J, Ja) and np.array_equal(D, Da) and np.array_equal(J, Jn)
        assert np.array_equal(D, Dn) and np.array_equal(J, Je) and np.array_equal(D, De)
    assert same(alone["change_tracts"], together["change_tracts"])
    for stem in list(enable)[:-1]:
        assert same(eleven[stem], together[stem]), stem
    assert together["change_tracts"][0] == 8 and together["change_tracts"][1].any()
