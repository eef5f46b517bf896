"""Change patterns counted on the device during run_mcmc (epv_set_change_patterns): the R = 12 + 2 (N-1) + I
uint32 rows equal, bit for bit, those numpy computes from the CPU oracle's paths after every batch sweep (rung B,
the same Philox sweeps; tests/patterns_ref.py) on every kernel path and on the tree shapes at which the kernel's
walk can go wrong, for one context and a LocalGroup of three, with masked leaf cells and a sampled root, over
capacity growth and manual sweeps; counting changes neither J, D, the accept count nor the paths; the window
read-out equals numpy's sums of the rows; all seven summaries together give what each gives alone."""
import numpy as np
import pytest

import bevents_ref
import orc
import patterns_ref
import test_summaries_together_gpu as six
from common import _tmp, ref_test_model, simulate
from epievo_amd import host
from epievo_amd.parallel import LocalGroup
from epievo_amd.sampler import EPV_ERR_STATE, DeviceSampler, EpvError

pytestmark = pytest.mark.gpu

OFF_TEXT = "change patterns are off: epv_set_change_patterns first"
# a caterpillar of five leaves: B = 8 branches, exactly one full chunk of the kernel's walk
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


def _oracle_rows(tree, model, fp, cap, seed, burn_in, batch, base, mask=None, sample_root=False):
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    if mask is not None:
        o.set_unobserved(mask)
    if sample_root:
        o.set_sample_root(True)
    o.reset()
    for w in range(burn_in):
        o.sweep(base + w)
    rows = np.zeros((patterns_ref.n_rows(tree), fp.n_sites), np.uint32)
    for w in range(batch):
        o.sweep(base + burn_in + w)
        rows += patterns_ref.counts(o.paths(), tree)
    return rows, o.paths()


def _check_invariants(tree, rows, ns, planes=None):
    """what must hold per site of any device result (planes: the branch events of the same run)"""
    B = tree.n_nodes - 1
    r = rows.astype(np.int64)
    changed = r[:7].sum(axis=0)
    sole = r[12:12 + 2 * B].sum(axis=0)
    one = r[patterns_ref.ONE_BRANCH]
    assert (changed <= ns).all()
    assert (r[0] <= sole).all() and (sole <= one).all() and (one <= changed).all()
    assert (one - sole <= r[patterns_ref.REVERTED]).all()
    for row in (patterns_ref.PAR_GAIN, patterns_ref.PAR_LOSS, patterns_ref.GAIN_AND_LOSS):
        assert (r[row] <= changed - one).all()
    clades = patterns_ref.clade_nodes(tree)
    for j, v in enumerate(clades):
        cl = r[12 + 2 * B + j]
        assert (cl <= changed).all()
        for i, u in enumerate(clades):             # u strictly inside v's clade: a child clade
            if v < u < v + int(tree.subtree_sizes[v]):
                assert (r[12 + 2 * B + i] <= cl).all()
    if not clades and all(int(p) == 0 for p in tree.parent_ids):       # a star
        assert not r[patterns_ref.GAIN_AND_LOSS].any()
    if B == 1:
        assert np.array_equal(one, changed) and not r[8:11].any()
    if planes is not None:
        p = planes.astype(np.int64)
        assert (r[12:12 + B] <= p[1]).all() and (r[12 + B:12 + 2 * B] <= p[2]).all()
        assert (p[3].sum(axis=0) >= changed).all()
        # a site of jumps_7plus holds at least seven jumps
        assert ((p[4] + p[5]).sum(axis=0) >= sum((h + 1) * r[h] for h in range(7))).all()


# (EPV_PHASE_*: 1 = V2 kernels, 2 = V2 with segment-parallel jumps, 3 = fused phase, 4 = V3 large-tree kernels)
NO_FUSED = {"EPV_FUSED_PHASE": "0"}
SEG = {"EPV_FUSED_PHASE": "0", "EPV_SEG_JUMPS": "1"}
# cfg, n, env, mode, batch sweeps, rows R
CASES = [
    ("tree", 40000, {}, 3, 3, 21),
    ("tree", 3001, NO_FUSED, 1, 3, 21),
    ("pair", 4000, SEG, 2, 3, 14),
    ("bal16", 3000, {}, 4, 3, 86),
    ("cat6", 3000, {}, None, 3, 36),
    ("multi", 3000, {}, None, 3, 30),
    ("star4", 257, {}, None, 3, 20),
    ("tree", 3, {}, None, 2, 21),
    ("cat5", 3000, {}, None, 3, 12 + 16 + 3),
]


@pytest.mark.parametrize("cfg,n,env,mode,batch,R", CASES, ids=["%s-%d" % c[:2] for c in CASES])
def test_rows_match_oracle_and_change_nothing(monkeypatch, cfg, n, env, mode, batch, R):
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # read when a context is created
    burn_in = 1
    model, tree, fp = _inputs(cfg, n)
    cap = _cap(fp)
    on, off = _dev(tree, model, fp, cap), _dev(tree, model, fp, cap)
    assert on.phase_mode() == off.phase_mode()
    if mode is not None:
        assert on.phase_mode() == mode
    on.enable_change_patterns()
    on.enable_branch_events()             # (for the invariants that tie the two together)
    on.reset()
    off.reset()
    # 1. nothing else changes
    J1, D1, a1 = on.run_mcmc(burn_in, batch, 77, sweep_base=5)
    J0, D0, a0 = off.run_mcmc(burn_in, batch, 77, sweep_base=5)
    assert a1 == a0 and np.array_equal(J1, J0) and np.array_equal(D1, D0)
    assert orc.paths_equal(on.paths(), off.paths())
    assert np.array_equal(on.tri_llh(), off.tri_llh())
    # 2. the rows, bit for bit
    ns, rows = on.change_patterns(counts=True)
    assert ns == batch and rows.dtype == np.uint32 and rows.shape == (R, n)       # sites 0 and n - 1 included
    Rl, clades, first, cnt = on.change_patterns_layout()
    assert (Rl, first, cnt) == (R, 0, n) and list(clades) == patterns_ref.clade_nodes(tree)
    want, opaths = _oracle_rows(tree, model, fp, cap, 77, burn_in, batch, 5)
    assert orc.paths_equal(on.paths(), opaths)
    assert np.array_equal(rows, want)
    # 3. no row is vacuous: on the reference alone
    if cfg in ("cat6", "multi", "bal16"):
        tot = want.sum(axis=1, dtype=np.int64)
        assert (tot > 0).all(), [nm for nm, t in zip(patterns_ref.row_names(tree), tot) if not t]
    elif n > 300:
        assert want[:3].any(axis=1).all() and want[patterns_ref.ONE_BRANCH].any()
        assert want[12:12 + 2 * (tree.n_nodes - 1)].any()
    # 4. invariants of the device result itself
    _check_invariants(tree, rows, ns, on.branch_events(counts=True)[1])
    ns2, avg = on.change_patterns()
    assert ns2 == batch and np.array_equal(avg, want / float(batch))
    s = host.change_pattern_summary(ns, rows, tree)
    assert np.array_equal(s["conserved"], 1.0 - want[:7].sum(axis=0) / float(batch))
    # 5. a read-out in the middle of a run leaves the counts alone; one more sweep adds one sample's rows
    on.run_mcmc(0, 1, 77, sweep_base=5 + burn_in + batch)
    ns3, rows3 = on.change_patterns(counts=True)
    assert ns3 == batch + 1
    assert np.array_equal(rows3, rows + patterns_ref.counts(on.paths(), tree))
    _check_invariants(tree, rows3, ns3, on.branch_events(counts=True)[1])
    on.reset_change_patterns()
    ns4, rows4 = on.change_patterns(counts=True)
    assert ns4 == 0 and not rows4.any()
    on.close()
    off.close()


def test_accumulate_after_manual_sweeps():
    """the caller drives the sweeps and takes a sample when it likes; branch lengths do not matter"""
    n = 3000
    model, tree, fp = simulate("cat6", n, seed=3)
    cap = _cap(fp)
    d = _dev(tree, model, fp, cap)
    d.enable_change_patterns()
    d.reset()
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=21)
    o.reset()
    want = np.zeros((36, n), np.uint32)
    for w in range(3):
        assert d.sweep(1, 21, sweep_base=w) == o.sweep(w)
        d.accumulate_change_patterns()
        want += patterns_ref.counts(o.paths(), tree)
    ns, rows = d.change_patterns(counts=True)
    assert ns == 3 and np.array_equal(rows, want)
    d.scale_jump_times(tree.branches * 1.25)           # new branch lengths move the jump times, not what is counted
    d.accumulate_change_patterns()
    want += patterns_ref.counts(o.paths(), tree)
    ns, rows = d.change_patterns(counts=True)
    assert ns == 4 and np.array_equal(rows, want)
    _check_invariants(tree, rows, ns)
    d.close()


def test_counts_survive_capacity_growth():
    """a deliberately tiny capacity: overflows widen the jump slots between batch sweeps (auto_grow); the rows
    keep accumulating and match the oracle run at the same capacities"""
    model, tree, fp = simulate("pair", 2000, seed=8)
    cap = int(fp.counts().max())
    d = _dev(tree, model, fp, cap)
    d.auto_grow = True
    d.enable_change_patterns()
    d.reset()
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=4)
    o.reset()
    want = np.zeros((14, 2000), np.uint32)
    for w in range(4):
        d.run_mcmc(0, 1, 4, sweep_base=w)
        o.sweep(w)
        want += patterns_ref.counts(o.paths(), tree)
        o.set_rung("B", d.capacity())
    assert d.capacity() > cap and d.capacity_events
    ns, rows = d.change_patterns(counts=True)
    assert ns == 4 and np.array_equal(rows, want)
    d.close()


@pytest.fixture(scope="module")
def counted():
    """one context with a few samples, shared by the read-out tests (which only read)"""
    n = 3003
    model, tree, fp = simulate("cat6", n, seed=2)
    d = _dev(tree, model, fp, _cap(fp))
    d.enable_change_patterns()
    d.reset()
    d.run_mcmc(1, 3, 13)
    ns, rows = d.change_patterns(counts=True)
    assert ns == 3 and rows.any(axis=1).sum() >= 30
    yield d, n, rows
    d.close()


@pytest.mark.parametrize("W", [1, 7, 64, 100, 300, 10 ** 6])
def test_windows_equal_numpy_sums(counted, W):
    d, n, rows = counted
    ns, win = d.change_pattern_windows(W)
    assert ns == 3 and win.dtype == np.uint64 and win.shape == (rows.shape[0], (n + W - 1) // W)
    assert np.array_equal(win, patterns_ref.windows(rows, W))
    assert np.array_equal(win, np.add.reduceat(rows.astype(np.uint64), np.arange(0, n, W), axis=1))
    if W == 1:
        assert np.array_equal(win, rows)
    # a piece of the windows, and windows beyond the genome: zeros there
    nw = win.shape[1]
    _, some = d.change_pattern_windows(W, first_window=nw // 2, n_windows=nw - nw // 2 + 3)
    assert np.array_equal(some[:, :nw - nw // 2], win[:, nw // 2:]) and not some[:, nw - nw // 2:].any()
    assert np.array_equal(d.change_patterns(counts=True)[1], rows)     # the accumulator is only read


def test_windows_outside_the_counted_range_are_zero():
    """a context that counts sites 2 .. n - 3 of a longer genome: windows elsewhere are zero, and the windows on
    its edges hold its own sites only"""
    n, g0, ng = 3001, 5000, 20000
    model, tree, fp = simulate("tree", n, seed=6)
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, _cap(fp), g0, ng)
    d.set_update_range(2, n - 3)               # a shard in the middle of the genome: two halo columns a side
    d.enable_change_patterns()
    d.reset()
    d.run_mcmc(0, 2, 3)
    assert d.change_patterns_layout()[2:] == (2, n - 4)
    ns, rows = d.change_patterns(counts=True)
    assert ns == 2 and rows.shape == (21, n - 4) and rows.any()
    for W in (1, 7, 64, 1000, 10 ** 6):
        _, win = d.change_pattern_windows(W)
        assert np.array_equal(win, patterns_ref.windows(rows, W, first_site=g0 + 2, n_global=ng))
        lo, hi = (g0 + 2) // W, (g0 + n - 3) // W
        assert not win[:, :lo].any() and not win[:, hi + 1:].any() and win.any()
    d.close()


def test_local_group_equals_single_context():
    n = 3300
    model, tree, fp = simulate("cat6", n, seed=4)
    cap = _cap(fp)
    one = _dev(tree, model, fp, cap)
    g = LocalGroup(0, shards=3, sweeps_per_refresh=10)
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    assert len(g.subs) == 3
    res = []
    for s in (one, g):
        s.enable_change_patterns()
        s.reset()
        res.append(s.run_mcmc(1, 3, 99, sweep_base=7))
    assert res[1][2] == res[0][2] and np.array_equal(res[1][0], res[0][0]) and np.array_equal(res[1][1], res[0][1])
    ns1, r1 = one.change_patterns(counts=True)
    nsg, rg = g.change_patterns(counts=True)
    assert ns1 == nsg == g.change_patterns_samples() == 3 and rg.shape == (36, n)
    assert np.array_equal(r1, rg)
    want, _ = _oracle_rows(tree, model, fp, cap, 99, 1, 3, 7)
    assert np.array_equal(rg, want)
    _check_invariants(tree, rg, 3)
    # windows: 100 divides none of the shard cuts, so the shards' contributions to a window add up
    assert any(a % 100 for a in g.a[1:])
    nw1, w1 = one.change_pattern_windows(100)
    nw3, wg = g.change_pattern_windows(100)
    assert nw1 == nw3 == 3 and np.array_equal(w1, wg) and np.array_equal(wg, patterns_ref.windows(want, 100))
    one.close()
    g.close()


def test_masked_leaf_cells():
    n = 601
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    leaves = [b for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1]
    leaf = max(leaves, key=lambda b: tree.branches[b])
    m = np.zeros((tree.n_nodes - 1, n), np.uint8)
    m[leaf - 1, [1, 31, 32, 33, 63, 64, 65, n - 2]] = 1
    d = _dev(tree, model, fp, cap)
    d.set_unobserved(m)
    d.enable_change_patterns()
    d.reset()
    d.run_mcmc(0, 8, 41)
    ns, rows = d.change_patterns(counts=True)
    want, opaths = _oracle_rows(tree, model, fp, cap, 41, 0, 8, 0, mask=m)
    assert ns == 8 and orc.paths_equal(d.paths(), opaths)
    assert np.array_equal(rows, want) and want.any()
    _check_invariants(tree, rows, ns)
    d.close()


def test_sampled_root():
    """set_options(sample_root=True): the root state moves, so the init states of the branches below it do"""
    n = 1000
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    d = _dev(tree, model, fp, cap)
    d.set_options(sample_root=True)
    d.enable_change_patterns()
    d.reset()
    d.run_mcmc(1, 4, 23, sweep_base=2)
    ns, rows = d.change_patterns(counts=True)
    want, opaths = _oracle_rows(tree, model, fp, cap, 23, 1, 4, 2, sample_root=True)
    assert ns == 4 and orc.paths_equal(d.paths(), opaths)
    root0 = fp.init.reshape(tree.n_nodes - 1, n)[0]
    assert (opaths.init.reshape(tree.n_nodes - 1, n)[0] != root0).any()            # the root did move
    assert np.array_equal(rows, want) and want.any()
    _check_invariants(tree, rows, ns)
    d.close()


def test_lifecycle_and_errors():
    model, tree, fp = simulate("tree", 3001, seed=6)
    d = _dev(tree, model, fp, _cap(fp))
    # off: nothing to read, nothing to add to
    for call in (d.change_patterns, lambda: d.change_pattern_windows(10), d.accumulate_change_patterns,
                 d.reset_change_patterns):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and OFF_TEXT in str(e.value)
    assert d.change_patterns_samples() == 0 and d.change_patterns_layout()[0] == 0
    d.reset()
    d.run_mcmc(0, 1, 5)                        # off costs nothing and counts nothing
    assert d.change_patterns_samples() == 0
    d.enable_change_patterns()
    assert d.change_patterns_layout()[2:] == (0, 3001)
    # before the first sample a new site range lays the rows out again; afterwards it is an error
    d.set_update_range(10, 2000)
    assert d.change_patterns_layout()[2:] == (10, 1991)
    d.set_update_range(1, 2999)
    d.reset()
    d.run_mcmc(0, 1, 5)
    assert d.change_patterns_samples() == 1
    rows = d.change_patterns(counts=True)[1]
    assert np.array_equal(rows, patterns_ref.counts(d.paths(), tree))
    d.set_update_range(10, 2000)
    d.reset()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(0, 1, 5, sweep_base=1)
    assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    d.set_update_range(1, 2999)
    d.reset()
    # off then on starts from zero
    d.enable_change_patterns(False)
    with pytest.raises(EpvError) as e:
        d.change_patterns()
    assert OFF_TEXT in str(e.value) and d.change_patterns_samples() == 0
    d.enable_change_patterns()
    ns, rows = d.change_patterns(counts=True)
    assert ns == 0 and rows.shape == (21, 3001) and not rows.any()
    d.close()


SEVEN = six.LAYERS + ("change_patterns",)


def test_all_seven_on_equal_each_alone():
    """all seven summaries on give the integers each gives alone; the six existing read-outs are unchanged by the
    seventh"""
    model, tree, fp = simulate("tree", six.N_SITES, seed=4)
    cap = six._cap(fp)
    enable = dict(six.ENABLE, change_patterns=lambda d: d.enable_change_patterns(True))
    read = dict(six.READ, change_patterns=lambda d: d.change_patterns(counts=True))

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
    for name in SEVEN:
        d = dev((name,))
        assert six._same_run(six._run(d), plain), name
        alone[name] = read[name](d)
        assert alone[name][0] == six.BATCH and any(np.asarray(x).any() for x in alone[name][1:]), name
        d.close()
    d6 = dev(six.LAYERS)
    assert six._same_run(six._run(d6), plain)
    d7 = dev(SEVEN[::-1])                            # (switched on against the order of the chain)
    assert six._same_run(six._run(d7), plain)
    for name in SEVEN:
        assert six._same_readout(read[name](d7), alone[name]), name
    for name in six.LAYERS:
        assert six._same_readout(read[name](d7), read[name](d6)), name
    assert d7.change_patterns_samples() == six.BATCH
    d6.close()
    d7.close()
