"""Posterior branch-event maps counted on the device during run_mcmc (epv_set_branch_events): the six
uint32 planes equal, bit for bit, those numpy computes from the CPU oracle's paths after every batch sweep
(rung B, the same Philox sweeps; tests/bevents_ref.py) on every kernel path, for one context and a
LocalGroup of three, with masked leaf cells, over capacity growth and manual sweeps; counting changes
neither J, D, the accept count nor the paths; the window read-out equals numpy's sums of the planes."""
import numpy as np
import pytest

import bevents_ref
import orc
from common import simulate
from epievo_amd.parallel import LocalGroup
from epievo_amd.sampler import EPV_ERR_STATE, DeviceSampler, EpvError

pytestmark = pytest.mark.gpu


def _dev(tree, model, fp, cap):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    return d


def _cap(fp):
    return int(max(16, 2 * fp.counts().max() + 8))


def _oracle_planes(tree, model, fp, cap, seed, burn_in, batch, base, mask=None):
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    if mask is not None:
        o.set_unobserved(mask)
    o.reset()
    for w in range(burn_in):
        o.sweep(base + w)
    planes = np.zeros((6, tree.n_nodes - 1, fp.n_sites), np.uint32)
    deep = np.zeros(2, np.int64)          # cells with k >= 2 seen from start state 0 / 1
    for w in range(batch):
        o.sweep(base + burn_in + w)
        p = o.paths()
        planes += bevents_ref.counts(p)
        k, a = p.counts(), p.init
        deep += [int(((k >= 2) & (a == 0)).sum()), int(((k >= 2) & (a == 1)).sum())]
    return planes, o.paths(), deep


def _check_invariants(tree, fp0, planes, ns, unobserved=None):
    """what must hold per cell of any device result (fp0: the uploaded paths, whose leaf ends are the data)"""
    p = planes.astype(np.int64)
    end1, net_gain, net_loss, changed, gains, losses = p
    assert np.array_equal(gains - losses, net_gain - net_loss)
    assert (net_gain + net_loss <= changed).all() and (changed <= ns).all()
    start1 = bevents_ref.start1(planes)
    parent = np.asarray(tree.parent_ids)
    for v in range(1, tree.n_nodes):
        if parent[v] == 0:                        # below the root: one root state for all of them
            first = int(np.nonzero(parent[1:] == 0)[0][0]) + 1
            assert np.array_equal(start1[v - 1], start1[first - 1])
        else:                                     # the parent's end is this branch's start
            assert np.array_equal(start1[v - 1], end1[parent[v] - 1])
    data = bevents_ref.counts(fp0)[0]
    leaf = np.asarray(tree.subtree_sizes)[1:] == 1
    obs = np.repeat(leaf[:, None], fp0.n_sites, axis=1)
    if unobserved is not None:
        obs &= unobserved == 0
    assert np.array_equal(end1[obs], ns * data[obs].astype(np.int64))


# (EPV_PHASE_*: 1 = V2 kernels, 2 = V2 with segment-parallel jumps, 3 = fused phase, 4 = V3 large-tree kernels)
NO_FUSED = {"EPV_FUSED_PHASE": "0"}
SEG = {"EPV_FUSED_PHASE": "0", "EPV_SEG_JUMPS": "1"}


@pytest.mark.parametrize("cfg,n,env,mode", [
    ("tree", 40000, {}, 3), ("tree", 3001, NO_FUSED, 1), ("bal16", 3000, {}, 4), ("pair", 4000, SEG, 2),
    ("tree", 3, {}, None), ("tree", 257, {}, None)])
def test_planes_match_oracle_and_change_nothing(monkeypatch, cfg, n, env, mode):
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # read when a context is created
    burn_in, batch = 1, (2 if n == 3 else 3)
    model, tree, fp = simulate(cfg, n, seed=6)
    cap = _cap(fp)
    on, off = _dev(tree, model, fp, cap), _dev(tree, model, fp, cap)
    assert on.phase_mode() == off.phase_mode()
    if mode is not None:
        assert on.phase_mode() == mode
    on.enable_branch_events()
    on.reset()
    off.reset()
    # 1. nothing else changes
    J1, D1, a1 = on.run_mcmc(burn_in, batch, 77, sweep_base=5)
    J0, D0, a0 = off.run_mcmc(burn_in, batch, 77, sweep_base=5)
    assert a1 == a0 and np.array_equal(J1, J0) and np.array_equal(D1, D0)
    assert orc.paths_equal(on.paths(), off.paths())
    assert np.array_equal(on.tri_llh(), off.tri_llh())
    # 2. the planes, bit for bit
    ns, planes = on.branch_events(counts=True)
    assert ns == batch and planes.dtype == np.uint32
    assert planes.shape == (6, tree.n_nodes - 1, n)                  # sites 0 and n - 1 included
    want, opaths, deep = _oracle_planes(tree, model, fp, cap, 77, burn_in, batch, 5)
    assert orc.paths_equal(on.paths(), opaths)
    assert np.array_equal(planes, want)
    # 3. no plane is vacuous
    if n not in (3, 257):
        assert deep[0] >= 1 and deep[1] >= 1 and want[1].any() and want[2].any()
    # 4. invariants of the device result itself
    _check_invariants(tree, fp, planes, ns)
    ns2, avg = on.branch_events()
    assert ns2 == batch and np.array_equal(avg, want / float(batch))
    # 5. a read-out in the middle of a run leaves the counts alone; one more sweep adds one sample's planes
    on.run_mcmc(0, 1, 77, sweep_base=5 + burn_in + batch)
    ns3, planes3 = on.branch_events(counts=True)
    assert ns3 == batch + 1
    assert np.array_equal(planes3, planes + bevents_ref.counts(on.paths()))
    _check_invariants(tree, fp, planes3, ns3)
    on.reset_branch_events()
    ns4, planes4 = on.branch_events(counts=True)
    assert ns4 == 0 and not planes4.any()
    on.close()
    off.close()


def test_accumulate_after_manual_sweeps():
    """the caller drives the sweeps and takes a sample when it likes; branch lengths do not matter"""
    model, tree, fp = simulate("tree", 5000, seed=3)
    cap = _cap(fp)
    d = _dev(tree, model, fp, cap)
    d.enable_branch_events()
    d.reset()
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=21)
    o.reset()
    want = np.zeros((6, tree.n_nodes - 1, 5000), np.uint32)
    for w in range(3):
        assert d.sweep(1, 21, sweep_base=w) == o.sweep(w)
        d.accumulate_branch_events()
        want += bevents_ref.counts(o.paths())
    ns, planes = d.branch_events(counts=True)
    assert ns == 3 and np.array_equal(planes, want)
    # new branch lengths move the jump times, not what is counted: there is no grid to refresh
    d.scale_jump_times(tree.branches * 1.25)
    d.accumulate_branch_events()
    want += bevents_ref.counts(o.paths())
    ns, planes = d.branch_events(counts=True)
    assert ns == 4 and np.array_equal(planes, want)
    _check_invariants(tree, fp, planes, ns)
    d.close()


def test_counts_survive_capacity_growth():
    """a deliberately tiny capacity: overflows widen the jump slots between batch sweeps (auto_grow);
    the planes keep accumulating and match the oracle run at the same capacities"""
    model, tree, fp = simulate("pair", 2000, seed=8)
    cap = int(fp.counts().max())
    d = _dev(tree, model, fp, cap)
    d.auto_grow = True
    d.enable_branch_events()
    d.reset()
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=4)
    o.reset()
    want = np.zeros((6, 1, 2000), np.uint32)
    for w in range(4):
        d.run_mcmc(0, 1, 4, sweep_base=w)
        o.sweep(w)
        want += bevents_ref.counts(o.paths())
        o.set_rung("B", d.capacity())
    assert d.capacity() > cap and d.capacity_events
    ns, planes = d.branch_events(counts=True)
    assert ns == 4 and np.array_equal(planes, want)
    d.close()


@pytest.fixture(scope="module")
def counted():
    """one context with a few samples, shared by the read-out tests (which only read)"""
    n = 5003
    model, tree, fp = simulate("tree", n, seed=2)
    d = _dev(tree, model, fp, _cap(fp))
    d.enable_branch_events()
    d.reset()
    d.run_mcmc(1, 3, 13)
    ns, planes = d.branch_events(counts=True)
    assert ns == 3 and planes[3].any()
    yield d, n, planes
    d.close()


@pytest.mark.parametrize("W", [1, 7, 64, 1000, 10 ** 6])
def test_windows_equal_numpy_sums(counted, W):
    d, n, planes = counted
    ns, win = d.branch_event_windows(W)
    assert ns == 3 and win.dtype == np.uint64 and win.shape == (6, planes.shape[1], (n + W - 1) // W)
    assert np.array_equal(win, bevents_ref.windows(planes, W))
    assert np.array_equal(win, np.add.reduceat(planes.astype(np.uint64), np.arange(0, n, W), axis=2))
    if W == 1:
        assert np.array_equal(win, planes)
    # a piece of the windows, and windows beyond the genome: zeros there
    nw = win.shape[2]
    _, some = d.branch_event_windows(W, first_window=nw // 2, n_windows=nw - nw // 2 + 3)
    assert np.array_equal(some[:, :, :nw - nw // 2], win[:, :, nw // 2:]) and not some[:, :, nw - nw // 2:].any()
    assert np.array_equal(d.branch_events(counts=True)[1], planes)     # the accumulator is only read


def test_windows_outside_the_counted_range_are_zero():
    """a context that counts sites 2 .. n - 3 of a longer genome: windows elsewhere are zero, and the windows
    on its edges hold its own sites only"""
    n, g0, ng = 3001, 5000, 20000
    model, tree, fp = simulate("tree", n, seed=6)
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, _cap(fp), g0, ng)
    d.set_update_range(2, n - 3)               # a shard in the middle of the genome: two halo columns a side
    d.enable_branch_events()
    d.reset()
    d.run_mcmc(0, 2, 3)
    first, cnt = d.branch_events_layout()
    assert (first, cnt) == (2, n - 4)
    ns, planes = d.branch_events(counts=True)
    assert ns == 2 and planes.shape[2] == n - 4
    for W in (1, 7, 64, 1000, 10 ** 6):
        _, win = d.branch_event_windows(W)
        assert np.array_equal(win, bevents_ref.windows(planes, W, first_site=g0 + 2, n_global=ng))
        lo, hi = (g0 + 2) // W, (g0 + n - 3) // W
        assert not win[:, :, :lo].any() and not win[:, :, hi + 1:].any() and win[0].any()
    d.close()


@pytest.mark.parametrize("cfg,n", [("tree", 20011), ("bal16", 9000)])
def test_local_group_equals_single_context(cfg, n):
    model, tree, fp = simulate(cfg, n, seed=4)
    cap, P = _cap(fp), 11
    ev, pa = _dev(tree, model, fp, cap), _dev(tree, model, fp, cap)     # each accumulator alone
    g = LocalGroup(0, 3)                                                # both together, three contexts
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    assert len(g.subs) == 3
    ev.enable_branch_events()
    pa.enable_path_average(P)
    g.enable_branch_events()
    g.enable_path_average(P)
    res = []
    for s in (ev, pa, g):
        s.reset()
        res.append(s.run_mcmc(1, 3, 99, sweep_base=7))
    for J, D, nacc in res[1:]:
        assert nacc == res[0][2] and np.array_equal(J, res[0][0]) and np.array_equal(D, res[0][1])
    nse, pe = ev.branch_events(counts=True)
    nsg, pg = g.branch_events(counts=True)
    assert nse == nsg == 3 and pg.shape == (6, tree.n_nodes - 1, n)
    assert np.array_equal(pe, pg)
    want, _, _ = _oracle_planes(tree, model, fp, cap, 99, 1, 3, 7)
    assert np.array_equal(pg, want)
    _check_invariants(tree, fp, pg, 3)
    # windows: 1000 divides none of the shard cuts, so the shards' contributions to a window add up
    assert any(a % 1000 for a in g.a[1:])
    nw1, we = ev.branch_event_windows(1000)
    nw3, wg = g.branch_event_windows(1000)
    assert nw1 == nw3 == 3 and np.array_equal(we, wg) and np.array_equal(wg, bevents_ref.windows(want, 1000))
    # the path average next to the events is the path average alone
    assert np.array_equal(g.path_average(counts=True)[1], pa.path_average(counts=True)[1])
    for s in (ev, pa, g):
        s.close()


def test_open_leaf_cells_are_imputed():
    n = 601
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    # the leaf on the longest branch: the chance that an open cell's state differs from its parent's grows with
    # the branch length, so that is where eight sweeps are likeliest to visit both states (on the 0.03 branch
    # of the first leaf the oracle's chain keeps all eight cells where they start)
    leaves = [b for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1]
    leaf = max(leaves, key=lambda b: tree.branches[b])
    m = np.zeros((tree.n_nodes - 1, n), np.uint8)
    cells = [1, 31, 32, 33, 63, 64, 65, n - 2]
    m[leaf - 1, cells] = 1
    d = _dev(tree, model, fp, cap)
    d.set_unobserved(m)
    d.enable_branch_events()
    d.reset()
    d.run_mcmc(0, 8, 41)
    ns, planes = d.branch_events(counts=True)
    assert ns == 8
    _check_invariants(tree, fp, planes, ns, unobserved=m)        # observed leaf cells: samples x data
    open_end1 = planes[0, leaf - 1, cells]
    assert ((open_end1 > 0) & (open_end1 < ns)).any(), open_end1  # an imputed state, neither 0 nor 1
    want, opaths, _ = _oracle_planes(tree, model, fp, cap, 41, 0, 8, 0, mask=m)
    assert orc.paths_equal(d.paths(), opaths)
    assert np.array_equal(planes, want)
    d.close()


def test_errors():
    model, tree, fp = simulate("tree", 3001, seed=6)
    d = _dev(tree, model, fp, _cap(fp))
    # off: nothing to read, nothing to add to
    for call in (d.branch_events, lambda: d.branch_event_windows(10), d.accumulate_branch_events,
                 d.reset_branch_events):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE
    assert d.branch_events_samples() == 0 and d.branch_events_layout() == (0, 0)
    d.reset()
    d.run_mcmc(0, 1, 5)                        # off costs nothing and counts nothing
    assert d.branch_events_samples() == 0
    d.enable_branch_events()
    assert d.branch_events_layout() == (0, 3001)
    # before the first sample a new site range lays the planes out again; afterwards it is an error
    d.set_update_range(10, 2000)
    assert d.branch_events_layout() == (10, 1991)
    d.set_update_range(1, 2999)
    d.reset()
    d.run_mcmc(0, 1, 5)
    assert d.branch_events_samples() == 1
    d.set_update_range(10, 2000)
    d.reset()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(0, 1, 5, sweep_base=1)
    assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    d.set_update_range(1, 2999)
    d.reset()
    # the sample cap: 2^21 samples fill the 32-bit counts (g <= 1024 per sample)
    planes = d.branch_events(counts=True)[1]
    d._ck(d.L.epv_branch_events_set_samples(d.h, 2 ** 21 - 1))
    d.run_mcmc(0, 1, 5, sweep_base=2)          # the last sample that fits
    assert d.branch_events_samples() == 2 ** 21
    paths = d.paths()
    for call in (d.accumulate_branch_events, lambda: d.run_mcmc(0, 1, 5, sweep_base=3)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and "2^21" in str(e.value)
    assert orc.paths_equal(d.paths(), paths)   # a refused run has not swept
    assert np.array_equal(d.branch_events(counts=True)[1], planes + bevents_ref.counts(paths))
    d.enable_branch_events(False)
    with pytest.raises(EpvError):
        d.branch_events()
    d.close()
