"""Regional sufficient statistics on the device (epv_set_window_stats): J and D per window of W global sites,
added over the batch sweeps of run_mcmc as exact integers.

Identity A: added over all windows (and all contexts of a genome) the accumulator equals the sum over the batch
sweeps of the counts run_mcmc_counts returns for the same run.  Identity B: window w equals the sum over the
batch sweeps of rung B (same Philox sweeps) of row w of orc_suffstats_rows (tests/wstat_ref.py).  Both bit for
bit, on every colour-phase kernel path, for window sizes below, at and above the 64-site tile, on dense histories
(every pair on the merge path), for three contexts whose shard cuts fall inside windows, and over the life cycle.
Counting changes neither J, D, the accept count, the paths, tri_llh nor the plan."""
import numpy as np
import pytest

import dense_cases as dc
import orc
import wstat_ref
from common import simulate
from epievo_amd.parallel import LocalGroup, NullComm, ShardedSampler
from epievo_amd.sampler import EPV_ERR_STATE, DeviceSampler, EpvError

pytestmark = pytest.mark.gpu

NO_FUSED = {"EPV_FUSED_PHASE": "0"}
SEG = {"EPV_FUSED_PHASE": "0", "EPV_SEG_JUMPS": "1"}
SEED, BASE, BURN_IN, BATCH = 77, 5, 1, 3


def _dev(tree, model, fp, cap):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    return d


def _cap(fp):
    return int(max(16, 2 * fp.counts().max() + 8))


def _oracle_run(tree, model, fp, cap, Ws, seed=SEED, burn_in=BURN_IN, batch=BATCH, base=BASE):
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    o.reset()
    acc, tot = wstat_ref.run(o, fp.n_sites, Ws, burn_in, batch, base)
    return acc, tot, o


# (EPV_PHASE_*: 1 = V2 kernels, 2 = V2 with segment-parallel jumps, 3 = fused phase, 4 = V3 large-tree kernels)
@pytest.mark.parametrize("cfg,n,env,mode,Ws", [
    ("tree", 3001, {}, 3, (1, 64, 100)),
    ("tree", 3001, NO_FUSED, 1, (3, 256)),
    ("pair", 1500, SEG, 2, (1, 100)),
    ("bal16", 700, {}, 4, (3, 64, 256)),       # B = 30: four branch chunks, the last of six
    ("tree", 3, {}, None, (1, 3)),             # one interior site
    ("tree", 65, {}, None, (1, 64)),           # tile and block edges: an edge column on either side
    ("tree", 257, {}, None, (1, 3, 1000)),     # 1000: one window, clamped to the genome
    ("tree", 258, {}, None, (3, 256))])
def test_windows_match_oracle_and_change_nothing(monkeypatch, cfg, n, env, mode, Ws):
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # read when a context is created
    batch = 2 if n == 3 else BATCH
    model, tree, fp = simulate(cfg, n, seed=6)
    cap, B = _cap(fp), tree.n_nodes - 1
    want, tot, o = _oracle_run(tree, model, fp, cap, Ws, batch=batch)
    if n >= 65:                               # not vacuous: jumps in two or more windows, none in another
        assert wstat_ref.not_vacuous(want[min(Ws)])
    off = _dev(tree, model, fp, cap)
    if mode is not None:
        assert off.phase_mode() == mode
    off.reset()
    counts0, a0 = off.run_mcmc_counts(BURN_IN, batch, SEED, sweep_base=BASE)
    assert np.array_equal(counts0.reshape(batch, B, 16), tot)
    J0, D0 = off.counts_to_stats(counts0, batch)
    for i, W in enumerate(Ws):
        on = _dev(tree, model, fp, cap)
        assert on.phase_mode() == off.phase_mode() and on.phase_plan() == off.phase_plan()
        on.enable_window_stats(W)
        Wc = min(W, n)
        nw = (n + Wc - 1) // Wc
        assert on.window_stats_layout() == (Wc, 1 // Wc, (n - 2) // Wc - 1 // Wc + 1)
        on.reset()
        # nothing else changes (the statistics of the run through either of the two statistics kernels)
        if i % 2 == 0:
            J1, D1, a1 = on.run_mcmc(BURN_IN, batch, SEED, sweep_base=BASE)
        else:
            c1, a1 = on.run_mcmc_counts(BURN_IN, batch, SEED, sweep_base=BASE)
            assert np.array_equal(c1, counts0)
            J1, D1 = on.counts_to_stats(c1, batch)
        assert a1 == a0 and np.array_equal(J1, J0) and np.array_equal(D1, D0)
        assert orc.paths_equal(on.paths(), off.paths()) and orc.paths_equal(on.paths(), o.paths())
        assert np.array_equal(on.tri_llh(), off.tri_llh())
        assert on.phase_plan() == off.phase_plan()
        ns, got = on.window_stats(counts=True)
        assert ns == batch and got.dtype == np.int64 and got.shape == (nw, B, 16)
        assert np.array_equal(got, want[W]), W                                   # identity B
        assert np.array_equal(got.sum(axis=0), counts0.reshape(batch, B, 16).sum(axis=0))   # identity A
        ns, J, D = on.window_stats()
        Jw, Dw = wstat_ref.to_stats(want[W], wstat_ref.scales(o), batch)
        assert ns == batch and np.array_equal(J, Jw) and np.array_equal(D, Dw)
        assert np.array_equal(np.ldexp(1.0, on.window_stats_scale_exps()), wstat_ref.scales(o)[1:])
        # a piece of the windows, and windows beyond the genome: zeros there
        _, some = on.window_counts(first_window=nw // 2, n_windows=nw - nw // 2 + 2)
        assert np.array_equal(some[:nw - nw // 2], got[nw // 2:]) and not some[nw - nw // 2:].any()
        on.close()
    off.close()


@pytest.mark.parametrize("name,n,share", [("weak-pair4", 600, 1.0), ("weak-bal16x60", 300, 0.99),
                                           ("flat-bal16x300", 200, 1.0)])
def test_dense_histories(name, n, share):
    """an interior (site, branch) triple with a jump on one of its three paths does not take the no-jump histogram:
    it is queued in the ring and merged by merge3.  On weak-pair4 and flat-bal16x300 that is every triple of the
    input, on weak-bal16x60 all but a few in a thousand.  On weak-pair4 (one branch) a block queues its 64 triples
    once; on the 16-leaf tree a block queues up to 64 per branch of its chunk of eight, so the 128-entry ring
    wraps"""
    model, tree, fp = dc.workload(name, n)
    cap, B = dc.capacity(name, fp), tree.n_nodes - 1
    assert dc.density(fp)["mean"] >= 2.0 and fp.n_sites == n <= 600
    nj = fp.counts().reshape(B, n)
    on_merge_path = nj[:, :-2] + nj[:, 1:-1] + nj[:, 2:] > 0
    assert on_merge_path.all() if share == 1.0 else on_merge_path.mean() >= share
    if name != "weak-pair4":
        assert B > 8
    Ws = (1, 100)
    o = dc.oracle(name, cap, n=n)
    want, tot = wstat_ref.run(o, n, Ws, BURN_IN, BATCH, BASE)
    for W in Ws:
        d = _dev(tree, model, fp, cap)
        d.enable_window_stats(W)
        d.reset()
        c, _ = d.run_mcmc_counts(BURN_IN, BATCH, dc.ORACLE_SEED, sweep_base=BASE)
        assert orc.paths_equal(d.paths(), o.paths())
        assert np.array_equal(c.reshape(BATCH, B, 16), tot)
        ns, got = d.window_stats(counts=True)
        assert ns == BATCH and np.array_equal(got, want[W])
        d.close()


@pytest.mark.parametrize("n,spr,k", [(1000, 60, None), (3100, 10, 3)])
def test_local_group_equals_single_context(n, spr, k):
    """a LocalGroup of three: ("tree", 1000) is too short to be cut (the group falls back to fewer contexts, which
    must not show either); ("tree", 3100) with the narrowest halos gives three contexts, cut at 1024 and 2048 --
    inside windows of 7 and of 100 sites"""
    model, tree, fp = simulate("tree", n, seed=4)
    cap, B = _cap(fp), tree.n_nodes - 1
    Ws = (7, 100)
    want, tot, o = _oracle_run(tree, model, fp, cap, Ws, seed=99, base=7)
    for W in Ws:
        one = _dev(tree, model, fp, cap)
        g = LocalGroup(0, 3, sweeps_per_refresh=spr)
        g.set_tree(tree)
        g.set_model(model)
        g.upload_paths(fp, cap)
        if k is not None:
            assert len(g.subs) == k and all(a % W for a in g.a[1:])
        one.enable_window_stats(W)
        g.enable_window_stats(W)
        res = []
        for s in (one, g):
            s.reset()
            res.append(s.run_mcmc(1, 3, 99, sweep_base=7))
        assert res[0][2] == res[1][2] and np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        ns1, c1 = one.window_stats(counts=True)
        nsg, cg = g.window_stats(counts=True)
        assert ns1 == nsg == 3 and np.array_equal(c1, cg) and np.array_equal(cg, want[W])
        assert np.array_equal(cg.sum(axis=0), tot.sum(axis=0))
        for a, b in zip(one.window_stats()[1:], g.window_stats()[1:]):
            assert np.array_equal(a, b)
        # every context returns zero outside the windows it holds, and holds the windows its owned sites meet
        for j, s in enumerate(g.subs):
            Wc, w0, nw = s.window_stats_layout()
            lo, hi = max(g.a[j], 1), min(g.b[j] - 1, n - 2)
            assert (Wc, w0, nw) == (W, lo // W, hi // W - lo // W + 1)
            _, part = s.window_counts()
            assert not part[:w0].any() and not part[w0 + nw:].any() and part[w0:w0 + nw, :, 8:].any()
        one.close()
        g.close()


@pytest.mark.parametrize("k", [1, 3])
def test_sharded_sampler_reads_out_its_engine(k):
    """ShardedSampler on one rank over the engines of the product -- a DeviceSampler, and a LocalGroup of three
    contexts -- gives the oracle's windows as integers and as J and D"""
    n, W = 3100, 100
    model, tree, fp = simulate("tree", n, seed=4)
    cap = _cap(fp)
    want, tot, o = _oracle_run(tree, model, fp, cap, (W,), seed=99, base=7)
    ss = ShardedSampler(NullComm(), 0, (lambda dev: LocalGroup(dev, 3, 10)) if k > 1 else None)
    ss.setup(model, tree, fp, [0, n], capacity=cap, sweeps_per_refresh=10)
    assert len(getattr(ss.dev, "subs", [ss.dev])) == k
    ss.enable_window_stats(W)
    ss.reset()
    ss.run_mcmc(BURN_IN, BATCH, 99, sweep_base=7)
    ns, got = ss.window_stats(counts=True)
    assert ns == BATCH and np.array_equal(got, want[W])
    ns, J, D = ss.window_stats()
    Jw, Dw = wstat_ref.to_stats(want[W], wstat_ref.scales(o), BATCH)
    assert ns == BATCH and np.array_equal(J, Jw) and np.array_equal(D, Dw)
    assert np.array_equal(np.ldexp(1.0, ss.window_stats_scale_exps()), wstat_ref.scales(o)[1:])
    ss.reset_window_stats()
    assert not ss.window_stats(counts=True)[1].any()
    ss.dev.close()


def test_lifecycle():
    n, W = 1500, 100
    model, tree, fp = simulate("tree", n, seed=6)
    cap, B = _cap(fp), tree.n_nodes - 1
    d = _dev(tree, model, fp, cap)
    # off: nothing to read, nothing to add to
    for call in (d.window_stats, d.accumulate_window_stats, d.reset_window_stats):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE
    assert d.window_stats_samples() == 0 and d.window_stats_layout() == (0, 0, 0)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=21)
    o.reset()
    d.enable_window_stats(W)
    # before the first sample a new site range lays the accumulator out again
    d.set_update_range(250, 1000)
    assert d.window_stats_layout() == (W, 2, 9)
    d.set_update_range(1, n - 2)
    assert d.window_stats_layout() == (W, 0, 15)
    d.reset()
    # manual sweeps, a sample when the caller likes; kept over reset() and set_model()
    want = np.zeros((15, B, 16), np.int64)
    for w in range(3):
        assert d.sweep(1, 21, sweep_base=w) == o.sweep(w)
        d.accumulate_window_stats()
        want += wstat_ref.rows(o, W, n)
        if w == 0:
            d.reset()
        if w == 1:
            d.set_model(model)
            d.reset()
    ns, got = d.window_stats(counts=True)
    assert ns == 3 and np.array_equal(got, want)
    # afterwards a changed site range is an error
    d.set_update_range(250, 1000)
    d.reset()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(0, 1, 21, sweep_base=3)
    assert e.value.code == EPV_ERR_STATE and "sites of this context changed" in str(e.value)
    d.set_update_range(1, n - 2)
    d.reset()
    # new branch lengths change k_b: the integers held and the integers to come would not mean the same
    new = tree.branches * 4.0
    d.scale_jump_times(new)
    o.scale_jump_times(new)
    paths = d.paths()
    with pytest.raises(EpvError) as e:
        d.accumulate_window_stats()
    assert e.value.code == EPV_ERR_STATE and "epv_reset_window_stats" in str(e.value)
    d.reset()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(0, 1, 21, sweep_base=3)
    assert e.value.code == EPV_ERR_STATE
    assert orc.paths_equal(d.paths(), paths)                       # refused before any sweep
    assert np.array_equal(d.window_stats(counts=True)[1], want)    # and nothing was added
    d.reset_window_stats()
    assert d.window_stats_samples() == 0 and not d.window_stats(counts=True)[1].any()
    d.accumulate_window_stats()
    ns, got = d.window_stats(counts=True)
    assert ns == 1 and np.array_equal(got, wstat_ref.rows(o, W, n))
    d.close()


def test_sample_cap():
    """(samples + batch) * min(W, owned sites) * max_b q_b >= 2^63 is refused, q_b = rint(T_b 2^k_b) + 3072"""
    n, W = 1500, 100
    model, tree, fp = simulate("tree", n, seed=6)
    d = _dev(tree, model, fp, _cap(fp))
    d.enable_window_stats(W)
    d.reset()
    o = orc.Oracle(tree, model, fp, "B", cap=_cap(fp), seed=5)
    sc = wstat_ref.scales(o)
    q = max(int(round(float(tree.branches[b]) * float(sc[b]))) + 3072 for b in range(1, tree.n_nodes))
    most = (2 ** 63 - 1) // (W * q)
    assert (most + 1) * W * q >= 2 ** 63 > most * W * q
    d._ck(d.L.epv_window_stats_set_samples(d.h, most - 1))
    d.run_mcmc(0, 1, 5)                           # the last sample that fits
    assert d.window_stats_samples() == most
    paths, held = d.paths(), d.window_stats(counts=True)[1]
    for call in (d.accumulate_window_stats, lambda: d.run_mcmc(0, 1, 5, sweep_base=1)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE
        assert "windows of %d sites" % W in str(e.value) and "at most %d samples" % most in str(e.value)
    assert orc.paths_equal(d.paths(), paths)      # a refused run has not swept
    assert np.array_equal(d.window_stats(counts=True)[1], held)
    # a batch that would pass the bound is refused as a whole, before its first sweep
    d._ck(d.L.epv_window_stats_set_samples(d.h, most - 2))
    with pytest.raises(EpvError) as e:
        d.run_mcmc(0, 3, 5, sweep_base=1)
    assert e.value.code == EPV_ERR_STATE and orc.paths_equal(d.paths(), paths)
    # W = 0 frees the accumulator
    d.enable_window_stats(0)
    assert d.window_stats_layout() == (0, 0, 0) and d.window_stats_samples() == 0
    with pytest.raises(EpvError):
        d.window_stats()
    d.run_mcmc(0, 1, 5, sweep_base=1)             # off costs nothing and counts nothing
    assert d.window_stats_samples() == 0
    d.close()


def test_counts_survive_capacity_growth():
    """a deliberately tiny capacity: overflows widen the jump slots between batch sweeps (auto_grow); the sums keep
    accumulating and match the oracle run at the same capacities"""
    n, W = 2000, 64
    model, tree, fp = simulate("pair", n, seed=8)
    cap = int(fp.counts().max())
    d = _dev(tree, model, fp, cap)
    d.auto_grow = True
    d.enable_window_stats(W)
    d.reset()
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=4)
    o.reset()
    want = np.zeros((wstat_ref.n_windows(n, W), 1, 16), np.int64)
    for w in range(4):
        d.run_mcmc(0, 1, 4, sweep_base=w)
        o.sweep(w)
        want += wstat_ref.rows(o, W, n)
        o.set_rung("B", d.capacity())
    assert d.capacity() > cap and d.capacity_events
    ns, got = d.window_stats(counts=True)
    assert ns == 4 and np.array_equal(got, want)
    d.close()
