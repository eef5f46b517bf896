"""Epoch statistics on the device (epv_set_epoch_stats): J and D per branch and epoch of the branch, added over
the batch sweeps of run_mcmc as exact integers.

After every batch sweep -- identity A: summed over the epochs the closed result equals, per branch and context,
the sum of what run_mcmc_counts returned so far; identity B: every (branch, epoch, context) cell equals the
yardstick (tests/epoch_ref.py: a plain-Python walk of rung B's paths of the same Philox sweeps); identity C: at
P = 1 the result is the whole-genome counts.  All bit for bit (Python ints), on the fused and the unfused phase,
at block and tile edges, on a tree whose 30 branches each get their own blocks, on dense histories where every
triple is walked from the ring, for three contexts, and over the life cycle.  Identity D (no dependence on how
the genome is cut) is the LocalGroup and ShardedSampler cases.  Counting changes neither J, D, the accept count,
the paths, tri_llh nor the plan.

Every case -- the LocalGroup, ShardedSampler, lifecycle and capacity-growth cases included -- is asserted to be a
real one on the oracle's own paths: for every P >= 3 some branch holds jumps in
two or more epochs and some interval meets three or more epochs (at P = 2 an interval meets both; at P = 1
neither can be), and some triple's clock ends off fixT_b, so the open-ended last epoch is exercised."""
import numpy as np
import pytest

import dense_cases as dc
import epoch_ref
import orc
import wstat_ref
from common import simulate
from epievo_amd.parallel import LocalGroup, NullComm, ShardedSampler
from epievo_amd.sampler import EPOCH_MAX_P, EPV_ERR_ARG, EPV_ERR_STATE, DeviceSampler, EpvError

pytestmark = pytest.mark.gpu

NO_FUSED = {"EPV_FUSED_PHASE": "0"}
PS = (1, 2, 7, 64, EPOCH_MAX_P)
SEED, BASE, BURN_IN, BATCH = 77, 5, 1, 3


def _dev(tree, model, fp, cap):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    return d


def _cap(fp):
    return int(max(16, 2 * fp.counts().max() + 8))


def _same(got, want):
    return got.shape == want.shape and all(int(a) == int(b) for a, b in zip(got.reshape(-1), want.reshape(-1)))


def _check_run(tree, model, fp, cap, o, seed, batch, Ps=PS, mode=None, base=BASE):
    """the main case: an `off` context and one context per P, run sweep by sweep next to the oracle"""
    B = tree.n_nodes - 1
    y = epoch_ref.Yard(o, tree, Ps)
    for w in range(BURN_IN):
        o.sweep(base + w)
    tot = np.zeros((batch, B, 16), np.int64)
    for w in range(batch):
        o.sweep(base + BURN_IN + w)
        y.add()
        tot[w] = wstat_ref.total(o, fp.n_sites)
    y.assert_not_vacuous()
    off = _dev(tree, model, fp, cap)
    if mode is not None:
        assert off.phase_mode() == mode
    off.reset()
    ons = []
    for P in Ps:
        on = _dev(tree, model, fp, cap)
        assert on.phase_plan() == off.phase_plan()
        on.enable_epoch_stats(P)
        assert on.phase_plan() == off.phase_plan() and on.epoch_stats_samples() == 0
        Pl, k, fixT = on.epoch_stats_layout()
        assert Pl == P and [int(f) for f in fixT] == y.fixT and np.array_equal(np.ldexp(1.0, k), y.sc[1:])
        on.reset()
        ons.append(on)
    for w in range(batch):
        burn, sb = (BURN_IN, base) if w == 0 else (0, base + BURN_IN + w)
        c0, a0 = off.run_mcmc_counts(burn, 1, seed, sweep_base=sb)
        assert np.array_equal(c0.reshape(B, 16), tot[w])
        J0, D0 = off.counts_to_stats(c0, 1)
        sofar = tot[:w + 1].sum(axis=0)
        for i, (P, on) in enumerate(zip(Ps, ons)):
            # nothing else changes (the statistics of the run through either of the two statistics kernels)
            if (i + w) % 2 == 0:
                J1, D1, a1 = on.run_mcmc(burn, 1, seed, sweep_base=sb)
            else:
                c1, a1 = on.run_mcmc_counts(burn, 1, seed, sweep_base=sb)
                assert np.array_equal(c1, c0)
                J1, D1 = on.counts_to_stats(c1, 1)
            assert a1 == a0 and np.array_equal(J1, J0) and np.array_equal(D1, D0)
            assert orc.paths_equal(on.paths(), off.paths()) and orc.paths_equal(on.paths(), o.paths()) \
                if w == batch - 1 else True
            assert np.array_equal(on.tri_llh(), off.tri_llh())
            assert on.phase_plan() == off.phase_plan() and on.phase_mode() == off.phase_mode()
            ns, J, D = on.epoch_stats(counts=True)
            assert ns == w + 1 and J.dtype == np.int64 and J.shape == D.shape == (B, P, 8)
            wantJ, wantD = y.after[w][P]
            assert _same(J, wantJ) and _same(D, wantD), (P, w)                              # identity B
            assert np.array_equal(J.sum(axis=1), sofar[:, :8]), (P, w)                      # identity A
            assert _same(D.sum(axis=1), sofar[:, 8:].astype(object)), (P, w)
            if P == 1:                                                                      # identity C
                assert np.array_equal(J[:, 0], sofar[:, :8]) and _same(D[:, 0], sofar[:, 8:].astype(object))
    for P, on in zip(Ps, ons):
        ns, J, D = on.epoch_stats()
        Jw, Dw = epoch_ref.to_stats(y.J[P], y.D[P], y.sc, batch)
        assert ns == batch and np.array_equal(J, Jw) and np.array_equal(D, Dw)
        on.close()
    off.close()


# (EPV_PHASE_*: 1 = V2 kernels, 3 = fused phase, 4 = V3 large-tree kernels)
@pytest.mark.parametrize("cfg,n,sim_seed,env,mode,batch", [
    ("tree", 3, 10, {}, None, 4),              # one interior site
    ("tree", 65, 6, {}, None, BATCH),          # an edge column on either side of the one tile
    ("tree", 257, 6, {}, None, BATCH),         # two blocks along the sites, the second of one site
    ("tree", 258, 6, {}, None, BATCH),
    ("tree", 700, 6, {}, 3, BATCH),
    ("tree", 700, 6, NO_FUSED, 1, BATCH),
    ("bal16", 300, 6, {}, 4, BATCH)])          # B = 30: thirty block rows, two tiles each
def test_epochs_match_yardstick_and_change_nothing(monkeypatch, cfg, n, sim_seed, env, mode, batch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # read when a context is created
    model, tree, fp = simulate(cfg, n, seed=sim_seed)
    cap = _cap(fp)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=SEED)
    o.reset()
    _check_run(tree, model, fp, cap, o, SEED, batch, mode=mode)


@pytest.mark.parametrize("name,n", [("weak-pair4", 600), ("flat-bal16x300", 200)])
def test_dense_histories(name, n):
    """every interior (site, branch) triple of the input has a jump on one of its three paths: none takes the
    no-jump histogram, all are queued in the ring and walked.  On weak-pair4 a block queues 256 triples per tile
    and walks them at once, the third tile's 86 at the end"""
    model, tree, fp = dc.workload(name, n)
    cap, B = dc.capacity(name, fp), tree.n_nodes - 1
    assert dc.density(fp)["mean"] >= 2.0 and fp.n_sites == n <= 600
    nj = fp.counts().reshape(B, n)
    assert (nj[:, :-2] + nj[:, 1:-1] + nj[:, 2:] > 0).all()
    o = dc.oracle(name, cap, n=n)
    _check_run(tree, model, fp, cap, o, dc.ORACLE_SEED, 2)


@pytest.mark.parametrize("n,spr,k", [(1000, 60, None), (3100, 10, 3)])
def test_local_group_equals_single_context(n, spr, k):
    """identity D: a LocalGroup of three -- ("tree", 1000) is too short to be cut, ("tree", 3100) with the narrowest
    halos gives three contexts cut at 1024 and 2048 -- adds its contexts' raw parts to the one-context result"""
    model, tree, fp = simulate("tree", n, seed=4)
    cap, B = _cap(fp), tree.n_nodes - 1
    Ps = (7, EPOCH_MAX_P)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=99)
    o.reset()
    y = epoch_ref.Yard(o, tree, Ps)
    o.sweep(7)
    for w in range(3):
        o.sweep(8 + w)
        y.add()
    y.assert_not_vacuous()
    for P in Ps:
        one = _dev(tree, model, fp, cap)
        g = LocalGroup(0, 3, sweeps_per_refresh=spr)
        g.set_tree(tree)
        g.set_model(model)
        g.upload_paths(fp, cap)
        if k is not None:
            assert len(g.subs) == k
        one.enable_epoch_stats(P)
        g.enable_epoch_stats(P)
        res = []
        for s in (one, g):
            s.reset()
            res.append(s.run_mcmc_counts(1, 3, 99, sweep_base=7))
        assert res[0][1] == res[1][1] and np.array_equal(res[0][0], res[1][0])
        ns1, J1, D1 = one.epoch_stats(counts=True)
        nsg, Jg, Dg = g.epoch_stats(counts=True)
        assert ns1 == nsg == 3 and np.array_equal(J1, Jg) and _same(D1, Dg)
        assert _same(Jg, y.J[P]) and _same(Dg, y.D[P]) and orc.paths_equal(g.paths(), o.paths())
        tot = res[0][0].reshape(3, B, 16).sum(axis=0)
        assert np.array_equal(Jg.sum(axis=1), tot[:, :8]) and _same(Dg.sum(axis=1), tot[:, 8:].astype(object))
        for a, b in zip(one.epoch_stats()[1:], g.epoch_stats()[1:]):
            assert np.array_equal(a, b)
        if k is not None:        # every context holds a part, and the parts differ from the whole
            raws = [s.epoch_raw()[1] for s in g.subs]
            assert all(r[..., 8:24].any() for r in raws)
            for a, b in zip(epoch_ref.parts_of(g.epoch_raw()[1]), epoch_ref.parts_of(one.epoch_raw()[1])):
                assert (a == b).all()
        one.close()
        g.close()


@pytest.mark.parametrize("k", [1, 3])
def test_sharded_sampler_reads_out_its_engine(k):
    """ShardedSampler on one rank over the engines of the product -- a DeviceSampler, and a LocalGroup of three
    contexts -- gives the yardstick's epochs as integers and as J and D"""
    n, P = 3100, 7
    model, tree, fp = simulate("tree", n, seed=4)
    cap = _cap(fp)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=99)
    o.reset()
    y = epoch_ref.Yard(o, tree, (P,))
    o.sweep(7)
    for w in range(2):
        o.sweep(8 + w)
        y.add()
    y.assert_not_vacuous()
    ss = ShardedSampler(NullComm(), 0, (lambda dev: LocalGroup(dev, 3, 10)) if k > 1 else None)
    ss.setup(model, tree, fp, [0, n], capacity=cap, sweeps_per_refresh=10)
    assert len(getattr(ss.dev, "subs", [ss.dev])) == k
    ss.enable_epoch_stats(P)
    ss.reset()
    ss.run_mcmc(1, 2, 99, sweep_base=7)
    ns, J, D = ss.epoch_stats(counts=True)
    assert ns == ss.epoch_stats_samples() == 2 and _same(J, y.J[P]) and _same(D, y.D[P])
    ns, Jf, Df = ss.epoch_stats()
    Jw, Dw = epoch_ref.to_stats(y.J[P], y.D[P], y.sc, 2)
    assert ns == 2 and np.array_equal(Jf, Jw) and np.array_equal(Df, Dw)
    ss.reset_epoch_stats()
    ns, J, D = ss.epoch_stats(counts=True)
    assert ns == 0 and not J.any() and not D.any()
    ss.dev.close()


def test_lifecycle():
    n, P = 1500, 7
    model, tree, fp = simulate("tree", n, seed=6)
    cap, B = _cap(fp), tree.n_nodes - 1
    d = _dev(tree, model, fp, cap)
    # off: nothing to read, nothing to add to
    for call in (d.epoch_stats, d.accumulate_epoch_stats, d.reset_epoch_stats):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE
    assert d.epoch_stats_samples() == 0 and d.epoch_stats_layout()[0] == 0
    with pytest.raises(ValueError):
        d.enable_epoch_stats(EPOCH_MAX_P + 1)
    assert d.L.epv_set_epoch_stats(d.h, EPOCH_MAX_P + 1) == EPV_ERR_ARG
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=21)
    o.reset()
    y = epoch_ref.Yard(o, tree, (P,))
    d.enable_epoch_stats(P)
    d.reset()
    # manual sweeps, a sample when the caller likes; kept over reset(), set_model() and a narrower update range
    for w in range(3):
        assert d.sweep(1, 21, sweep_base=w) == o.sweep(w)
        d.accumulate_epoch_stats()
        y.add()
        if w == 0:
            d.reset()
        if w == 1:
            d.set_model(model)
            d.reset()
    y.assert_not_vacuous()
    ns, J, D = d.epoch_stats(counts=True)
    assert ns == 3 and _same(J, y.J[P]) and _same(D, y.D[P])
    # new branch lengths change k_b: the integers held and the integers to come would not mean the same
    new = tree.branches * 4.0
    d.scale_jump_times(new)
    o.scale_jump_times(new)
    paths = d.paths()
    with pytest.raises(EpvError) as e:
        d.accumulate_epoch_stats()
    assert e.value.code == EPV_ERR_STATE and "epv_reset_epoch_stats" in str(e.value)
    d.reset()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(0, 1, 21, sweep_base=3)
    assert e.value.code == EPV_ERR_STATE
    assert orc.paths_equal(d.paths(), paths)                       # refused before any sweep
    ns, J2, D2 = d.epoch_stats(counts=True)                        # and nothing was added; the layout is the samples'
    assert ns == 3 and _same(J2, y.J[P]) and _same(D2, y.D[P])
    assert [int(f) for f in d.epoch_stats_layout()[2]] == y.fixT
    d.reset_epoch_stats()
    ns, J, D = d.epoch_stats(counts=True)
    assert ns == 0 and not J.any() and not D.any()
    d.accumulate_epoch_stats()
    tree4 = type("T", (), {"branches": new, "n_nodes": tree.n_nodes})
    y4 = epoch_ref.Yard(o, tree4, (P,))
    y4.add()
    y4.assert_not_vacuous()
    assert y4.fixT != y.fixT or not np.array_equal(y4.sc, y.sc)
    ns, J, D = d.epoch_stats(counts=True)
    assert ns == 1 and _same(J, y4.J[P]) and _same(D, y4.D[P])
    # P = 0 frees the accumulator; off costs nothing and counts nothing
    d.enable_epoch_stats(0)
    assert d.epoch_stats_layout()[0] == 0 and d.epoch_stats_samples() == 0
    d.reset()
    d.run_mcmc(0, 1, 5, sweep_base=1)
    assert d.epoch_stats_samples() == 0
    d.close()


def test_sample_cap():
    """(samples + batch) * blocks along the sites >= 2^32 is refused: every 64-bit word of the accumulator takes
    at most one addend below 2^32 per block and sample.  1500 sites and 4 branches: six one-tile blocks"""
    n, P = 1500, 2
    model, tree, fp = simulate("tree", n, seed=6)
    d = _dev(tree, model, fp, _cap(fp))
    d.enable_epoch_stats(P)
    d.reset()
    blocks = (n - 2 + 255) // 256
    most = (2 ** 32 - 1) // blocks
    assert (most + 1) * blocks >= 2 ** 32 > most * blocks
    d._ck(d.L.epv_epoch_stats_set_samples(d.h, most - 1))
    d.run_mcmc(0, 1, 5)                           # the last sample that fits
    assert d.epoch_stats_samples() == most
    paths, held = d.paths(), d.epoch_raw()[1]
    for call in (d.accumulate_epoch_stats, lambda: d.run_mcmc(0, 1, 5, sweep_base=1)):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE
        assert "%d blocks" % blocks in str(e.value) and "at most %d samples" % most in str(e.value)
    assert orc.paths_equal(d.paths(), paths)      # a refused run has not swept
    assert np.array_equal(d.epoch_raw()[1], held)
    # a batch that would pass the bound is refused as a whole, before its first sweep
    d._ck(d.L.epv_epoch_stats_set_samples(d.h, most - 2))
    with pytest.raises(EpvError) as e:
        d.run_mcmc(0, 3, 5, sweep_base=1)
    assert e.value.code == EPV_ERR_STATE and orc.paths_equal(d.paths(), paths)
    d.close()


def test_counts_survive_capacity_growth():
    """a deliberately tiny capacity: overflows widen the jump slots between batch sweeps (auto_grow); the sums keep
    accumulating and match the oracle run at the same capacities"""
    n, P = 2000, 64
    model, tree, fp = simulate("pair", n, seed=8)
    cap = int(fp.counts().max())
    d = _dev(tree, model, fp, cap)
    d.auto_grow = True
    d.enable_epoch_stats(P)
    d.reset()
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=4)
    o.reset()
    y = epoch_ref.Yard(o, tree, (P,))
    for w in range(4):
        d.run_mcmc(0, 1, 4, sweep_base=w)
        o.sweep(w)
        y.add()
        o.set_rung("B", d.capacity())
    y.assert_not_vacuous()
    assert d.capacity() > cap and d.capacity_events
    ns, J, D = d.epoch_stats(counts=True)
    assert ns == 4 and _same(J, y.J[P]) and _same(D, y.D[P])
    d.close()
