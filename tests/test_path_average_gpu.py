"""The average history of the sampled paths, counted on the device during run_mcmc
(epv_set_path_average): the counts equal, exactly, those numpy computes from the CPU oracle's paths
after every batch sweep (rung B, the same Philox sweeps), on every kernel path, for one context and a
LocalGroup of three; averaging does not change J, D, the accept count or the paths."""
import numpy as np
import pytest

import orc
import pavg_ref
from common import simulate
from epievo_amd.parallel import LocalGroup
from epievo_amd.sampler import DeviceSampler, EpvError

pytestmark = pytest.mark.gpu


def _dev(tree, model, fp, cap):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    return d


def _oracle_counts(tree, model, fp, cap, seed, burn_in, batch, base, P):
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    o.reset()
    for w in range(burn_in):
        o.sweep(base + w)
    cnt = np.zeros((tree.n_nodes - 1, fp.n_sites, P), np.uint32)
    for w in range(batch):
        o.sweep(base + burn_in + w)
        cnt += pavg_ref.counts(o.paths(), tree.branches, P)
    return cnt, o.paths()


# (EPV_PHASE_*: 1 = V2 kernels, 2 = V2 with segment-parallel jumps, 3 = fused phase, 4 = V3 large-tree kernels)
NO_FUSED = {"EPV_FUSED_PHASE": "0"}
SEG = {"EPV_FUSED_PHASE": "0", "EPV_SEG_JUMPS": "1"}
NO_SEG = {"EPV_FUSED_PHASE": "0", "EPV_SEG_JUMPS": "0"}


@pytest.mark.parametrize("cfg,n,P,burn_in,batch,env,mode", [
    ("tree", 40000, 100, 1, 3, {}, 3), ("tree", 3001, 7, 2, 2, NO_FUSED, 1),
    ("bal16", 3000, 2, 1, 2, {}, 4), ("bal16", 2500, 100, 0, 2, {}, 4),
    ("pair", 4000, 7, 1, 3, SEG, 2), ("pair", 3000, 100, 0, 2, NO_SEG, 1)])
def test_counts_match_oracle_and_change_nothing(monkeypatch, cfg, n, P, burn_in, batch, env, mode):
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # read when a context is created
    model, tree, fp = simulate(cfg, n, seed=6)
    cap = int(max(16, 2 * fp.counts().max() + 8))
    on, off = _dev(tree, model, fp, cap), _dev(tree, model, fp, cap)
    assert on.phase_mode() == off.phase_mode() == mode
    on.enable_path_average(P)
    on.reset()
    off.reset()
    J1, D1, a1 = on.run_mcmc(burn_in, batch, 77, sweep_base=5)
    J0, D0, a0 = off.run_mcmc(burn_in, batch, 77, sweep_base=5)
    assert a1 == a0 and np.array_equal(J1, J0) and np.array_equal(D1, D0)
    assert orc.paths_equal(on.paths(), off.paths())
    ns, cnt = on.path_average(counts=True)
    assert ns == batch and cnt.shape == (tree.n_nodes - 1, n, P)     # sites 0 and n - 1 included
    want, opaths = _oracle_counts(tree, model, fp, cap, 77, burn_in, batch, 5, P)
    assert orc.paths_equal(on.paths(), opaths)
    assert np.array_equal(cnt, want)
    ns2, avg = on.path_average()
    assert ns2 == batch and np.array_equal(avg, want / float(batch))
    # a read-out in the middle of a run leaves the counts alone; later sweeps add to them
    J2, D2, _ = on.run_mcmc(0, 1, 77, sweep_base=5 + burn_in + batch)
    ns3, cnt3 = on.path_average(counts=True)
    assert ns3 == batch + 1
    assert np.array_equal(cnt3, cnt + pavg_ref.counts(on.paths(), tree.branches, P))
    on.reset_path_average()
    assert on.path_average(counts=True)[0] == 0 and not on.path_average(counts=True)[1].any()
    on.close()
    off.close()


def test_counts_survive_capacity_growth():
    """a deliberately tiny capacity: overflows widen the jump slots between batch sweeps (auto_grow);
    the counts keep accumulating and match the oracle run at the same capacities"""
    model, tree, fp = simulate("pair", 2000, seed=8)
    cap, P = int(fp.counts().max()), 13
    d = _dev(tree, model, fp, cap)
    d.auto_grow = True
    d.enable_path_average(P)
    d.reset()
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=4)
    o.reset()
    want = np.zeros((1, 2000, P), np.uint32)
    for w in range(4):
        d.run_mcmc(0, 1, 4, sweep_base=w)
        o.sweep(w)
        want += pavg_ref.counts(o.paths(), tree.branches, P)
        o.set_rung("B", d.capacity())
    assert d.capacity() > cap and d.capacity_events
    ns, cnt = d.path_average(counts=True)
    assert ns == 4 and np.array_equal(cnt, want)


@pytest.mark.parametrize("cfg,n", [("tree", 20011), ("bal16", 9000)])
def test_local_group_counts_equal_single_context(cfg, n):
    model, tree, fp = simulate(cfg, n, seed=4)
    cap = int(max(16, 2 * fp.counts().max() + 8))
    P = 11
    d = _dev(tree, model, fp, cap)
    g = LocalGroup(0, 3)
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    assert len(g.subs) == 3
    d.enable_path_average(P)
    g.enable_path_average(P)
    d.reset()
    g.reset()
    Jd, Dd, nd = d.run_mcmc(1, 3, 99, sweep_base=7)
    Jg, Dg, ng = g.run_mcmc(1, 3, 99, sweep_base=7)
    assert nd == ng and np.array_equal(Jd, Jg) and np.array_equal(Dd, Dg)
    nsd, cd = d.path_average(counts=True)
    nsg, cg = g.path_average(counts=True)
    assert nsd == nsg == 3 and cg.shape == (tree.n_nodes - 1, n, P)
    assert np.array_equal(cd, cg)
    want, _ = _oracle_counts(tree, model, fp, cap, 99, 1, 3, 7, P)
    assert np.array_equal(cg, want)
    g.close()
    d.close()


def test_accumulate_after_manual_sweeps():
    """the epievo_sim_pairwise pattern: the caller drives the sweeps and takes a sample when it likes"""
    model, tree, fp = simulate("tree", 5000, seed=3)
    cap = int(max(16, 2 * fp.counts().max() + 8))
    P = 50
    d = _dev(tree, model, fp, cap)
    d.enable_path_average(P)
    d.reset()
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=21)
    o.reset()
    want = np.zeros((tree.n_nodes - 1, 5000, P), np.uint32)
    for w in range(3):
        assert d.sweep(1, 21, sweep_base=w) == o.sweep(w)
        d.accumulate_path_average()
        want += pavg_ref.counts(o.paths(), tree.branches, P)
    ns, cnt = d.path_average(counts=True)
    assert ns == 3 and np.array_equal(cnt, want)
    # a changed branch length refreshes the grid for the next samples
    nb = tree.branches * 1.25
    d.scale_jump_times(nb)
    d.accumulate_path_average()
    want += pavg_ref.counts(d.paths(), nb, P)
    assert np.array_equal(d.path_average(counts=True)[1], want)


def test_too_many_points_fail_cleanly():
    model, tree, fp = simulate("tree", 10000, seed=1)
    d = _dev(tree, model, fp, 32)
    with pytest.raises(EpvError) as e:
        d.enable_path_average(2 ** 31)
    assert "GB of device memory" in str(e.value)
    with pytest.raises(EpvError):
        d.enable_path_average(1)
    # the context is still usable, averaging off
    d.reset()
    d.run_mcmc(0, 1, 5)
    assert d.path_average_samples() == 0
