"""The statistics pass of the sharded path: epv_run_mcmc_counts and epv_suffstat_wave_kernel against rung B.

epv_run_mcmc_counts has one statistics launch, epv_suffstat_wave_kernel (one wave per 64 sites, rows folded
modulo EPV_STATW_ROWS, one reduction stage, one wait for everything the host reads); DeviceSampler.run_mcmc_counts
calls it on one context, LocalGroup on two or three.  The library has no call that names the statistics kernel of
a run the way epv_phase_plan names a colour phase's, so the path is fixed by the entry point, and the colour
phase's plan is asserted to be the same before and after.  Every case runs two burn-in sweeps first, so that sel
is mixed 0 / 1 when the batch sweeps are counted, and compares the integer totals of every batch sweep's J and
fixed-point D, J and D as doubles and the accept count bit for bit with the oracle's parallel rung.

  shapes   n = 3, 64, 65, 66, 257, 700 sites on pair (1 branch), tree (4) and bal8 (14: a second blockIdx.y group)
  cuts     two contexts cut by hand at a site that is no multiple of 64, with odd halos: owned ranges begin and
           end inside a 64-site wave and inside a 256-site block
  dense    histories of dense_cases.py: a wave queues more than 64 slow items (the ring is flushed inside the
           branch loop) and columns hold three and more jumps (the merge fetches later jumps)
  groups   two and three contexts of a LocalGroup return the integers of one context

Without a GPU the oracle's side of every case runs here: its J and D after the burn-in sweeps against the
plain-Python yardstick of dense_cases.py (J exactly, D within the fixed-point bound)."""
import numpy as np
import pytest

import dense_cases as dc
import orc
from common import config, ref_test_model
from epievo_amd import host

BURN_IN, BATCH, SEED, BASE = 2, 3, 29, 4
TREES = ("pair", "tree", "bal8")
SIZES = (3, 64, 65, 66, 257, 700)
# (n, cut, halo): context A holds [0, cut + halo) and owns [0, cut), B holds [cut - halo, n) and owns [cut, n);
# 15 colour phases use up 30 halo columns
CUTS = ((257, 129, 37), (700, 300, 37), (700, 449, 33))
DENSE = ("weak-tree40", "weak-pair25", "weak-bal8x100")
GROUP_N = 3300          # the least a LocalGroup of three cuts into three: 3 x (2 x 256 halo + 2 x 256) = 3072

_inputs = {}


def small(tree_name, n):
    key = (tree_name, n)
    if key not in _inputs:
        model, tree = ref_test_model(), config(tree_name)
        fp = host.simulate(model, tree, n, 6)
        _inputs[key] = (model, tree, fp, int(max(16, 2 * fp.counts().max() + 8)))
    return _inputs[key]


def oracle_counts(model, tree, fp, cap, seed=SEED, prepared=None):
    """rung B: (J, D, accepted) of run_mcmc(BURN_IN, BATCH)"""
    o = prepared or orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    if prepared is None:
        o.reset()
    J, D, nacc, _ = o.run_mcmc(BURN_IN, BATCH, sweep_base=BASE)
    o.close()
    return J, D, nacc


def device(model, tree, fp, cap, offset=0, n_global=None, halo=None):
    from epievo_amd.sampler import DeviceSampler
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap, offset, n_global)
    if halo:
        d.set_halo(*halo)
    d.reset()
    return d


def run_counts(d, seed=SEED):
    plan = d.phase_plan()
    counts, nacc = d.run_mcmc_counts(BURN_IN, BATCH, seed, sweep_base=BASE)
    assert d.phase_plan() == plan
    assert counts.shape == (BATCH, 16 * d.B)
    return counts, nacc


def check(d, counts, nacc, expect):
    Jo, Do, no = expect
    J, D = d.counts_to_stats(counts, BATCH)
    print("accepted %d (oracle %d), sum J %.0f (oracle %.0f)" % (nacc, no, J.sum() * BATCH, Jo.sum() * BATCH))
    assert nacc == no
    assert np.array_equal(J, Jo)
    assert np.array_equal(D.view(np.uint64), Do.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_one_context_matches_rung_b(n):
    for name in TREES:
        model, tree, fp, cap = small(name, n)
        d = device(model, tree, fp, cap)
        counts, nacc = run_counts(d)
        check(d, counts, nacc, oracle_counts(model, tree, fp, cap))
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,cut,halo", CUTS)
def test_owned_ranges_cut_inside_waves_and_blocks(n, cut, halo):
    for name in ("tree", "bal8"):
        model, tree, fp, cap = small(name, n)
        a = device(model, tree, fp.slice_sites(0, cut + halo), cap, 0, n, (0, halo))
        b = device(model, tree, fp.slice_sites(cut - halo, n), cap, cut - halo, n, (halo, 0))
        ca, na = run_counts(a)
        cb, nb = run_counts(b)
        assert ca.any() and cb.any()
        check(a, ca + cb, na + nb, oracle_counts(model, tree, fp, cap))
        a.close()
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", DENSE)
def test_dense_histories_match_rung_b(name):
    model, tree, fp = dc.workload(name)
    cap = dc.capacity(name, fp)
    d = device(model, tree, fp, cap)
    counts, nacc = run_counts(d, dc.ORACLE_SEED)
    check(d, counts, nacc, oracle_counts(model, tree, fp, cap, prepared=dc.oracle(name, cap)))
    d.close()


@pytest.mark.gpu
def test_two_and_three_contexts_return_the_same_integers():
    from epievo_amd.parallel import LocalGroup
    model, tree, fp, cap = small("tree", GROUP_N)
    one = device(model, tree, fp, cap)
    c1, n1 = run_counts(one)
    check(one, c1, n1, oracle_counts(model, tree, fp, cap))
    for k in (2, 3):
        g = LocalGroup(0, k, sweeps_per_refresh=BURN_IN + BATCH)
        g.set_tree(tree)
        g.set_model(model)
        g.upload_paths(fp, cap)
        g.reset()
        assert len(g.subs) == k
        ck, nk = g.run_mcmc_counts(BURN_IN, BATCH, SEED, sweep_base=BASE)
        assert nk == n1 and np.array_equal(ck, c1)
        g.close()
    one.close()


# ---- without a GPU: the oracle's side of the same cases
def _oracle_against_yardstick(model, tree, fp, cap, o=None, seed=SEED):
    o = o or orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    o.reset()
    for w in range(BURN_IN):
        o.sweep(BASE + w)
    J, D = o.suffstats()
    Jy, Dy, n_int = dc.yardstick(o.paths(), tree.branches)
    assert np.array_equal(J.reshape(-1, 8), Jy)
    assert np.all(np.abs(D.reshape(-1, 8) - Dy) <= dc.dwell_bound(n_int, Dy, dc.stat_scales(o)))
    Jb, Db, nacc, _ = o.run_mcmc(0, BATCH, sweep_base=BASE + BURN_IN)
    assert np.all(Jb >= 0) and np.all(Db >= 0) and 0 <= nacc <= BATCH * max(fp.n_sites - 2, 0)
    # every site spends the whole branch in some context: the D of a branch add up to (n - 2) T
    T = np.asarray(tree.branches)[1:]
    assert np.allclose(Db.reshape(-1, 8).sum(axis=1), (fp.n_sites - 2) * T, rtol=1e-9, atol=0)
    o.close()


@pytest.mark.parametrize("n", SIZES)
def test_oracle_small_cases(n):
    for name in TREES:
        _oracle_against_yardstick(*small(name, n))


@pytest.mark.parametrize("name", DENSE)
def test_oracle_dense_cases(name):
    model, tree, fp = dc.workload(name)
    cap = dc.capacity(name, fp)
    _oracle_against_yardstick(model, tree, fp, cap, o=dc.oracle(name, cap))


def test_cases_cover_the_shapes():
    """the cuts fall inside a wave and inside a block, the halos last the run, and the group really splits"""
    from epievo_amd.parallel import halo_width
    for n, cut, halo in CUTS:
        assert cut % 64 and (cut - halo) % 64 and (cut + halo) % 256 and halo >= 6 * (BURN_IN + BATCH) + 2 and halo % 2
        assert 0 < cut - halo and cut + halo < n
    assert GROUP_N >= 3 * (2 * halo_width(BURN_IN + BATCH) + 2 * 256)
    assert config("bal8").n_nodes - 1 > 8 and config("pair").n_nodes - 1 == 1 and config("tree").n_nodes - 1 == 4
