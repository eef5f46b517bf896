"""The six posterior summaries of run_mcmc switched on together (the table of layers in epv_abi.hip, DESIGN.md
section 7.15).  Every other test enables one layer at a time; these pin that the layers coexist and in which order
the chain takes them:

  * all six on give, bit for bit, the integers and sample counts that each gives alone, and the J, D, accept
    count and paths of a context with no layer;
  * the same through two contexts on one GPU (LocalGroup);
  * of two layers that would both refuse a batch, the earlier one of the chain is the one reported, before any
    sweep;
  * switching the layers off frees and forgets: no samples, every read-out refused, the chain as without them,
    and a layer switched on again starts from zero.

About 300 sites: the owned range spans two 256-site blocks and five 64-site tiles.  The LocalGroup case takes
2100 sites, the fewest at which the group keeps two contexts (each must own more than its two halos of 256)."""
import numpy as np
import pytest

import orc
from common import simulate
from epievo_amd.parallel import LocalGroup
from epievo_amd.sampler import EPV_ERR_STATE, DeviceSampler, EpvError

pytestmark = pytest.mark.gpu

N_SITES, N_GROUP = 300, 2100
SEED, BASE, BURN_IN, BATCH = 77, 5, 1, 3

# in the order of the chain
LAYERS = ("path_average", "branch_events", "window_stats", "epoch_stats", "lineage_origins", "domain_stats")
ENABLE = {
    "path_average": lambda d: d.enable_path_average(3),
    "branch_events": lambda d: d.enable_branch_events(True),
    "window_stats": lambda d: d.enable_window_stats(48),
    "epoch_stats": lambda d: d.enable_epoch_stats(4),
    "lineage_origins": lambda d: d.enable_lineage_origins(True),
    "domain_stats": lambda d: d.enable_domain_stats(BATCH),
}
DISABLE = {
    "path_average": lambda d: d.enable_path_average(0),
    "branch_events": lambda d: d.enable_branch_events(False),
    "window_stats": lambda d: d.enable_window_stats(0),
    "epoch_stats": lambda d: d.enable_epoch_stats(0),
    "lineage_origins": lambda d: d.enable_lineage_origins(False),
    "domain_stats": lambda d: d.enable_domain_stats(0),
}
# the integer read-out of a context: a tuple that begins with the sample count
READ = {
    "path_average": lambda d: d.path_average(counts=True),
    "branch_events": lambda d: d.branch_events(counts=True),
    "window_stats": lambda d: d.window_stats(counts=True),
    "epoch_stats": lambda d: d.epoch_raw(),
    "lineage_origins": lambda d: d.lineage_origins(counts=True),
    "domain_stats": lambda d: d.domain_stats_part(),
}
SAMPLES = {name: (lambda d, name=name: getattr(d, name + "_samples")()) for name in LAYERS}
OFF_TEXT = {
    "path_average": "path average is off",
    "branch_events": "branch events are off: epv_set_branch_events first",
    "window_stats": "window statistics are off: epv_set_window_stats first",
    "epoch_stats": "epoch statistics are off: epv_set_epoch_stats first",
    "lineage_origins": "lineage origins are off: epv_set_lineage_origins first",
    "domain_stats": "domain statistics are off: epv_set_domain_stats first",
}


def _cap(fp):
    return int(max(16, 2 * fp.counts().max() + 8))


def _dev(tree, model, fp, cap, layers=()):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    for name in layers:
        ENABLE[name](d)
    d.reset()
    return d


def _run(d, sweep_base=BASE, burn_in=BURN_IN):
    J, D, acc = d.run_mcmc(burn_in, BATCH, SEED, sweep_base=sweep_base)
    return J, D, acc, d.paths()


def _same_run(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and orc.paths_equal(a[3], b[3])


def _same_readout(a, b):
    """sample counts equal, arrays equal in type, shape and every integer"""
    if len(a) != len(b) or a[0] != b[0]:
        return False
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


@pytest.fixture(scope="module")
def case():
    """the inputs, the run of a context with no layer, and every layer's read-out on a context of its own"""
    model, tree, fp = simulate("tree", N_SITES, seed=4)
    cap = _cap(fp)
    none = _dev(tree, model, fp, cap)
    plain = _run(none)
    none.close()
    alone = {}
    for name in LAYERS:
        d = _dev(tree, model, fp, cap, (name,))
        assert _same_run(_run(d), plain), name
        alone[name] = READ[name](d)
        assert alone[name][0] == BATCH and any(np.asarray(x).any() for x in alone[name][1:]), name   # (not vacuous)
        d.close()
    return model, tree, fp, cap, plain, alone


def test_all_on_equals_each_alone(case):
    model, tree, fp, cap, plain, alone = case
    d = _dev(tree, model, fp, cap, LAYERS[::-1])     # (switched on against the order of the chain)
    assert _same_run(_run(d), plain)
    for name in LAYERS:
        assert SAMPLES[name](d) == BATCH, name
        assert _same_readout(READ[name](d), alone[name]), name
    d.close()


def test_two_contexts_on_one_gpu():
    model, tree, fp = simulate("tree", N_GROUP, seed=4)
    cap = _cap(fp)
    one = _dev(tree, model, fp, cap, LAYERS)
    plain = _run(one)
    runs = []
    for layers in ((), LAYERS):
        g = LocalGroup(0, shards=2, sweeps_per_refresh=10)
        g.set_tree(tree)
        g.set_model(model)
        g.upload_paths(fp, cap)
        assert len(g.subs) == 2
        for name in layers:
            ENABLE[name](g)
        g.reset()
        runs.append(_run(g))
        if layers:
            for name in LAYERS:
                assert SAMPLES[name](g) == BATCH, name
            assert _same_readout(g.window_stats(counts=True), one.window_stats(counts=True))
            ns, J, D = g.epoch_stats(counts=True)
            ns1, J1, D1 = one.epoch_stats(counts=True)
            assert ns == ns1 == BATCH and J.dtype == J1.dtype and np.array_equal(J, J1)
            assert D.shape == D1.shape and all(int(a) == int(b) for a, b in zip(D.reshape(-1), D1.reshape(-1)))
            assert J.any() and any(int(a) for a in D.reshape(-1))
        g.close()
    assert _same_run(runs[0], plain) and _same_run(runs[1], plain)
    one.close()


def test_first_layer_of_the_chain_that_refuses_is_reported(case):
    model, tree, fp, cap, _, _ = case
    d = _dev(tree, model, fp, cap, LAYERS[::-1])
    d._ck(d.L.epv_lineage_origins_set_samples(d.h, 2 ** 21 - 1))
    d._ck(d.L.epv_branch_events_set_samples(d.h, 2 ** 21 - 1))
    paths = d.paths()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(0, 2, SEED, sweep_base=BASE)
    assert e.value.code == EPV_ERR_STATE and "branch events" in str(e.value) and "lineage origins" not in str(e.value)
    assert orc.paths_equal(d.paths(), paths)         # a refused run has not swept
    d.reset_branch_events()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(0, 2, SEED, sweep_base=BASE)
    assert e.value.code == EPV_ERR_STATE and "lineage origins" in str(e.value) and "branch events" not in str(e.value)
    assert orc.paths_equal(d.paths(), paths)
    assert all(SAMPLES[name](d) == 0 for name in LAYERS if name != "lineage_origins")   # no layer took a sample
    d.close()


def test_off_frees_and_forgets(case):
    model, tree, fp, cap, plain, _ = case
    none = _dev(tree, model, fp, cap)
    d = _dev(tree, model, fp, cap, LAYERS)
    assert _same_run(_run(d), plain) and _same_run(_run(none), plain)
    for name in LAYERS:
        DISABLE[name](d)
    for name in LAYERS:
        assert SAMPLES[name](d) == 0, name
        with pytest.raises(EpvError) as e:
            READ[name](d)
        assert e.value.code == EPV_ERR_STATE and OFF_TEXT[name] in str(e.value), name
    with pytest.raises(EpvError) as e:               # (the wrapper above answers for the path average itself)
        d._ck(d.L.epv_get_path_average(d.h, 0, 0, None))
    assert e.value.code == EPV_ERR_STATE and "path average is off: epv_set_path_average first" in str(e.value)
    more = BASE + BURN_IN + BATCH
    assert _same_run(_run(d, more, 0), _run(none, more, 0))
    d.enable_branch_events(True)
    ns, planes = d.branch_events(counts=True)
    assert ns == 0 and not planes.any()
    d.run_mcmc(0, 1, SEED, sweep_base=more + BATCH)
    assert d.branch_events_samples() == 1 and all(SAMPLES[name](d) == 0 for name in LAYERS if name != "branch_events")
    d.close()
    none.close()
