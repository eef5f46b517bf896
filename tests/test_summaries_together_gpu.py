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


# ---- the five layers that are joint along the genome, which pack their bit rows with one kernel (epv_rows.h)
# a caterpillar of five leaves: B = 8 branches, exactly one full batch of the pack kernel's meta loads; bal16 has
# B = 30, a partial last batch
CAT5_NWK = "((((A:0.05,B:0.07)U:0.04,C:0.1)V:0.03,D:0.15)W:0.06,E:0.2)R:0.0;\n"
PART_N, PART_LO, PART_HI, PART_BATCH, PART_LAG = 700, 37, 373, 2, 65
PART_LAYERS = {
    "domain_stats": (lambda d, state: d.enable_domain_stats(PART_BATCH), lambda d: d.domain_stats_part()),
    "domain_turnover": (lambda d, state: d.enable_domain_turnover(PART_BATCH), lambda d: d.domain_turnover_part()),
    "spatial_correlation": (lambda d, state: d.enable_spatial_correlation(PART_LAG, PART_BATCH),
                            lambda d: d.spatial_correlation_part()),
    "domain_maps": (lambda d, state: d.enable_domain_maps((1, 5, 20), state, PART_BATCH), lambda d: d.domain_maps_part()),
    "change_tracts": (lambda d, state: d.enable_change_tracts(PART_BATCH), lambda d: d.change_tracts_part()),
}


def _part_inputs(cfg):
    if cfg == "cat5":
        from common import _tmp, ref_test_model
        from epievo_amd import host
        model, tree = ref_test_model(), host.Tree.read(_tmp("cat5.nwk", CAT5_NWK))
        return model, tree, host.simulate(model, tree, PART_N, 6)
    return simulate(cfg, PART_N, seed=6)


@pytest.mark.parametrize("cfg,state", [("cat5", 0), ("bal16", 1)])
def test_part_layers_together_equal_each_alone(cfg, state):
    """One context that counts sites 37 .. 373: 337 sites, six words of which the last holds 17 sites, two blocks of
    the pack kernel of which the second has two tiles.  The five layers on at once, each packing its own rows in the
    same run, give bit for bit the part each gives alone; and where two layers pack the same rows, their results
    agree: the node rows of the spectra and the correlations (a node's pairs that disagree at lag 1 are its run ends),
    the end rows of the turnover and the node rows of the spectra (a row's runs, kept or not, are the node's), the
    end rows of the turnover and of the tracts (below)."""
    model, tree, fp = _part_inputs(cfg)
    cap, N = _cap(fp), tree.n_nodes
    B, cnt = N - 1, PART_HI - PART_LO + 1
    assert cnt % 64 and ((cnt + 63) // 64) % 4

    def run(names):
        d = DeviceSampler(0)
        d.set_tree(tree)
        d.set_model(model)
        d.upload_paths(fp, cap)
        d.set_update_range(PART_LO, PART_HI)
        for name in names:
            PART_LAYERS[name][0](d, state)
        d.reset()
        out = d.run_mcmc(BURN_IN, PART_BATCH, SEED, sweep_base=BASE)
        return d, out

    d, out = run(list(PART_LAYERS)[::-1])             # (switched on against the order of the chain)
    together = {name: PART_LAYERS[name][1](d) for name in PART_LAYERS}
    for name in PART_LAYERS:
        one, out1 = run([name])
        alone = PART_LAYERS[name][1](one)
        one.close()
        assert out1[2] == out[2] and np.array_equal(out1[0], out[0]) and np.array_equal(out1[1], out[1]), name
        assert alone[0] == PART_BATCH and any(np.asarray(x).any() for x in alone[1:]), name      # (not vacuous)
        assert len(alone) == len(together[name]), name
        for x, y in zip(alone, together[name]):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), name
    assert d.domain_stats_layout()[:4] == (N, 128, PART_LO, cnt)
    assert d.domain_turnover_layout()[:4] == (2 * B, 128, PART_LO, cnt)
    assert d.spatial_correlation_layout()[:4] == (N + B, PART_LAG, PART_LO, cnt)
    assert d.domain_maps_layout()[:5] == (N, (1, 5, 20), state, PART_LO, cnt)
    assert d.change_tracts_layout()[:5] == (B, 27, 128, PART_LO, cnt)
    # node rows: the spectra and the correlations
    dns, dhist, dlen = d.domain_stats()
    cns, n11, left1, right1 = d.spatial_correlation()
    assert dns == cns == PART_BATCH
    for v in range(N):
        disagree = int(left1[v, 1] - n11[v, 1]) + int(right1[v, 1] - n11[v, 1])
        assert disagree == int(dhist[v].sum()) - PART_BATCH
        assert int(n11[v, 0]) == int(dlen[v, 1])      # the ones of a node's row
    # end rows and node rows: the turnover and the spectra
    tns, thist, tlen, tedges = together["domain_turnover"]
    _, phist, plen, _ = together["domain_stats"]
    for b in range(B):
        for row, node in ((2 * b + 1, b + 1), (2 * b, int(tree.parent_ids[b + 1]))):
            assert np.array_equal(thist[row].sum(axis=1), phist[node]) and np.array_equal(tlen[row].sum(axis=1), plen[node])
    # end rows: the turnover and the tracts.  Over the samples, the ones of a branch's end row less those of its
    # start row are its gained less its lost sites.  The pure tracts say how many of each they hold; a mixed tract
    # holds at least one of each, so the mixed tracts' M sites in m tracts leave a difference of at most M - 2 m, of
    # the parity of M.  A run that turned over holds changed sites alone: no more than the tracts hold
    _, _, clen = d.domain_turnover()
    _, xhist, xlen = d.change_tracts()
    assert (clen.sum(axis=(1, 2)) == PART_BATCH * cnt).all()
    for b in range(B):
        net = int(clen[2 * b + 1, 1].sum()) - int(clen[2 * b, 1].sum())
        pure = int(xlen[b, 0:9].sum()) - int(xlen[b, 9:18].sum())
        M, m = int(xlen[b, 18:27].sum()), int(xhist[b, 18:27].sum())
        assert abs(net - pure) <= M - 2 * m and (net - pure - M) % 2 == 0, b
        assert max(int(clen[2 * b, :, 0].sum()), int(clen[2 * b + 1, :, 0].sum())) <= int(xlen[b].sum()), b
    assert int(xlen.sum()) > 0 and int(clen[:, :, 0].sum()) > 0       # (changes exist, and runs that turned over)
    d.close()


# two trees of five nodes: parents (0, 0, 1, 1, 0) and (0, 0, 0, 2, 2).  The paths of one fit the other
LIFE_NWK = ("((A:0.1,B:0.2)U:0.1,C:0.3)R:0.0;\n", "(A:0.1,(B:0.2,C:0.3)U:0.1)R:0.0;\n")
LIFE_ENABLE = {
    "domain_stats": lambda d, m: d.enable_domain_stats(m), "domain_turnover": lambda d, m: d.enable_domain_turnover(m),
    "spatial_correlation": lambda d, m: d.enable_spatial_correlation(8, m),
    "domain_maps": lambda d, m: d.enable_domain_maps((1, 3), 1, m), "change_tracts": lambda d, m: d.enable_change_tracts(m)}
LIFE_NOUN = {"domain_stats": "domain statistics", "domain_turnover": "domain turnover",
             "spatial_correlation": "spatial correlations", "domain_maps": "domain maps", "change_tracts": "change tracts"}


@pytest.mark.parametrize("name", list(LIFE_ENABLE))
def test_part_layer_lifecycle(name):
    """what the five layers that keep a part share (PartState in epv_abi.hip), on a small tree at 65 sites: a reset and
    a read-out with no samples; a sample beyond max_samples; the tree changed after samples, which the spectra
    refuse (their rows depend on every parent) and the other four take (theirs depend on the number of nodes and the
    root's first child, or on the branches alone); the site range changed after samples"""
    from common import _tmp, ref_test_model
    from epievo_amd import host
    n = 65
    model = ref_test_model()
    tree, other = (host.Tree.read(_tmp("life%d.nwk" % i, nwk)) for i, nwk in enumerate(LIFE_NWK))
    assert tree.n_nodes == other.n_nodes == 5 and list(tree.parent_ids) != list(other.parent_ids)
    fp = host.simulate(model, tree, n, 6)
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, _cap(fp))
    LIFE_ENABLE[name](d, 2)
    d.reset()
    part, samples = getattr(d, name + "_part"), getattr(d, name + "_samples")
    accumulate, reset, layout = getattr(d, "accumulate_" + name), getattr(d, "reset_" + name), getattr(d, name + "_layout")
    # no samples: reset, then read
    reset()
    got = part()
    assert got[0] == 0 and samples() == 0 and not any(np.asarray(x).any() for x in got[2 if name in ("spatial_correlation", "domain_maps") else 1:])
    # a sample beyond max
    accumulate()
    accumulate()
    held = part()
    with pytest.raises(EpvError) as e:
        accumulate()
    assert e.value.code == EPV_ERR_STATE and "samples" in str(e.value) and LIFE_NOUN[name] in str(e.value)
    assert "epv_reset_" + name in str(e.value) and "epv_set_" + name in str(e.value) and samples() == 2
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(part(), held))
    # the tree changed after samples
    reset()
    accumulate()
    d.set_tree(other)
    if name == "domain_stats":
        with pytest.raises(EpvError) as e:
            accumulate()
        assert e.value.code == EPV_ERR_STATE and "the tree changed after the domain statistics took samples" in str(e.value)
        assert "epv_reset_domain_stats" in str(e.value) and samples() == 1
        reset()                                       # (no samples: laid out for the tree of now)
        accumulate()
        assert samples() == 1
    else:
        accumulate()
        assert samples() == 2
    d.set_tree(tree)
    # the site range changed after samples
    reset()
    accumulate()
    d.set_update_range(5, 40)
    with pytest.raises(EpvError) as e:
        accumulate()
    assert e.value.code == EPV_ERR_STATE and "sites of this context changed after the " + LIFE_NOUN[name] in str(e.value)
    assert "epv_set_" + name + " again" in str(e.value) and samples() == 1
    LIFE_ENABLE[name](d, 1)
    first_count = layout()[-3:-1]
    assert first_count == (5, 36) and samples() == 0
    accumulate()
    assert samples() == 1 and part()[0] == 1
    d.close()
