"""Chain mixing diagnostics counted on the device during run_mcmc (epv_set_mixing): samples, pair counts and every
row equal, bit for bit, what numpy computes from the CPU oracle's paths after every sweep (rung B, the same Philox
sweeps; tests/mixing_ref.py) on every kernel path, over two run_mcmc calls (a run boundary) with a batch beyond the
lag (the ring wraps), for one context and a LocalGroup of three, and for explicit samples under the run rules;
counting changes neither J, D, the accept count, the paths nor tri_llh; all ten layers on at once give what each
gives alone."""
import numpy as np
import pytest

import mixing_ref
import orc
from common import simulate
from epievo_amd.parallel import LocalGroup
from epievo_amd.sampler import EPV_ERR_ARG, EPV_ERR_STATE, DeviceSampler, EpvError

pytestmark = pytest.mark.gpu

MAX_LAG, BURN_IN, BATCH, SEED = 3, 1, 5, 77


def _dev(tree, model, fp, cap):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    return d


def _cap(fp):
    return int(max(16, 2 * fp.counts().max() + 8))


def _oracle_two_calls(tree, model, fp, cap, seed=SEED, max_lag=MAX_LAG, burn_in=BURN_IN, batch=BATCH, base=5):
    """two run_mcmc calls on the oracle -> (the yardstick, the accept counts of the batch sweeps, the final paths,
    sites with a linked pair whose init states and jump counts agree and whose times differ)"""
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    o.reset()
    m = mixing_ref.Mixing(fp.n_sites, max_lag)
    nacc, w, times_only = 0, base, np.zeros(fp.n_sites, bool)
    for _ in range(2):
        for _ in range(burn_in):
            o.sweep(w)
            w += 1
        last = o.paths()
        m.open_run(last)
        for _ in range(batch):
            nacc += o.sweep(w)
            w += 1
            p = o.paths()
            B, n = p.n_nodes - 1, p.n_sites
            same_shape = ((p.init.reshape(B, n) == last.init.reshape(B, n)).all(axis=0) &
                          (p.counts().reshape(B, n) == last.counts().reshape(B, n)).all(axis=0))
            times_only |= same_shape & mixing_ref.differs(last, p)
            m.sample(p)
            last = p
        m.close_run()
    return m, nacc, o.paths(), times_only


def _assert_counts_equal(got, want):
    assert got[0] == want[0] and got[1] == want[1], (got[:2], want[:2])
    names = ("pairs", "moved", "S1", "S2", "C")
    for name, a, b in zip(names, got[2:], want[2:]):
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, a.shape, b.dtype, b.shape)
        assert np.array_equal(a, b), (name, np.nonzero(a != b))


# (EPV_PHASE_*: 1 = V2 kernels, 2 = V2 with segment-parallel jumps, 3 = fused phase, 4 = V3 large-tree kernels)
NO_FUSED = {"EPV_FUSED_PHASE": "0"}
SEG = {"EPV_FUSED_PHASE": "0", "EPV_SEG_JUMPS": "1"}


@pytest.mark.parametrize("cfg,n,env,mode", [
    ("tree", 40000, {}, 3), ("tree", 3001, NO_FUSED, 1), ("bal16", 3000, {}, 4), ("pair", 4000, SEG, 2),
    ("tree", 3, {}, None), ("tree", 257, {}, None)])
def test_counts_match_oracle_and_change_nothing(monkeypatch, cfg, n, env, mode):
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # read when a context is created
    model, tree, fp = simulate(cfg, n, seed=6)
    cap = _cap(fp)
    on, off = _dev(tree, model, fp, cap), _dev(tree, model, fp, cap)
    assert on.phase_mode() == off.phase_mode()
    if mode is not None:
        assert on.phase_mode() == mode
    on.enable_mixing(MAX_LAG)
    assert on.mixing_layout() == (0, n, MAX_LAG)                           # sites 0 and n - 1 included
    on.reset()
    off.reset()
    # 1. nothing else changes, over two calls
    acc = 0
    for call in range(2):
        base = 5 + call * (BURN_IN + BATCH)
        J1, D1, a1 = on.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=base)
        J0, D0, a0 = off.run_mcmc(BURN_IN, BATCH, SEED, sweep_base=base)
        assert a1 == a0 and np.array_equal(J1, J0) and np.array_equal(D1, D0)
        acc += a1
    assert orc.paths_equal(on.paths(), off.paths())
    assert np.array_equal(on.tri_llh(), off.tri_llh())
    # 2. the counts, bit for bit
    got = on.mixing(counts=True)
    ref, nacc, opaths, times_only = _oracle_two_calls(tree, model, fp, cap)
    assert orc.paths_equal(on.paths(), opaths) and nacc == acc
    _assert_counts_equal(got, ref.counts())
    ns, mp, pairs, moved, S1, S2, C = got
    assert (ns, mp) == (2 * BATCH, 2 * BATCH) and on.mixing_samples() == ns
    assert pairs.tolist() == [0] + [2 * (BATCH - k) for k in range(1, MAX_LAG + 1)]
    # 3. nothing is vacuous
    if n not in (3, 257):
        assert ((moved > 0) & (moved < mp)).any()
        assert C[MAX_LAG - 1].any()
        assert times_only.any()             # a fingerprint that skipped the jump times would miss these moves
        assert (moved[times_only] > 0).all()
    # 4. invariants of the device result itself
    assert (moved <= mp).all() and int(moved.sum(dtype=np.uint64)) <= acc
    assert all(ns * int(b) >= int(a) ** 2 for a, b in zip(S1[:2000], S2[:2000]))
    assert (float(ns) * S2.astype(np.float64) >= S1.astype(np.float64) ** 2 * (1.0 - 1e-12)).all()
    assert moved[0] == 0 and moved[n - 1] == 0                             # the sampler never changes the end sites
    # the summary is host.mixing_summary of the counts, and the window sums are numpy's
    s = on.mixing()
    assert s["samples"] == ns and np.array_equal(s["move_rate"], moved / float(mp))
    for W in (1, 7, 1000):
        wns, wmp, win = on.mixing_windows(W)
        assert (wns, wmp) == (ns, mp) and win.dtype == np.uint64
        assert np.array_equal(win, mixing_ref.windows(moved, W))
    on.reset_mixing()
    z = on.mixing(counts=True)
    assert z[:2] == (0, 0) and not any(a.any() for a in z[2:])
    on.close()
    off.close()


def test_local_group_equals_single_context():
    n = 20011
    model, tree, fp = simulate("tree", n, seed=4)
    cap = _cap(fp)
    one = _dev(tree, model, fp, cap)
    g = LocalGroup(0, 3)
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    assert len(g.subs) == 3
    res = []
    for s in (one, g):
        s.enable_mixing(MAX_LAG)
        s.reset()
        res.append([s.run_mcmc(BURN_IN, BATCH, 99, sweep_base=7 + c * (BURN_IN + BATCH)) for c in range(2)])
    for (J, D, a), (Jg, Dg, ag) in zip(*res):
        assert a == ag and np.array_equal(J, Jg) and np.array_equal(D, Dg)
    got1, got3 = one.mixing(counts=True), g.mixing(counts=True)
    assert got3[3].shape == (n,) and g.mixing_layout() == (0, n, MAX_LAG)
    _assert_counts_equal(got3, got1)
    ref, _, _, _ = _oracle_two_calls(tree, model, fp, cap, seed=99, base=7)
    _assert_counts_equal(got3, ref.counts())
    assert any(a % 1000 for a in g.a[1:])                   # 1000 divides none of the shard cuts
    w1, w3 = one.mixing_windows(1000), g.mixing_windows(1000)
    assert w1[:2] == w3[:2] and np.array_equal(w1[2], w3[2]) and np.array_equal(w3[2], mixing_ref.windows(got1[3], 1000))
    one.close()
    g.close()


def test_explicit_samples_follow_the_run_rules():
    n = 5000
    model, tree, fp = simulate("tree", n, seed=3)
    cap = _cap(fp)
    d = _dev(tree, model, fp, cap)
    d.enable_mixing(MAX_LAG)
    d.reset()
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=21)
    o.reset()
    m = mixing_ref.Mixing(n, MAX_LAG)
    # three single sweeps, a sample after each: the first opens a run, the next two are linked
    for w in range(3):
        assert d.sweep(1, 21, sweep_base=w) == o.sweep(w)
        d.accumulate_mixing()
        m.sample(o.paths(), linked=w > 0)
    _assert_counts_equal(d.mixing(counts=True), m.counts())
    assert (m.samples, m.moved_pairs) == (3, 2) and m.pairs.tolist() == [0, 2, 1, 0] and m.moved.any()
    # two sweeps since the last sample: a new run, linked to nothing
    assert d.sweep(2, 21, sweep_base=3) == o.sweep(3) + o.sweep(4)
    d.accumulate_mixing()
    m.sample(o.paths(), linked=False)
    _assert_counts_equal(d.mixing(counts=True), m.counts())
    # one sweep: linked again
    assert d.sweep(1, 21, sweep_base=5) == o.sweep(5)
    d.accumulate_mixing()
    m.sample(o.paths())
    _assert_counts_equal(d.mixing(counts=True), m.counts())
    assert (m.samples, m.moved_pairs) == (5, 3) and m.pairs.tolist() == [0, 3, 1, 0]
    # new branch lengths between two samples close the run, although exactly one sweep has passed
    nb = tree.branches * 1.25
    d.scale_jump_times(nb)
    o.scale_jump_times(nb)
    d.reset()
    o.reset()
    assert d.sweep(1, 21, sweep_base=6) == o.sweep(6)
    d.accumulate_mixing()
    m.sample(o.paths(), linked=False)
    got = d.mixing(counts=True)
    _assert_counts_equal(got, m.counts())
    assert (got[0], got[1]) == (6, 3)
    # a run_mcmc call closes its run: the sample after one more sweep is linked to nothing
    d.run_mcmc(0, 2, 21, sweep_base=7)
    m.open_run(o.paths())
    for w in (7, 8):
        o.sweep(w)
        m.sample(o.paths())
    m.close_run()
    assert d.sweep(1, 21, sweep_base=9) == o.sweep(9)
    d.accumulate_mixing()
    m.sample(o.paths(), linked=False)
    got = d.mixing(counts=True)
    _assert_counts_equal(got, m.counts())
    assert (got[0], got[1]) == (9, 5) and got[2].tolist() == [0, 4, 1, 0]
    d.close()


def test_refusals():
    model, tree, fp = simulate("pair", 3001, seed=6)
    d = _dev(tree, model, fp, _cap(fp))
    # off: nothing to read, nothing to add to
    for call in (d.mixing, lambda: d.mixing_windows(10), d.accumulate_mixing, d.reset_mixing):
        with pytest.raises(EpvError) as e:
            call()
        assert e.value.code == EPV_ERR_STATE and "mixing diagnostics are off: epv_set_mixing first" in str(e.value)
    assert d.mixing_samples() == 0 and d.mixing_layout() == (0, 0, 0)
    # max_lag: 1 .. 16; 17 is refused and leaves the layer as it was (off), 0 is the C ABI's "off"
    with pytest.raises(EpvError) as e:
        d.enable_mixing(17)
    assert e.value.code == EPV_ERR_ARG and d.mixing_layout() == (0, 0, 0)
    d.enable_mixing(16)
    assert d.mixing_layout() == (0, 3001, 16)
    d.enable_mixing(0)
    with pytest.raises(EpvError) as e:
        d.mixing()
    assert e.value.code == EPV_ERR_STATE
    d.enable_mixing(MAX_LAG)
    # before the first sample a new site range lays out again; afterwards it is an error
    d.set_update_range(10, 2000)
    assert d.mixing_layout() == (10, 1991, MAX_LAG)
    d.set_update_range(1, 2999)
    d.reset()
    d.run_mcmc(0, 1, 5)
    assert d.mixing_samples() == 1
    d.set_update_range(10, 2000)
    d.reset()
    with pytest.raises(EpvError) as e:
        d.run_mcmc(0, 1, 5, sweep_base=1)
    assert e.value.code == EPV_ERR_STATE and "sites of this context changed after the mixing diagnostics took samples" in str(e.value)
    d.set_update_range(1, 2999)
    d.reset()
    # the cap: a batch that would pass 2^21 samples is refused before any sweep
    paths, before = d.paths(), d.mixing(counts=True)
    with pytest.raises(EpvError) as e:
        d.run_mcmc(0, 2 ** 21, 5, sweep_base=2)
    assert e.value.code == EPV_ERR_STATE and "would pass 2097152 samples" in str(e.value)
    assert orc.paths_equal(d.paths(), paths)
    _assert_counts_equal(d.mixing(counts=True), before)
    d.close()


def test_all_ten_layers_together():
    """every layer on at once gives what it gives alone, the tenth included"""
    n = 3001
    model, tree, fp = simulate("tree", n, seed=6)
    cap = _cap(fp)
    enable = {
        "path_average": (7,), "branch_events": (), "window_stats": (100,), "epoch_stats": (3,), "lineage_origins": (),
        "domain_stats": (8,), "change_patterns": (), "domain_turnover": (8,), "spatial_correlation": (5, 8),
        "mixing": (MAX_LAG,)}
    read = {
        "path_average": lambda d: d.path_average(counts=True), "branch_events": lambda d: d.branch_events(counts=True),
        "window_stats": lambda d: d.window_stats(counts=True), "epoch_stats": lambda d: d.epoch_raw(),
        "lineage_origins": lambda d: d.lineage_origins(counts=True), "domain_stats": lambda d: d.domain_stats(),
        "change_patterns": lambda d: d.change_patterns(counts=True), "domain_turnover": lambda d: d.domain_turnover(),
        "spatial_correlation": lambda d: d.spatial_correlation(), "mixing": lambda d: d.mixing(counts=True)}

    def run(stems):
        d = _dev(tree, model, fp, cap)
        for stem in stems:
            getattr(d, "enable_" + stem)(*enable[stem])
        d.reset()
        out = [d.run_mcmc(BURN_IN, 4, SEED, sweep_base=c * 5) for c in range(2)]
        res = {stem: read[stem](d) for stem in stems}
        d.close()
        return out, res

    out_all, together = run(list(enable))
    for stem in enable:
        out, alone = run([stem])
        for (J, D, a), (Ja, Da, aa) in zip(out, out_all):
            assert a == aa and np.array_equal(J, Ja) and np.array_equal(D, Da)
        assert len(alone[stem]) == len(together[stem]), stem
        for x, y in zip(alone[stem], together[stem]):
            assert np.array_equal(np.asarray(x), np.asarray(y)), stem
    assert together["mixing"][0] == 8 and together["mixing"][3].any()
