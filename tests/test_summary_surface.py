"""The posterior summaries in the Python layers above the device, without a GPU: the public surface of the five
samplers as it was before the layers were given one shape (names and parameter lists, recorded then), the one C ABI
table, LocalGroup's lifecycle methods and read-outs of all nine summaries over stand-ins for its shards, and
ShardedSampler.path_average over stand-ins for the device and the collective."""
import inspect
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import corr_ref
import domains_ref
import turnover_ref
from epievo_amd import _build, host

# public methods and their parameters (inspect.signature), recorded from the commit before the refactor
SURFACE = {
    "DeviceSampler": """
        accumulate_branch_events(self); accumulate_change_patterns(self); accumulate_domain_stats(self);
        accumulate_domain_turnover(self); accumulate_epoch_stats(self); accumulate_lineage_origins(self);
        accumulate_path_average(self); accumulate_spatial_correlation(self); accumulate_window_stats(self); alloc(self,
        nbytes); branch_event_windows(self, W, first_window=0, n_windows=None); branch_events(self, counts=False);
        branch_events_layout(self); branch_events_samples(self); capacity(self); change_pattern_windows(self, W,
        first_window=0, n_windows=None); change_patterns(self, counts=False); change_patterns_layout(self);
        change_patterns_samples(self); close(self); column_bytes(self); copy_columns_to(self, first, count, other,
        other_first); counters(self); counts_to_stats(self, counts, batch, average=True); dev_alloc(self, nbytes);
        dev_free(self, p); domain_stats(self); domain_stats_layout(self); domain_stats_part(self);
        domain_stats_samples(self); domain_turnover(self); domain_turnover_layout(self); domain_turnover_part(self);
        domain_turnover_samples(self); enable_branch_events(self, on=True); enable_change_patterns(self, on=True);
        enable_domain_stats(self, max_samples); enable_domain_turnover(self, max_samples); enable_epoch_stats(self, P);
        enable_lineage_origins(self, on=True); enable_path_average(self, n_points); enable_spatial_correlation(self,
        max_lag, max_samples); enable_window_stats(self, W); epoch_raw(self); epoch_stats(self, counts=False);
        epoch_stats_layout(self); epoch_stats_samples(self); forward_last_ms(self); forward_simulate(self, n_sites,
        seed, root=None, capacity=0); get_columns(self, first, count); halo_phases_left(self); indep_expectation(self,
        rates); indep_node_posterior(self, rates); indep_suffstats(self); indep_update_paths(self, rates, seed,
        sweep=0); init_paths_indep(self, root, leaf, seed, capacity=0); kernel_time_ms(self); leaf_evidence_cells(self);
        lineage_origin_rows(self); lineage_origin_windows(self, W, first_window=0, n_windows=None);
        lineage_origins(self, counts=False); lineage_origins_layout(self); lineage_origins_samples(self);
        lineage_origins_scale_exp(self); math_kat(self, op, items, where=0); merge_kat(self, items); pack_columns(self,
        first, count, buf); path_average(self, counts=False, chunk_bytes=268435456); path_average_layout(self);
        path_average_samples(self); paths(self); phase_mode(self); phase_plan(self); philox_kat(self, seed, counters);
        put_columns(self, first, count, buf); read(self, buf, offset, count, dtype=<class 'numpy.float64'>);
        reset(self); reset_branch_events(self); reset_change_patterns(self); reset_domain_stats(self);
        reset_domain_turnover(self); reset_epoch_stats(self); reset_lineage_origins(self); reset_path_average(self);
        reset_spatial_correlation(self); reset_window_stats(self); run_mcmc(self, burn_in, batch, seed, sweep_base=0,
        average=True); run_mcmc_counts(self, burn_in, batch, seed, sweep_base=0); scale_jump_times(self, new_branches);
        set_capacity(self, capacity); set_halo(self, left, right); set_leaf_evidence(self, p_state1); set_model(self,
        model); set_options(self, reference_proposal_ratio=False, forward_rejection=False, sample_root=False);
        set_timing(self, on); set_tree(self, tree); set_unobserved(self, mask); set_update_range(self, first, last);
        spatial_correlation(self); spatial_correlation_layout(self); spatial_correlation_part(self);
        spatial_correlation_samples(self); suffstats(self); sweep(self, n_sweeps, seed, sweep_base=0); sweep_phase(self,
        colour, seed, sweep); tri_llh(self); unobserved_cells(self); unpack_columns(self, first, count, buf);
        upload_paths(self, fp, capacity=0, global_site_offset=0, n_global=None); window_counts(self, first_window=0,
        n_windows=None); window_counts_to_stats(self, counts, samples); window_stats(self, counts=False);
        window_stats_layout(self); window_stats_samples(self); window_stats_scale_exps(self); write(self, buf, offset,
        arr)
    """,
    "SingleSiteSampler": """
        accumulate_branch_events(self); accumulate_change_patterns(self); accumulate_domain_stats(self);
        accumulate_domain_turnover(self); accumulate_epoch_stats(self); accumulate_lineage_origins(self);
        accumulate_path_average(self); accumulate_spatial_correlation(self); accumulate_window_stats(self);
        branch_event_windows(self, W); branch_events(self, counts=False); change_pattern_windows(self, W);
        change_patterns(self, counts=False); change_patterns_layout(self); change_patterns_samples(self);
        domain_stats(self); domain_stats_layout(self); domain_stats_part(self); domain_stats_samples(self);
        domain_turnover(self); domain_turnover_layout(self); domain_turnover_part(self); domain_turnover_samples(self);
        enable_branch_events(self, on=True); enable_change_patterns(self, on=True); enable_domain_stats(self,
        max_samples); enable_domain_turnover(self, max_samples); enable_epoch_stats(self, P);
        enable_lineage_origins(self, on=True); enable_path_average(self, n_points); enable_spatial_correlation(self,
        max_lag, max_samples); enable_window_stats(self, W); epoch_stats(self, counts=False); epoch_stats_samples(self);
        lineage_origin_rows(self); lineage_origin_windows(self, W, first_window=0, n_windows=None);
        lineage_origins(self, counts=False); lineage_origins_layout(self); lineage_origins_samples(self);
        lineage_origins_scale_exp(self); path_average(self, counts=False); paths(self); reset(self, model, tree,
        paths=None); reset_branch_events(self); reset_change_patterns(self); reset_domain_stats(self);
        reset_domain_turnover(self); reset_epoch_stats(self); reset_lineage_origins(self); reset_path_average(self);
        reset_spatial_correlation(self); reset_window_stats(self); run_mcmc(self, seed, em_iter=0);
        scale_jump_times(self, new_branches); set_leaf_evidence(self, p_state1); set_unobserved(self, mask);
        spatial_correlation(self); spatial_correlation_layout(self); spatial_correlation_part(self);
        spatial_correlation_samples(self); sweeps(self, n, seed, sweep_base=0); window_stats(self, counts=False)
    """,
    "ShardedSampler": """
        accumulate_branch_events(self); accumulate_change_patterns(self); accumulate_domain_stats(self);
        accumulate_domain_turnover(self); accumulate_epoch_stats(self); accumulate_lineage_origins(self);
        accumulate_path_average(self); accumulate_spatial_correlation(self); accumulate_window_stats(self);
        branch_event_windows(self, W); branch_events(self, counts=False); change_pattern_windows(self, W);
        change_patterns(self, counts=False); change_patterns_samples(self); domain_stats(self);
        domain_stats_layout(self); domain_stats_part(self); domain_stats_samples(self); domain_turnover(self);
        domain_turnover_layout(self); domain_turnover_part(self); domain_turnover_samples(self);
        enable_branch_events(self, on=True); enable_change_patterns(self, on=True); enable_domain_stats(self,
        max_samples); enable_domain_turnover(self, max_samples); enable_epoch_stats(self, P);
        enable_lineage_origins(self, on=True); enable_path_average(self, n_points); enable_spatial_correlation(self,
        max_lag, max_samples); enable_window_stats(self, W); epoch_stats(self, counts=False); epoch_stats_samples(self);
        lineage_origin_rows(self); lineage_origin_windows(self, W); lineage_origins(self, counts=False);
        lineage_origins_layout(self); lineage_origins_samples(self); lineage_origins_scale_exp(self); owned_paths(self);
        owned_sites(self); path_average(self, counts=False); refresh_halos(self); reset(self);
        reset_branch_events(self); reset_change_patterns(self); reset_domain_stats(self); reset_domain_turnover(self);
        reset_epoch_stats(self); reset_lineage_origins(self); reset_path_average(self); reset_spatial_correlation(self);
        reset_window_stats(self); run_mcmc(self, burn_in, batch, seed, sweep_base=0); scale_jump_times(self,
        new_branches); set_model(self, model); setup(self, model, tree, fp_own, cuts, capacity=16,
        sweeps_per_refresh=60); spatial_correlation(self); spatial_correlation_layout(self);
        spatial_correlation_part(self); spatial_correlation_samples(self); sweeps(self, n_sweeps, seed, sweep_base=0);
        window_stats(self, counts=False); window_stats_scale_exps(self)
    """,
    "LocalGroup": """
        accumulate_branch_events(self); accumulate_change_patterns(self); accumulate_domain_stats(self);
        accumulate_domain_turnover(self); accumulate_epoch_stats(self); accumulate_lineage_origins(self);
        accumulate_path_average(self); accumulate_spatial_correlation(self); accumulate_window_stats(self); alloc(self,
        nbytes); branch_event_windows(self, W, first_window=0, n_windows=None); branch_events(self, counts=False);
        branch_events_samples(self); capacity(self); change_pattern_windows(self, W, first_window=0, n_windows=None);
        change_patterns(self, counts=False); change_patterns_samples(self); close(self); column_bytes(self);
        counters(self); counts_to_stats(self, counts, batch, average=True); domain_stats(self);
        domain_stats_layout(self); domain_stats_part(self); domain_stats_samples(self); domain_turnover(self);
        domain_turnover_layout(self); domain_turnover_part(self); domain_turnover_samples(self);
        enable_branch_events(self, on=True); enable_change_patterns(self, on=True); enable_domain_stats(self,
        max_samples); enable_domain_turnover(self, max_samples); enable_epoch_stats(self, P);
        enable_lineage_origins(self, on=True); enable_path_average(self, n_points); enable_spatial_correlation(self,
        max_lag, max_samples); enable_window_stats(self, W); epoch_raw(self); epoch_stats(self, counts=False);
        epoch_stats_layout(self); epoch_stats_samples(self); get_columns(self, first, count); halo_phases_left(self);
        kernel_time_ms(self); lineage_origin_rows(self); lineage_origin_windows(self, W, first_window=0,
        n_windows=None); lineage_origins(self, counts=False); lineage_origins_layout(self);
        lineage_origins_samples(self); lineage_origins_scale_exp(self); pack_columns(self, first, count, buf);
        path_average(self, counts=False); path_average_samples(self); paths(self); phase_mode(self); put_columns(self,
        first, count, buf); read(self, buf, offset, count, dtype=<class 'numpy.float64'>); reset(self);
        reset_branch_events(self); reset_change_patterns(self); reset_domain_stats(self); reset_domain_turnover(self);
        reset_epoch_stats(self); reset_lineage_origins(self); reset_path_average(self); reset_spatial_correlation(self);
        reset_window_stats(self); run_mcmc(self, burn_in, batch, seed, sweep_base=0, average=True);
        run_mcmc_counts(self, burn_in, batch, seed, sweep_base=0); scale_jump_times(self, new_branches);
        set_capacity(self, capacity); set_halo(self, left, right); set_model(self, model); set_options(self, **kw);
        set_timing(self, on); set_tree(self, tree); spatial_correlation(self); spatial_correlation_layout(self);
        spatial_correlation_part(self); spatial_correlation_samples(self); sweep(self, n_sweeps, seed, sweep_base=0);
        tri_llh(self); unpack_columns(self, first, count, buf); upload_paths(self, fp, capacity=0, global_site_offset=0,
        n_global=None); window_counts(self, first_window=0, n_windows=None); window_counts_to_stats(self, counts,
        samples); window_stats(self, counts=False); window_stats_samples(self); window_stats_scale_exps(self);
        write(self, buf, offset, arr)
    """,
    "CppSampler": """
        accumulate_domain_stats(self); accumulate_domain_turnover(self); accumulate_lineage_origins(self);
        accumulate_spatial_correlation(self); branch_event_windows(self, W); branch_events(self, counts=False);
        change_pattern_windows(self, W); change_patterns(self, counts=False); close(self); domain_stats(self);
        domain_stats_part(self); domain_turnover(self); domain_turnover_part(self); enable_branch_events(self, on=True);
        enable_change_patterns(self, on=True); enable_domain_stats(self, max_samples); enable_domain_turnover(self,
        max_samples); enable_epoch_stats(self, P); enable_lineage_origins(self, on=True); enable_path_average(self,
        n_points); enable_spatial_correlation(self, max_lag, max_samples); enable_window_stats(self, W);
        epoch_stats(self, counts=False); kernel_time_ms(self); layout(self); lineage_origin_rows(self);
        lineage_origin_windows(self, W); lineage_origins(self, counts=False); lineage_origins_scale_exp(self);
        path_average(self, counts=False); paths(self); phase_mode(self); reset(self, model, tree=None, fp=None,
        n_global=0); reset_domain_stats(self); reset_domain_turnover(self); reset_lineage_origins(self);
        reset_spatial_correlation(self); run_mcmc(self, seed, em_iteration=0); scale_jump_times(self, branches);
        set_leaf_evidence(self, p_state1); set_options(self, reference_proposal_ratio=False, forward_rejection=False,
        sample_root=False); set_timing(self, every); set_unobserved(self, mask); spatial_correlation(self);
        spatial_correlation_part(self); window_stats(self, counts=False)
    """,
}

# the nine summaries in the order of the device's chain, with the nouns of the layers' messages as they were
NOUNS = [("path_average", "a path-average"), ("branch_events", "a branch-event"),
         ("window_stats", "a window-statistics"), ("epoch_stats", "an epoch-statistics"),
         ("lineage_origins", "a lineage-origin"), ("domain_stats", "a domain-statistics"),
         ("change_patterns", "a change-pattern"), ("domain_turnover", "a domain-turnover"),
         ("spatial_correlation", "a spatial-correlation")]


def _classes():
    from epievo_amd.driver import CppSampler
    from epievo_amd.parallel import LocalGroup, ShardedSampler
    from epievo_amd.sampler import DeviceSampler, SingleSiteSampler
    return {c.__name__: c for c in (DeviceSampler, SingleSiteSampler, ShardedSampler, LocalGroup, CppSampler)}


def _recorded(text):
    """"name(p, q=0); ..." -> [(name, [p, q=0])]"""
    out = []
    for item in " ".join(text.split()).split("; "):
        name, params = item.rstrip(")").split("(", 1)
        out.append((name, params.split(", ")))
    return out


@pytest.mark.parametrize("cls", sorted(SURFACE))
def test_public_surface_is_what_it_was(cls):
    c = _classes()[cls]
    recorded = _recorded(SURFACE[cls])
    assert len(recorded) == len({n for n, _ in recorded}) >= 46
    for name, before in recorded:
        fn = getattr(c, name, None)
        assert callable(fn), (cls, name)
        params = list(inspect.signature(fn).parameters.values())
        now = [str(p) for p in params]
        assert now[:len(before)] == before, (cls, name, now)
        if cls == "SingleSiteSampler":     # a forward may take all its target takes: optional arguments only
            assert all(p.default is not inspect.Parameter.empty for p in params[len(before):]), (cls, name, now)
        else:
            assert now == before, (cls, name, now)


def test_summary_table_is_the_chain_and_every_sampler_has_its_methods():
    from epievo_amd.summaries import SUMMARIES
    assert [(s.stem, "%s %s" % (s.article, s.noun)) for s in SUMMARIES] == NOUNS
    classes = _classes()
    for stem, _ in NOUNS:
        for name in ("enable_" + stem, "reset_" + stem, "accumulate_" + stem, stem + "_samples"):
            for cls in ("DeviceSampler", "SingleSiteSampler", "ShardedSampler", "LocalGroup"):
                assert inspect.isfunction(vars(classes[cls]).get(name)), (cls, name)     # in the class's own vars()
        # a forward carries the signature and the docstring of the method it forwards to
        dev, fwd = classes["DeviceSampler"], classes["SingleSiteSampler"]
        for name in ("enable_" + stem, "accumulate_" + stem):
            assert inspect.signature(getattr(fwd, name)) == inspect.signature(getattr(dev, name))
            assert getattr(fwd, name).__doc__ == getattr(dev, name).__doc__ and getattr(dev, name).__doc__
            assert getattr(dev, name).__name__ == getattr(fwd, name).__name__ == name


def test_forwards_resolve_on_the_engine_at_call_time():
    classes = _classes()
    for cls in ("SingleSiteSampler", "ShardedSampler"):
        s = object.__new__(classes[cls])
        s.dev = _Sub({}, 3)
        assert s.enable_spatial_correlation(5, max_samples=9) is None and s.lineage_origins_samples() == 3
        assert s.dev.calls == [("enable_spatial_correlation", (5,), {"max_samples": 9}), ("lineage_origins_samples", (), {})]
    s = object.__new__(classes["SingleSiteSampler"])
    s.dev = _Sub({"branch_event_windows": (np.arange(4, dtype=np.uint64),)}, 3)
    assert s.branch_event_windows(2, 1, n_windows=4)[0] == 3      # the window range reaches the device
    assert s.dev.calls == [("branch_event_windows", (2, 1), {"n_windows": 4})]


def test_abi_table_declares_every_symbol_once():
    from epievo_amd import sampler
    assert len(sampler.ABI_SYMBOLS) == len(set(sampler.ABI_SYMBOLS)) >= 123
    for stem, _ in NOUNS:
        for name in ("epv_set_" + stem, "epv_reset_" + stem, "epv_accumulate_" + stem, "epv_%s_samples" % stem):
            assert name in sampler.ABI_SYMBOLS
    if not os.path.exists(_build.HIP_SO):
        pytest.skip("the HIP library is not built")
    L = sampler.lib()
    undeclared = [n for n in sampler.ABI_SYMBOLS if getattr(L, n).argtypes is None]
    assert not undeclared, undeclared
    import ctypes
    assert L.epv_reset_async.argtypes == [ctypes.c_void_p]
    assert L.epv_copy_columns_async.argtypes == [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                                 ctypes.c_uint64, ctypes.c_int]


# ---- LocalGroup over stand-ins for its shards
N_SITES, CUT, B, N, P, LAG, W = 40, 24, 2, 3, 2, 5, 7       # a three-node tree over 40 sites split 24/16


class _Sub:
    """a shard (or an engine) that answers every read-out with the sample count and the arrays it was given, notes
    every call, and has the sample counts `ns` (one number, or per summary stem)"""
    n_global = N_SITES

    def __init__(self, outs, ns):
        self.outs, self.ns, self.calls = outs, ns, []

    STEM_OF = {"window_counts": "window_stats", "epoch_raw": "epoch_stats", "branch_event_windows": "branch_events",
               "change_pattern_windows": "change_patterns", "lineage_origin_windows": "lineage_origins"}

    def _count(self, name):
        if not isinstance(self.ns, dict):
            return self.ns
        for suffix in ("_samples", "_part"):
            name = name[:-len(suffix)] if name.endswith(suffix) else name
        return self.ns[self.STEM_OF.get(name, name)]

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            if name.endswith("_samples"):
                return self._count(name)
            if name in ("lineage_origins_scale_exp", "epoch_stats_layout"):
                return self.outs[name]
            if name in self.outs:
                return (self._count(name),) + tuple(self.outs[name])
        return call


def _shard_outs(rng, a, b):
    """what a shard that owns the sites [a, b) could hold: random counts of the right shapes and dtypes, and true
    parts of random rows for the three summaries whose parts merge"""
    cnt, nw = b - a, -(-N_SITES // W)
    u32 = lambda *shape: rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    u64 = lambda *shape: rng.integers(0, 2 ** 62, shape, dtype=np.uint64)
    raw = u64(B, P, 32)
    raw[..., 24:] = 0                                      # (no cover terms: any closing rule is met)
    rows = np.array([[1, 0], [1, 1], [2, 0], [2, 2]], np.uint32)
    x = {k: rng.integers(0, 2, (r, N_SITES)).astype(np.uint8)[:, a:b] for k, r in (("d", N), ("t", 2 * B), ("c", N + B))}
    return {
        "path_average": (u32(B, cnt, P),), "branch_events": (u32(6, B, cnt),), "change_patterns": (u32(12 + 2 * B, cnt),),
        "branch_event_windows": (u64(6, B, nw),), "change_pattern_windows": (u64(12 + 2 * B, nw),),
        "window_counts": (rng.integers(-2 ** 62, 2 ** 62, (nw, B, 16)),), "epoch_raw": (raw,),
        "lineage_origins": (rows, u32(4, cnt), u64(2, cnt)), "lineage_origin_windows": (u64(4, nw), u64(2, nw)),
        "lineage_origins_scale_exp": 33, "epoch_stats_layout": (P, np.array([30, 31], np.intc), np.array([5, 9], np.uint64)),
        "domain_stats_part": domains_ref.part(x["d"]), "domain_turnover_part": turnover_ref.part(x["t"]),
        "spatial_correlation_part": corr_ref.part(x["c"], LAG),
    }


@pytest.fixture()
def group():
    from epievo_amd.parallel import LocalGroup
    rng = np.random.default_rng(7)
    g = object.__new__(LocalGroup)
    g.subs = [_Sub(_shard_outs(rng, 0, CUT), {s: 1 for s, _ in NOUNS}),
              _Sub(_shard_outs(rng, CUT, N_SITES), {s: 1 for s, _ in NOUNS})]
    g.pool, g.halo_mode, g._closed = ThreadPoolExecutor(max_workers=2), False, True
    yield g
    g.pool.shutdown(wait=True)


@pytest.mark.parametrize("stem,noun", NOUNS)
def test_group_lifecycle_reaches_every_shard(group, stem, noun):
    args = {"spatial_correlation": (LAG, 4)}.get(stem, (3,))
    assert getattr(group, "enable_" + stem)(*args) is None
    assert getattr(group, "reset_" + stem)() is None
    for s in group.subs:
        s.ns[stem] = 11 + group.subs.index(s)
        assert s.calls == [("enable_" + stem, args, {}), ("reset_" + stem, (), {})]
        del s.calls[:]
    assert getattr(group, stem + "_samples")() == 11              # the first shard's
    if stem == "spatial_correlation":
        assert group._corr_lag == LAG                                   # (run_mcmc_counts reads it)
    # before the first reset() of the group the shards' ranges overlap: no sample
    del group.subs[0].calls[:]
    with pytest.raises(RuntimeError) as e:
        getattr(group, "accumulate_" + stem)()
    assert str(e.value) == "reset() the group before taking %s sample" % noun
    assert not group.subs[0].calls and not group.subs[1].calls
    group.halo_mode = True
    assert getattr(group, "accumulate_" + stem)() is None
    assert all(s.calls == [("accumulate_" + stem, (), {})] for s in group.subs)


def _cat(parts, i, axis=1):
    return np.concatenate([p[i] for p in parts], axis=axis)


# (LocalGroup's read-out, its arguments, the summary, the shards' read-out and the arguments it must get, what the
# group must return after the sample count from the shards' answers without theirs)
READ_OUTS = [
    ("path_average", dict(counts=True), "path_average", "path_average", ((), dict(counts=True)),
     lambda p: (_cat(p, 0),)),
    ("branch_events", dict(counts=True), "branch_events", "branch_events", ((), dict(counts=True)),
     lambda p: (_cat(p, 0, 2),)),
    ("branch_event_windows", dict(W=W), "branch_events", "branch_event_windows", ((W, 0, 6), {}),
     lambda p: (p[0][0] + p[1][0],)),
    ("branch_event_windows", dict(W=W, first_window=2, n_windows=3), "branch_events", "branch_event_windows",
     ((W, 2, 3), {}), lambda p: (p[0][0] + p[1][0],)),
    ("change_patterns", dict(counts=True), "change_patterns", "change_patterns", ((), dict(counts=True)),
     lambda p: (_cat(p, 0),)),
    ("change_pattern_windows", dict(W=W, first_window=1), "change_patterns", "change_pattern_windows", ((W, 1, 5), {}),
     lambda p: (p[0][0] + p[1][0],)),
    ("window_counts", dict(first_window=1, n_windows=2), "window_stats", "window_counts", ((1, 2), {}),
     lambda p: (p[0][0] + p[1][0],)),
    ("window_stats", dict(counts=True), "window_stats", "window_counts", ((0, None), {}),
     lambda p: (p[0][0] + p[1][0],)),
    ("epoch_raw", {}, "epoch_stats", "epoch_raw", ((), {}), lambda p: (host.epoch_raw_add([q[0] for q in p]),)),
    ("epoch_stats", dict(counts=True), "epoch_stats", "epoch_raw", ((), {}),
     lambda p: host.epoch_close(host.epoch_raw_add([q[0] for q in p]), np.array([5, 9], np.uint64))),
    ("lineage_origins", dict(counts=True), "lineage_origins", "lineage_origins", ((), dict(counts=True)),
     lambda p: (p[0][0], _cat(p, 1), _cat(p, 2))),
    ("lineage_origin_windows", dict(W=W), "lineage_origins", "lineage_origin_windows", ((W, 0, 6), {}),
     lambda p: (p[0][0] + p[1][0], p[0][1] + p[1][1])),
    ("domain_stats_part", {}, "domain_stats", "domain_stats_part", ((), {}), lambda p: host.domain_parts_merge(p)),
    ("domain_stats", {}, "domain_stats", "domain_stats_part", ((), {}),
     lambda p: host.domain_part_close(*host.domain_parts_merge(p))),
    ("domain_turnover_part", {}, "domain_turnover", "domain_turnover_part", ((), {}),
     lambda p: host.turnover_parts_merge(p)),
    ("domain_turnover", {}, "domain_turnover", "domain_turnover_part", ((), {}),
     lambda p: host.turnover_part_close(*host.turnover_parts_merge(p))),
    ("spatial_correlation_part", {}, "spatial_correlation", "spatial_correlation_part", ((), {}),
     lambda p: host.corr_parts_merge(p)),
    ("spatial_correlation", {}, "spatial_correlation", "spatial_correlation_part", ((), {}),
     lambda p: host.corr_part_close(*host.corr_parts_merge(p))),
]


def _same(got, want):
    if isinstance(want, (int, np.integer)):
        return got == want
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("case", READ_OUTS, ids=["%s%d" % (c[0], i) for i, c in enumerate(READ_OUTS)])
def test_group_read_out_combines_the_shards(group, case):
    name, kwargs, stem, sub_name, sub_args, combine = case
    noun = dict(NOUNS)[stem].split(" ", 1)[1]
    got = getattr(group, name)(**kwargs)
    want = combine([s.outs[sub_name] for s in group.subs])
    assert got[0] == 1 and len(got) == 1 + len(want)
    assert all(_same(g, w) for g, w in zip(got[1:], want)), name
    for s in group.subs:
        assert (sub_name, sub_args[0], sub_args[1]) in s.calls, s.calls
    # the shards must hold the same number of samples
    group.subs[1].ns[stem] = 2
    with pytest.raises(RuntimeError) as e:
        getattr(group, name)(**kwargs)
    assert str(e.value) == "the shards of the group hold different numbers of %s samples" % noun


def test_group_read_outs_per_sample_and_sums_that_refuse_to_wrap(group):
    for s in group.subs:
        s.ns = 4
    for name, axis in (("path_average", 1), ("branch_events", 2), ("change_patterns", 1)):
        ns, got = getattr(group, name)()
        assert ns == 4 and got.dtype == np.float64
        assert np.array_equal(got, _cat([s.outs[name] for s in group.subs], 0, axis) / 4.0)
    ns, rows, origin, age = group.lineage_origins()
    parts = [s.outs["lineage_origins"] for s in group.subs]
    assert np.array_equal(origin, _cat(parts, 1) / 4.0)
    assert np.array_equal(age, np.ldexp(_cat(parts, 2).astype(np.float64), -33) / 4.0)
    for s in group.subs:                                   # no sample: the zeros as float64, nothing divided
        s.ns = 0
        s.outs["path_average"] = (np.zeros((B, 3, P), np.uint32),)
    ns, got = group.path_average()
    assert ns == 0 and got.dtype == np.float64 and got.shape == (B, 6, P) and not got.any()
    with pytest.raises(ValueError, match="a window holds at least one site"):
        group.lineage_origin_windows(0)
    for s in group.subs:
        s.outs["lineage_origin_windows"] = (np.ones((4, 6), np.uint64), np.full((2, 6), 2 ** 63, np.uint64))
    with pytest.raises(OverflowError, match="64 bits"):
        group.lineage_origin_windows(W)


# ---- ShardedSampler.path_average over stand-ins for the device and the collective
class _Buf:
    def __init__(self, nbytes):
        self.data = np.zeros(nbytes, np.uint8)

    def free(self):
        pass


class _FakeDev:
    """what ShardedSampler asks of its device: this rank's counts, and host-side buffers"""

    def __init__(self, ns, own):
        self.ns, self.own = ns, own

    def path_average(self, counts=False):
        assert counts
        return self.ns, self.own

    def alloc(self, nbytes):
        return _Buf(nbytes)

    def write(self, buf, offset, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf.data[offset:offset + raw.size] = raw

    def read(self, buf, offset, count, dtype=np.float64):
        return buf.data[offset:offset + count * np.dtype(dtype).itemsize].view(dtype).copy()


class _FakeComm:
    """an all-gather among ranks that run one after the other: pieces are remembered by rank"""

    def __init__(self, world, rank, pieces):
        self.world, self.rank, self.pieces, self.collectives = world, rank, pieces, 0

    def all_gather(self, dev, piece, gathered):
        self.collectives += 1
        self.pieces[self.rank] = piece.data.copy()
        k = piece.data.size
        for r, p in self.pieces.items():
            if p.size == k:
                gathered.data[r * k:(r + 1) * k] = p


@pytest.fixture()
def ranks():
    from epievo_amd.parallel import ShardedSampler
    cuts, ns = [0, 5, 12, 16], 2 ** 32 + 5                 # unequal widths: the padding matters; both count words do
    full = np.random.default_rng(3).integers(0, 2 ** 32, (3, 16, 2), dtype=np.uint64).astype(np.uint32)
    assert (full > 2 ** 31).any()
    pieces, out = {}, []
    for r in range(3):
        s = object.__new__(ShardedSampler)
        s.comm, s.cuts = _FakeComm(3, r, pieces), cuts
        s.dev = _FakeDev(ns, full[:, cuts[r]:cuts[r + 1]].copy())
        out.append(s)
    return out, full, ns


def test_sharded_path_average_concatenates_in_genome_order(ranks):
    shards, full, ns = ranks
    for s in shards:                                       # round 0 only fills the pieces: the others' are still missing
        if s is shards[-1]:
            s.path_average(counts=True)
        else:
            with pytest.raises(RuntimeError, match="different numbers"):
                s.path_average(counts=True)
    for r, s in enumerate(shards):
        s.comm.collectives = 0
        got_ns, got = s.path_average(counts=True)
        assert got_ns == ns and got.dtype == np.uint32 and got.shape == full.shape and np.array_equal(got, full)
        assert s.comm.collectives == 1
        # the piece on the wire: [B, widest rank, P] with this rank's sites first, then the sample count in two words
        words = s.comm.pieces[r].view(np.uint32)
        assert words.size == 3 * 7 * 2 + 2 and words[-2:].tolist() == [5, 1]
        padded = words[:-2].reshape(3, 7, 2)
        assert np.array_equal(padded[:, :s.dev.own.shape[1]], s.dev.own) and not padded[:, s.dev.own.shape[1]:].any()
        got_ns, mean = s.path_average()
        assert got_ns == ns and mean.dtype == np.float64 and np.array_equal(mean, full / float(ns))


def test_sharded_path_average_sample_counts_must_agree(ranks):
    shards, full, ns = ranks
    for s in shards:
        try:
            s.path_average(counts=True)
        except RuntimeError:
            pass
    shards[1].dev.ns = ns - 2 ** 32                        # the low word alone would agree
    for s in (shards[1], shards[0]):
        with pytest.raises(RuntimeError) as e:
            s.path_average(counts=True)
        assert str(e.value) == "the ranks hold different numbers of path-average samples"
    shards[1].dev.ns = ns
    shards[1].dev.own = shards[1].dev.own[:, :-1]
    with pytest.raises(RuntimeError, match="this rank counts 6 sites, it owns 7"):
        shards[1].path_average()


def test_sharded_path_average_of_one_rank_makes_no_collective():
    from epievo_amd.parallel import ShardedSampler
    own = np.arange(3 * 16 * 2, dtype=np.uint32).reshape(3, 16, 2)
    s = object.__new__(ShardedSampler)
    s.comm, s.cuts, s.dev = _FakeComm(1, 0, {}), [0, 16], _FakeDev(3, own)
    ns, got = s.path_average(counts=True)
    assert ns == 3 and np.array_equal(got, own) and got.dtype == np.uint32
    assert np.array_equal(s.path_average()[1], own / 3.0)
    assert s.comm.collectives == 0 and not s.comm.pieces
