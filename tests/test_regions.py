"""Genomic regions without a GPU: the two formulations of the chain agree on the CPU, the
host functions, the slices a group hands its shards, the symbols, and the plans the GPU rows expect."""
import ctypes
import os
import re

import numpy as np
import pytest

import orc
import regions_ref as rr
from common import ref_test_model
from epievo_amd import _build, host
from test_kernel_matrix import make_tree

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(tree="tree", n=rr.N_SITES):
    model, t = ref_test_model(), make_tree(tree)
    fp = host.simulate(model, t, n, 6)
    return model, t, fp, int(max(16, 2 * fp.counts().max() + 8))


# ---- fixed ends == independent regions, on the CPU
@pytest.mark.parametrize("opts", [{}, {"forward_rejection": True}, {"sample_root": True}], ids=["default", "fr", "sr"])
@pytest.mark.parametrize("layout", [rr.LAYOUT_A, rr.LAYOUT_B], ids=["A", "B"])
def test_regions_alone_are_the_whole_genome_stepped_over_the_free_sites(layout, opts):
    model, tree, fp, cap = _inputs()
    ref = rr.RegionsRef(tree, model, fp, layout, cap, 19, opts)
    nacc = sum(ref.sweep(w) for w in range(4, 9))
    whole, nacc_whole = rr.whole_genome_paths(tree, model, fp, layout, cap, 19, 5, 4, opts)
    assert nacc == nacc_whole > 0
    assert orc.paths_equal(ref.paths(), whole)
    # the end sites of every region are what they were, the inner sites moved
    mask = host.region_fixed_mask(fp.n_sites, layout)
    for s in np.nonzero(mask)[0]:
        assert orc.paths_equal(whole.slice_sites(int(s), int(s) + 1), fp.slice_sites(int(s), int(s) + 1))
    assert not orc.paths_equal(whole, fp)


def test_layouts_put_the_breaks_where_the_kernels_have_edges():
    for layout in (rr.LAYOUT_A, rr.LAYOUT_B):
        assert sum(layout) == rr.N_SITES and min(layout) == 3
    a, b = (set(np.nonzero(host.region_fixed_mask(rr.N_SITES, l))[0]) for l in (rr.LAYOUT_A, rr.LAYOUT_B))
    assert {63, 64, 127, 128, 192, 193, 255, 256} <= a           # breaks on wave edges (64, 128, 256), one past one (193)
    assert {255, 256} <= a and {256, 257} <= b                   # both sides of the 256-site block edge
    assert {s % 3 for s in a} == {s % 3 for s in b} == {0, 1, 2}
    assert rr.LAYOUT_A.count(3) == 2 and rr.LAYOUT_B.count(3) == 1


# ---- host functions
def test_fixed_mask_of_regions():
    m = host.region_fixed_mask(10, [3, 4, 3])
    assert m.dtype == np.uint8 and m.tolist() == [1, 0, 1, 1, 0, 0, 1, 1, 0, 1]
    # a 3-site region: two fixed sites next to the neighbours', one site that is updated
    assert host.region_fixed_mask(3, [3]).tolist() == [1, 0, 1]
    with pytest.raises(ValueError, match="region 1 holds 2 sites, a region holds at least 3"):
        host.region_fixed_mask(5, [3, 2])
    with pytest.raises(ValueError, match="hold 7 sites in all, the paths hold 8"):
        host.region_fixed_mask(8, [3, 4])


def test_read_regions(tmp_path):
    f = tmp_path / "genome.sizes"
    f.write_text("# chrom.sizes\nchr1\t5\n\nchr2  3\n#gap\nchr3 4\n")
    assert host.read_regions(str(f), 12) == [5, 3, 4]
    for text, n, line, what in [
            ("chr1 5\nchr2\n", 8, 2, "found 1 fields"),
            ("chr1 5 x\n", 5, 1, "found 3 fields"),
            ("chr1 5\nchr2 three\n", 8, 2, "not an integer: three"),
            ("chr1 5\n# c\nchr2 2\n", 7, 3, "region chr2 holds 2 sites, a region holds at least 3"),
            ("chr1 5\nchr2 -4\n", 9, 2, "holds -4 sites"),
            ("chr1 5\nchr2 4\n", 8, 2, "the regions up to chr2 hold 9 sites, the paths hold 8"),
            ("chr1 5\nchr2 4\n", 10, 2, "the regions hold 9 sites in all, the paths hold 10"),
            ("# nothing\n", 10, 0, "the regions hold 0 sites in all")]:
        f.write_text(text)
        with pytest.raises(ValueError) as e:
            host.read_regions(str(f), n)
        assert "line %d:" % line in str(e.value) and what in str(e.value), str(e.value)


# ---- the slices a group hands its shards, over stand-ins for them
class _Sub:
    def __init__(self):
        self.calls = []

    def set_fixed_sites(self, mask):
        self.calls.append(None if mask is None else np.array(mask, np.uint8))

    def fixed_sites(self):
        return 0 if not self.calls or self.calls[-1] is None else int(self.calls[-1].sum())


def _group(n, lo, hi, g0=0, n_global=None):
    from epievo_amd.parallel import LocalGroup
    g = object.__new__(LocalGroup)
    g.subs = [_Sub() for _ in lo]
    g.lo, g.hi, g.n_sites = lo, hi, n
    g._g0, g._n_global = g0, n if n_global is None else n_global
    return g


def test_group_hands_every_shard_its_slice_halos_included():
    n, H = 40, 4
    g = _group(n, [0, 12 - H, 28 - H], [12 + H, 28 + H, n])       # three shards cut at 12 and 28, 4 halo columns
    lengths = [11, 3, 15, 11]                                      # breaks at 11 (cut - 1), 14 (halo), 29 (cut + 1)
    whole = host.region_fixed_mask(n, lengths)
    g.set_regions(lengths)
    for j, s in enumerate(g.subs):
        assert len(s.calls) == 1 and np.array_equal(s.calls[0], whole[g.lo[j]:g.hi[j]])
    # a halo column that its owner holds fixed is held fixed in the neighbour's copy
    assert g.subs[0].calls[0][13] == 1 and g.subs[1].calls[0][13 - 8] == 1 and g.subs[1].calls[0][10 - 8] == 1
    assert g.fixed_sites() == sum(int(whole[a:b].sum()) for a, b in zip(g.lo, g.hi))
    g.set_regions(None)
    assert all(s.calls[-1] is None for s in g.subs)
    with pytest.raises(ValueError, match="40 sites"):
        g.set_fixed_sites(np.zeros(39))
    # a group that is itself a shard of a longer genome takes its window of the genome's mask
    g = _group(n, [0, 20 - H], [20 + H, n], g0=100, n_global=200)
    g.set_regions([110, 90])
    whole = host.region_fixed_mask(200, [110, 90])[100:140]
    assert whole.tolist().count(1) == 2 and np.array_equal(g.subs[0].calls[0], whole[:24])
    assert np.array_equal(g.subs[1].calls[0], whole[16:])
    # one shard: the whole mask
    g = _group(n, [0], [n])
    g.set_regions([20, 20])
    assert np.array_equal(g.subs[0].calls[0], host.region_fixed_mask(n, [20, 20]))


def test_sharded_sampler_hands_its_engine_the_window_and_counts_the_free_sites():
    from epievo_amd.parallel import ShardedSampler
    s = object.__new__(ShardedSampler)
    s.dev, s.n_global, s.g0, s.n_loc = _Sub(), 100, 30, 50
    s.set_regions([40, 3, 57])
    whole = host.region_fixed_mask(100, [40, 3, 57])
    assert np.array_equal(s.dev.calls[0], whole[30:80]) and s._n_fixed == 4        # (the genome's ends do not count)
    s.set_regions(None)
    assert s.dev.calls[-1] is None and s._n_fixed == 0


def test_single_site_sampler_keeps_regions_across_resets():
    from epievo_amd.sampler import SingleSiteSampler

    class Dev(_Sub):
        n_sites = 0

        def set_tree(self, t): pass
        def set_model(self, m): pass
        def reset(self): pass
        def set_options(self, **kw): pass

        def upload_paths(self, fp, cap):
            self.n_sites = fp.n_sites
            self.calls.append("upload")

        def run_mcmc(self, burn_in, batch, seed, base):
            return np.zeros(8), np.zeros(8), 12
    model, tree, fp, cap = _inputs("pair", 10)
    s = object.__new__(SingleSiteSampler)
    s.__dict__.update(burn_in=1, batch=2, capacity=cap, dev=Dev(), _uploaded=False, _unobserved=None, _leaf_evidence=None,
                      _regions=None, SAMPLE_ROOT=False, direct_sampler=False, direct_fused=False, leaf_fast=False)
    s._apply_sample_root = lambda: None
    s.set_regions([3, 7])                 # before paths: kept
    assert s.dev.calls == []
    s.reset(model, tree, fp)
    assert s.dev.calls[0] == "upload" and s.dev.calls[1].tolist() == [1, 0, 1, 1, 0, 0, 0, 0, 0, 1]
    s.reset(model, tree, fp)              # new paths: applied again
    assert s.dev.calls[2] == "upload" and np.array_equal(s.dev.calls[3], s.dev.calls[1])
    # the acceptance rate is over the sites that can be updated: 8 interior sites, 2 of them fixed... as the device says
    s.dev.fixed_sites = lambda: 2
    assert s.run_mcmc(1)[2] == 12 / float(2 * (10 - 2 - 2))
    s.set_regions(None)
    assert s.dev.calls[-1] is None and s.run_mcmc(1)[2] == 12 / float(2 * 8)


# ---- symbols
def test_header_table_and_library_agree_on_the_new_symbols():
    from epievo_amd.sampler import ABI, ABI_SYMBOLS
    header = open(os.path.join(_ROOT, "include", "epievo_mi355x.h")).read()
    assert re.search(r"int epv_set_fixed_sites\(epv_ctx \*ctx, const uint8_t \*mask[^)]*\);", header)
    assert re.search(r"int epv_fixed_sites\(epv_ctx \*ctx, uint64_t \*n_fixed_updatable\);", header)
    u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    assert ABI["epv_set_fixed_sites"] == ([ctypes.c_void_p, u8p], ctypes.c_int)
    assert ABI["epv_fixed_sites"] == ([ctypes.c_void_p, u64p], ctypes.c_int)
    assert ABI_SYMBOLS.count("epv_set_fixed_sites") == ABI_SYMBOLS.count("epv_fixed_sites") == 1
    if not os.path.exists(_build.HIP_SO):
        pytest.skip("the HIP library is not built")
    L = ctypes.CDLL(_build.HIP_SO)
    assert hasattr(L, "epv_set_fixed_sites") and hasattr(L, "epv_fixed_sites")


# ---- the plans the GPU rows expect (tests/test_regions_gpu.py), from the planner without a GPU: fixed sites are no input
# of the plan, so a row's family is the one its knobs and options select on any context
def test_gpu_rows_name_the_plan_their_knobs_select():
    from regions_gpu_child import leaf_mask
    from test_regions_gpu import ROWS
    assert len({r[0] for r in ROWS}) == len(ROWS) == 13
    for rid, tree, env, more, expect in ROWS:
        model, t, fp, cap = _inputs(tree)
        kbar = fp.counts().sum() / (fp.n_sites * (t.n_nodes - 1))
        opts = more.get("opts", {})
        options = (1 if opts.get("reference_proposal_ratio") else 0) | (2 if opts.get("forward_rejection") else 0) | \
            (4 if opts.get("sample_root") else 0) | (8 if more.get("direct") else 0) | \
            (16 if more.get("direct_fused") else 0) | (32 if more.get("leaf_fast") else 0)
        unobs = int(leaf_mask(t, fp.n_sites).sum()) if more.get("leaf") else 0
        plan = host.phase_plan(t, fp.n_sites, cap, kbar, options, unobs, 0, knobs=env)
        bad = dict((k, (v, plan[k])) for k, v in expect.items() if plan[k] != v)
        assert not bad, (rid, bad, plan)
        if rid == "direct":
            assert plan["propose"] != "fused"
