"""Genomic regions on the GPU (epv_set_fixed_sites): the first and the last site of every
region are held fixed by guards around the colour-phase kernels, and their triples are taken off the integer
statistics.  Every case runs in a fresh process (tests/regions_gpu_child.py) with its EPV_* knobs in the environment.

n = 600 in two layouts.  Together they put a break on a 64-site wave edge (A: a region starts at 64, 128 and 256), one
site either side of one (A: 193, B: 257 start a region; the last sites 63, 127, 255 sit before one), on both sides of
the statistics kernels' 256-site block edge (A: 255 | 256, B: 256 | 257, 259 | 260), they hold 3-site regions with ONE
site that is updated (A: two, B: one), and their fixed sites fall on all three colours.

The rows, one per kernel family, compare run_mcmc_counts(2, 3) bit for bit with tests/regions_ref.py (every region
alone through the oracle's rung B): the paths, the integer J and D of every batch sweep, the accept count, and the
cached triple likelihoods of the non-fixed sites; the plan is asserted to be the family the row names.  The oracle has
no direct sampler: the two direct rows compare with every region run alone on the device under an update range
(regions_gpu_child.device_regions_ref)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import regions_ref as rr

_TESTS = os.path.dirname(os.path.abspath(__file__))

_SEP = {"EPV_FUSED_PHASE": "0"}
_L64 = {"EPV_FUSED_PHASE": "1", "EPV_FUSED_LANES": "64"}


def fused(nn, lanes=16):
    return dict(propose="fused", small_nn=nn, jumps="fused", accept="fused", fused_lanes=lanes)


# (id, tree, environment, spec entries, expected plan fields)
ROWS = [
    ("fused-small-tree", "tree", {}, {}, fused(5)),
    ("fused-generic", "star5", {}, {}, fused(0)),
    ("fused-lanes64", "tree", _L64, {}, fused(5, 64)),
    ("v2-lds", "tree", dict(_SEP, EPV_SEG_JUMPS="0"), {}, dict(propose="V2", gpool=False, listed=True)),
    ("v1-lds", "tree", dict(_SEP, EPV_PROPOSE_V1="1"), {}, dict(propose="V1", gpool=False, accept="accept_cache")),
    ("v1-global", "tree", dict(_SEP, EPV_PROPOSE_V1="1", EPV_FORCE_GLOBAL_POOL="1"), {},
     dict(propose="V1", gpool=True, accept="accept_cache")),
    ("v3-bal16", "bal16", dict(_SEP, EPV_PROPOSE_V3="1"), {}, dict(propose="V3", accept="accept3", listed=True)),
    ("forward-rejection", "tree", {}, dict(opts={"forward_rejection": True}), fused(5)),
    ("direct", "tree", {}, dict(direct=True), dict(direct=True)),
    ("direct-fused", "tree", {}, dict(direct=True, direct_fused=True), dict(direct=True, propose="fused", small_nn=5)),
    ("leaf-mask", "tree", {}, dict(leaf=True), dict(propose="V1", unobs=True)),
    ("leaf-mask-fast", "tree", {}, dict(leaf=True, leaf_fast=True), dict(propose="fused", small_nn=5, unobs=True)),
    ("sample-root", "tree", {}, dict(opts={"sample_root": True}), dict(propose="V1", refq=True)),
]
LAYOUTS = [("A", rr.LAYOUT_A), ("B", rr.LAYOUT_B)]


def child(spec, env=None, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(_TESTS, "regions_gpu_child.py"), json.dumps(spec)],
                       env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stderr[-3000:]
    return json.loads(r.stdout[3:])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [l[1] for l in LAYOUTS], ids=[l[0] for l in LAYOUTS])
@pytest.mark.parametrize("tree,env,more,expect", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_regions_equal_the_regions_run_alone(tree, env, more, expect, layout):
    out = child(dict(kind="row", tree=tree, layout=layout, expect=expect, **more), env)
    if more.get("direct") and not more.get("direct_fused"):
        assert out["plan"]["propose"] != "fused"
    assert out["nacc"] > 0


@pytest.mark.gpu
def test_no_mask_and_an_empty_mask_are_the_context_without_one():
    assert child(dict(kind="default"))["launches"] == 15


@pytest.mark.gpu
def test_a_region_does_not_see_another_regions_data():
    child(dict(kind="decoupling", layout=rr.LAYOUT_A, region=2))


@pytest.mark.gpu
def test_the_mask_outlives_overflow_regrow_rescaling_and_reset():
    child(dict(kind="lifetime", layout=rr.LAYOUT_A))


# LocalGroup(shards = 3) takes three shards from 3 * 1536 sites (tests/test_local_group.py) and cuts them at 1536 and
# 3072, with 512 halo columns either side of a cut.  Breaks on a cut, one site before it, one site after it, and
# inside the halos on both sides of a cut; a 3-site region across a cut
GROUP_N = 4608
GROUP_LAYOUTS = [
    ("on-cut", [1200, 336, 264, 1271, 1537]),                  # 1200 (halo), 1536 (cut), 1800 (halo), 3071 (cut - 1)
    ("beside-cut", [1535, 3, 1535, 435, 1100]),                # 1535 (cut - 1), 1538, 3073 (cut + 1), 3508 (halo)
    ("after-cut", [1537, 1000, 2071]),                         # 1537 (cut + 1), 2537
]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [l[1] for l in GROUP_LAYOUTS], ids=[l[0] for l in GROUP_LAYOUTS])
def test_three_shards_equal_the_single_context(layout):
    assert sum(layout) == GROUP_N
    child(dict(kind="group", n=GROUP_N, layout=layout, cuts=[1536, 3072]))


@pytest.mark.gpu
def test_cpp_driver_over_two_contexts_equals_the_single_context():
    # (two contexts from 32768 sites on, cut at 16384: a 3-site region across the cut, a break inside the halo)
    child(dict(kind="cpp", n=40000, layout=[16383, 3, 100, 23514]), {"EPV_DEVICES": "0,0"})


@pytest.mark.gpu
def test_programs_take_a_regions_file(tmp_path):
    child(dict(kind="cli", layout=rr.LAYOUT_A, tmp=str(tmp_path)))


@pytest.mark.gpu
def test_the_seven_spanning_layers_and_fixed_sites_refuse_each_other():
    assert child(dict(kind="refusing", layout=rr.LAYOUT_A))["layers"] == 7


@pytest.mark.gpu
def test_the_five_per_site_layers_work_under_regions():
    child(dict(kind="layers", layout=rr.LAYOUT_A))
