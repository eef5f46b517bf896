"""The record pool of the second proposal kernel and of the fused phase in its buffers (plan_p2, csrc/epv_plan.h),
without a GPU, through libepv_host.so.

A lane of epv_mh_propose2_kernel runs in a round only when its records fit the wave's pool.  One lane's worst case is
every branch with 2C+1 segments: B (2C+2) Felsenstein records of 2 doubles and B (2C+1) heavy-segment records of
hrec doubles.  A pool below that never lets such a lane run, and the kernel's round loop has no other exit, so the
floor has to hold for every kernel phase_plan can launch in the pool, under every option word -- the options may
change after the pool is planned.  hrec by kernel: 8 in every fused body, 10 in the second kernel when it lists
segments for the segment-parallel jump kernels (jumps == "segments"), 8 in the second kernel otherwise.

The benchmark's shape (tree.nwk, a third of 1e6 sites per context, capacity 16, 0.052 jumps per path, no knob) has
to come out at 8-double records: its launch then takes at most 163840 / 11 bytes of LDS, eleven one-wave blocks per
CU, where 10-double records took 16544 bytes and nine."""
import itertools

import pytest

from common import _tmp, config
from epievo_amd import host

LDS_PER_CU = 163840
STAR8_NWK = "(A:0.1,B:0.2,C:0.05,D:0.3,E:0.15,F:0.1,G:0.2,H:0.05)R:0.0;\n"
# N -> tree
TREES = {2: lambda: config("pair"), 3: lambda: config("cherry"), 5: lambda: config("tree"),
         9: lambda: host.Tree.read(_tmp("star8.nwk", STAR8_NWK)), 15: lambda: config("bal8")}
KBARS = (0.01, 0.3, 2.0)
# capacity 0 asks upload_paths for the smallest it allows, max(16, 2 max + 8), max = the paths' largest jump count:
# taken here as 2, 5 and 12 at the three densities (16, 18 and 32; at 32 a branch has up to 65 segments, beyond the
# fused phase's limit, so that shape is planned without it)
MINIMAL = {0.01: 16, 0.3: 18, 2.0: 32}
CAPS = (0, 1, 16, 31)
SEG_JUMPS = (None, "0", "1")
# every option bit phase_plan reads (reference ratio 1, forward rejection 2, sampled root 4, direct sampler 8, its
# fused bodies 16, leaf fast 32), with and without held leaf cells
OPTION_WORDS = tuple(range(64))
HELD = ((0, 0), (3, 0), (0, 2), (3, 2))
N_SITES = 333334


def floor(B, C, hrec):
    return 2 * B * (2 * C + 2) + hrec * B * (2 * C + 1)


def hrec_of(plan):
    """doubles per heavy-segment record of the proposal kernel a plan launches; None where it has no LDS pool of
    this kind (first and third kernel)"""
    if plan["propose"] == "fused":
        return 8
    if plan["propose"] == "V2":
        return 10 if plan["jumps"] == "segments" else 8
    return None


def test_benchmark_shape_fits_eleven_blocks():
    plan, p2 = host.phase_plan_p2(config("tree"), N_SITES, 16, 0.052)
    print("plan", plan, "p2", p2)
    assert plan["propose"] == "fused" and plan["small_nn"] == 5 and plan["fused_lanes"] == 64
    assert p2["planned"] and p2["fused"]
    assert p2["lds"] <= LDS_PER_CU // 11, p2            # 14 894 B; 16 544 B with 10-double records
    assert p2["pool"] >= floor(4, 16, 8)


@pytest.mark.parametrize("N", sorted(TREES))
def test_pool_holds_one_lanes_worst_case_of_every_reachable_kernel(N):
    tree = TREES[N]()
    assert tree.n_nodes == N
    B = N - 1
    seen = set()
    for C0, kbar, sj in itertools.product(CAPS, KBARS, SEG_JUMPS):
        C = C0 or MINIMAL[kbar]
        for extra in ({}, {"EPV_FORCE_LDS_POOL": "1"}, {"EPV_FUSED_PHASE": "0"}, {"EPV_FUSED_PHASE": "1"},
                      {"EPV_P2_SMALL_TREE": "0"}):
            knobs = dict(extra) if sj is None else dict(extra, EPV_SEG_JUMPS=sj)
            for opt, (unobs, evid) in itertools.product(OPTION_WORDS, HELD):
                plan, p2 = host.phase_plan_p2(tree, N_SITES, C, kbar, opt, unobs, evid, knobs)
                h = hrec_of(plan)
                if h is None:
                    continue
                assert p2["planned"], (C, kbar, knobs, opt, plan)
                seen.add((plan["propose"], h))
                assert p2["pool"] >= floor(B, C, h), (C, kbar, knobs, opt, unobs, evid, plan, p2, floor(B, C, h))
                assert p2["pool"] * 8 < p2["lds"] <= LDS_PER_CU
    # the grid reaches the fused bodies, the second kernel with 10-double records and with 8
    if N <= 9:
        assert ("fused", 8) in seen and ("V2", 10) in seen and ("V2", 8) in seen, seen
