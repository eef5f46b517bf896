"""The fused colour phase at 32 and 64 sites per wave (and once at 8), the launch tails of every colour-phase
path, update ranges and the halo mode, each against the oracle's parallel rung B, bit for bit.

A context chooses the sites per wave of its fused phase from its size (plan_p2 in epv_plan.h: 16 up to a
phase capacity of 32768 sites, 32 up to 65536, 64 above; phase capacity = (n + 2) // 3 + 1), so every other
parity test of the suite, none above n = 40000, runs 16 sites per wave.  Here EPV_FUSED_LANES sets the width on
genomes of a few hundred sites, whose per-colour site counts are chosen around one wave:

  n = 3, 4, 5    one to three interior sites: one, two, three colours with a single site
  n = 3L + 1     the colours have L - 1, L and L sites: one wave whose last lane is invalid
  n = 3L + 2     every colour is exactly one full wave
  n = 3L + 3     the launch has two waves; one colour has L + 1 sites (a second wave with one valid lane), the
                 other two have L (a second wave with no valid lane at all)
  n = 6L + 4     2L + 1, 2L + 1 and 2L sites

Each row runs in a fresh process with its knobs in the environment (a context reads them when it is created),
asserts the plan after reset() -- the proposal kernel, the small-tree body and fused_lanes -- and then compares
with rung B: the cached triple likelihoods after reset(), the accept count, paths and likelihoods after each of
four single sweeps (thirty at n <= 5), then J, D, the accept count and the overflow counter of run_mcmc(1, 2).
One process handles all lengths of a row.

  TAILS      the lengths above at 32 and 64 sites per wave: pair (NN = 2), tree (NN = 5), star5 (generic body),
             pair and tree again under forward rejection; one row at 8 sites per wave
  OVERFLOW   n = 6L + 4 at the input's own maximum as capacity: the overflow decisions are the oracle's
  RANGES     epv_set_update_range at n = 9L + 5: ranges that start at sites 1 .. 4 (all three colours, and the
             genome's first interior site), of 1, 2, 3, 3L and 3L + 1 sites, and one that ends at n - 2; the
             oracle is driven site by site in colour order, columns outside the range keep the input
  HALO       two contexts on one GPU (LocalGroup) at n = 3100 against one unsharded oracle: reset(), run_mcmc and
             twice 60 sweeps (a halo of 512 columns lasts 85, so the second call refreshes the internal halos)
  DEFAULT    no knob: the four lengths around the two thresholds of plan_p2, the only naturally chosen 32- and
             64-lane runs small enough for the oracle, at capacity 31 (the largest the fused phase takes)
  SEPARATE   the same tails through the separate kernels (EPV_FUSED_PHASE=0): V2 with and without segment
             jumps, V1 and V3, around one full block of each kernel's width

The CPU test beside them checks the tables' arithmetic and, on the oracle alone, that no row is vacuous: the
seeds are chosen so that the oracle's chain accepts a proposal and leaves the input on every length."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
from common import config, ref_test_model
from epievo_amd import host

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))

WIDTHS = (32, 64)
SIM_SEED = 6
TINY = (3, 4, 5)
# (label, n, lanes of a launch over the whole genome, sites per colour in ascending order), each from the width
SHAPES = [
    ("last-lane-invalid", lambda L: 3 * L + 1, lambda L: L, lambda L: [L - 1, L, L]),
    ("full-wave", lambda L: 3 * L + 2, lambda L: L, lambda L: [L, L, L]),
    ("one-lane-and-empty-wave", lambda L: 3 * L + 3, lambda L: L + 1, lambda L: [L, L, L + 1]),
    ("two-waves", lambda L: 6 * L + 4, lambda L: 2 * L + 1, lambda L: [2 * L, 2 * L + 1, 2 * L + 1]),
]
TINY_COUNTS = {3: [0, 0, 1], 4: [0, 1, 1], 5: [1, 1, 1]}


def threads(n):
    """lanes of a colour phase over the whole genome: ceil((n - 2) / 3), as launch_phase counts them"""
    return -(-(n - 2) // 3)


def colour_counts(n):
    """interior sites 1 .. n - 2 per colour (site % 3), ascending"""
    return sorted(len(range(c or 3, n - 1, 3)) for c in range(3))


def tail_lengths(L):
    return list(TINY) + [s[1](L) for s in SHAPES]


def block_lengths(width):
    """the three lengths around one full block of `width` lanes"""
    return [s[1](width) for s in SHAPES[:3]]


def sweeps_for(n):
    return 30 if n <= 5 else 4


def fused(nn, lanes):
    return dict(propose="fused", small_nn=nn, jumps="fused", accept="fused", gpool=False, listed=False,
                fused_lanes=lanes)


def lanes_env(L):
    return {"EPV_FUSED_PHASE": "1", "EPV_FUSED_LANES": str(L)}


FR = {"forward_rejection": True}
_SEP = {"EPV_FUSED_PHASE": "0"}

# (id, tree, nodes, lengths, env, options, expected plan fields, seed of the chain).  The seeds are chosen on the
# oracle (test_no_tail_row_is_vacuous): with most seeds the single interior site of n = 3 ends thirty sweeps on the
# path it started with
TAILS = []
for _L in WIDTHS:
    TAILS += [
        ("pair-%d" % _L, "pair", 2, tail_lengths(_L), lanes_env(_L), {}, fused(2, _L), 14),
        ("tree-%d" % _L, "tree", 5, tail_lengths(_L), lanes_env(_L), {}, fused(5, _L), 64),
        # (six nodes on a few hundred sites: whether the record pool "typically" fits LDS, and with it the plan,
        # turns on the sample's mean jump count -- n = 196 goes to the large-tree kernel -- so the pool is forced)
        ("star5-%d" % _L, "star5", 6, tail_lengths(_L), dict(lanes_env(_L), EPV_FORCE_LDS_POOL="1"), {}, fused(0, _L), 21),
        ("fr-pair-%d" % _L, "pair", 2, tail_lengths(_L), lanes_env(_L), FR, fused(2, _L), 14),
        ("fr-tree-%d" % _L, "tree", 5, tail_lengths(_L), lanes_env(_L), FR, fused(5, _L), 64),
    ]
# a width the library accepts and nothing else runs: 27 sites are 9, 8 and 8 of a colour
TAILS.append(("tree-8", "tree", 5, [27], lanes_env(8), {}, fused(5, 8), 19))

# the separate kernels, around one full block of their launches.  Block widths (launch_propose and
# launch_accept in epv_abi.hip): the second proposal kernel 64 lanes; the first one PlanV1's threads, 64; both followed by
# epv_mh_accept_kernel in blocks of 256.  The large-tree kernel 256 lanes, followed by epv_mh_accept3_kernel in
# blocks of 256 lanes = 84 sites (three lanes a site, 21 sites a wave)
_V2 = dict(propose="V2", gpool=False, accept="accept_cache", listed=True, small_nn=0, p3_words=0, fused_lanes=0)
_LEN_64 = list(TINY) + block_lengths(64) + block_lengths(256)
_LEN_256 = list(TINY) + block_lengths(84) + block_lengths(256)
SEPARATE = [
    ("v2-jumps", "tree", 5, _LEN_64, dict(_SEP, EPV_SEG_JUMPS="0"), {}, dict(_V2, jumps="jumps_all"), 64),
    ("v2-segments", "tree", 5, _LEN_64, dict(_SEP, EPV_SEG_JUMPS="1"), {}, dict(_V2, jumps="segments"), 64),
    ("v1", "tree", 5, _LEN_64, dict(_SEP, EPV_PROPOSE_V1="1"), {},
     dict(propose="V1", gpool=False, refq=False, jumps="jumps_all", accept="accept_cache", listed=False, p3_words=0,
          fused_lanes=0), 64),
    ("v3", "bal16", 31, _LEN_256, dict(_SEP, EPV_PROPOSE_V3="1"), {},
     dict(propose="V3", p3_words=1, p3_slab_pool=False, jumps="jumps_all", accept="accept3", listed=True, gpool=False,
          fused_lanes=0), 7),
]

# (id, tree, nodes, n, env, expected plan fields, seed): the capacity is the input's own maximum, three sweeps
OVERFLOW = [("overflow-%s-%d" % (t, L), t, nn, 6 * L + 4, lanes_env(L), fused(nn, L), 15)
            for L in WIDTHS for t, nn in (("tree", 5), ("pair", 2))]

RANGE_SWEEPS = 4


def update_ranges(L):
    n = 9 * L + 5
    out = [(first, first + length - 1) for first in (1, 2, 3, 4) for length in (1, 2, 3, 3 * L, 3 * L + 1)]
    return n, out + [(n - 2 - 3 * L, n - 2)]


# (id, tree, nodes, width, env, expected plan fields, seed)
RANGES = [("ranges-%s-%d" % (t, L), t, nn, L, lanes_env(L), fused(nn, L), 19)
          for L in WIDTHS for t, nn in (("tree", 5), ("pair", 2))]

HALO_N, HALO_SEED, HALO_SWEEPS = 3100, 31, 60       # (two contexts need 3072 sites)
HALO = [("halo-%d" % L, L) for L in WIDTHS]


def phase_cap(n):
    return (n + 2) // 3 + 1


def last_n_with(cap):
    return 3 * (cap - 1)


def first_n_with(cap):
    return 3 * (cap - 1) - 2


FUSED_CAP = 31
# (id, n, sites per wave, compared with the oracle)
DEFAULT = [
    ("cap-32768", last_n_with(32768), 16, False),
    ("cap-32769", first_n_with(32769), 32, True),
    ("cap-65536", last_n_with(65536), 32, True),
    ("cap-65537", first_n_with(65537), 64, True),
]


# ---- shared by the child processes and the CPU test
def make_input(tree_name, n):
    model, tree = ref_test_model(), config(tree_name)
    return model, tree, host.simulate(model, tree, n, SIM_SEED)


def roomy(fp):
    return int(max(16, 2 * fp.counts().max() + 8))


def oracle(tree, model, fp, cap, seed, opts):
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    o.set_sampler(bool(opts.get("forward_rejection")))
    o.reset()
    return o


def oracle_range_sweep(o, first, last, w):
    """one sweep over [first, last] in the device's order: colour by colour, every site of the colour"""
    return sum(o.mh_site(s, w) for c in range(3) for s in range(first, last + 1) if s % 3 == c)


def columns_equal(a, b, lo, hi):
    return lo >= hi or orc.paths_equal(a.slice_sites(lo, hi), b.slice_sites(lo, hi))


_HEAD = r'''
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import orc
import test_fused_lanes as fl
from epievo_amd.sampler import DeviceSampler
spec = json.loads(%(spec)r)
opts, expect, seed = spec.get("opts", {}), spec.get("expect", {}), spec.get("seed", 0)

def device(tree, model, fp, cap, rng=None):
    d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap); d.set_options(**opts)
    if rng:
        d.set_update_range(*rng)
    d.reset()
    return d

def check_plan(d, n):
    plan = d.phase_plan()
    print("plan", n, json.dumps(plan), flush=True)
    bad = dict((k, (v, plan[k])) for k, v in expect.items() if plan[k] != v)
    assert not bad, "n = %%d: plan differs (expected, got): %%r; plan %%r" %% (n, bad, plan)
    return plan

def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))
'''

# every length of a row against rung B: likelihoods after reset(), single sweeps, run_mcmc
_PARITY = _HEAD + r'''
for n in spec["lengths"]:
    model, tree, fp = fl.make_input(spec["tree"], n)
    assert tree.n_nodes == spec["nodes"], tree.n_nodes
    cap = fl.roomy(fp)
    d = device(tree, model, fp, cap)
    plan = check_plan(d, n)
    o = fl.oracle(tree, model, fp, cap, seed, opts)
    assert same_bits(d.tri_llh(), o.tri_llh()), (n, "likelihoods after reset()")
    W, total = fl.sweeps_for(n), 0
    for w in range(W):
        nd, no = d.sweep(1, seed, sweep_base=w), o.sweep(w)
        assert nd == no, (n, w, nd, no)
        assert orc.paths_equal(d.paths(), o.paths()), (n, w, "paths")
        assert same_bits(d.tri_llh(), o.tri_llh()), (n, w, "likelihoods")
        total += nd
    Jd, Dd, nd = d.run_mcmc(1, 2, seed, sweep_base=W)
    Jo, Do, no, _ = o.run_mcmc(1, 2, sweep_base=W)
    assert nd == no, (n, nd, no)
    assert np.array_equal(Jd, Jo) and np.array_equal(Dd, Do), (n, "J, D")
    assert orc.paths_equal(d.paths(), o.paths()) and same_bits(d.tri_llh(), o.tri_llh()), (n, "after run_mcmc")
    assert d.counters()["overflow"] == o.counters()["overflow"], (n, d.counters(), o.counters())
    assert d.phase_plan() == plan
    print("length", n, "accepted", total, "+", nd, flush=True)
    d.close()
print("ok")
'''

# a capacity that overflows: the overflow decisions must be the sequential sampler's too
_OVERFLOW = _HEAD + r'''
n = spec["n"]
model, tree, fp = fl.make_input(spec["tree"], n)
cap = int(fp.counts().max())
d = device(tree, model, fp, cap)
check_plan(d, n)
o = fl.oracle(tree, model, fp, cap, seed, opts)
assert same_bits(d.tri_llh(), o.tri_llh())
for w in range(3):
    try:
        d.sweep(1, seed, sweep_base=w)
    except Exception as e:
        assert "rejected" in str(e) or "capacity" in str(e).lower(), e
    o.sweep(w)
    assert orc.paths_equal(d.paths(), o.paths()), "paths differ after overflow sweep %%d" %% w
    assert same_bits(d.tri_llh(), o.tri_llh()), w
print("overflow", d.counters()["overflow"], o.counters()["overflow"], flush=True)
assert d.counters()["overflow"] == o.counters()["overflow"] > 0
d.close()
print("ok")
'''

# update ranges: the oracle driven site by site in colour order
_RANGES = _HEAD + r'''
n, ranges = fl.update_ranges(spec["width"])
model, tree, fp = fl.make_input(spec["tree"], n)
cap = fl.roomy(fp)
for first, last in ranges:
    d = device(tree, model, fp, cap, (first, last))
    check_plan(d, n)
    o = fl.oracle(tree, model, fp, cap, seed, opts)
    assert same_bits(d.tri_llh(), o.tri_llh())
    nd = no = 0
    for w in range(fl.RANGE_SWEEPS):
        nd += d.sweep(1, seed, sweep_base=w)
        no += fl.oracle_range_sweep(o, first, last, w)
        p = d.paths()
        assert orc.paths_equal(p, o.paths()), (first, last, w, "paths")
        assert same_bits(d.tri_llh(), o.tri_llh()), (first, last, w, "likelihoods")
        assert fl.columns_equal(p, fp, 0, first) and fl.columns_equal(p, fp, last + 1, n), (first, last, w, "outside")
    assert nd == no, (first, last, nd, no)
    print("range", first, last, "accepted", nd, flush=True)
    d.close()
print("ok")
'''

# halo mode: two contexts on one GPU against one unsharded oracle
_HALO = _HEAD + r'''
from epievo_amd.parallel import LocalGroup
L, n, S = spec["width"], fl.HALO_N, fl.HALO_SWEEPS
model, tree, fp = fl.make_input("tree", n)
cap = fl.roomy(fp)
g = LocalGroup(0, 2)
g.set_tree(tree); g.set_model(model); g.upload_paths(fp, cap)
assert len(g.subs) == 2
g.reset()
for s in g.subs:
    plan = s.phase_plan()
    print("plan", json.dumps(plan), flush=True)
    assert plan["propose"] == "fused" and plan["small_nn"] == 5 and plan["fused_lanes"] == L, plan
o = fl.oracle(tree, model, fp, cap, fl.HALO_SEED, {})
assert same_bits(g.tri_llh(), o.tri_llh())
Jg, Dg, ng = g.run_mcmc(2, 3, fl.HALO_SEED, sweep_base=7)
Jo, Do, no, _ = o.run_mcmc(2, 3, sweep_base=7)
assert ng == no, (ng, no)
assert np.array_equal(Jg, Jo) and np.array_equal(Dg, Do)
assert orc.paths_equal(g.paths(), o.paths()) and same_bits(g.tri_llh(), o.tri_llh())
# 60 sweeps twice: the second call finds fewer phases left than it needs and refreshes the internal halos
base = 12
for call in range(2):
    refresh = g.halo_phases_left() < 3 * S
    ng = g.sweep(S, fl.HALO_SEED, sweep_base=base)
    no = sum(o.sweep(base + w) for w in range(S))
    assert ng == no, (call, ng, no)
    assert orc.paths_equal(g.paths(), o.paths()), (call, "paths")
    assert same_bits(g.tri_llh(), o.tri_llh()), (call, "likelihoods")
    base += S
assert refresh, "no internal refresh happened"
assert all(s.phase_plan()["fused_lanes"] == L for s in g.subs)
g.close()
print("ok")
'''

# the width a context chooses by itself
_DEFAULT = _HEAD + r'''
n = spec["n"]
model, tree, fp = fl.make_input("pair", n)
# the fused phase's largest capacity (2 C + 1 <= 64 segments on a branch): on this many sites the usual
# 2 max + 8 is 30 to 36, and above 31 the context takes the separate kernels
cap = fl.FUSED_CAP
assert fp.counts().max() <= cap
d = device(tree, model, fp, cap)
plan = check_plan(d, n)
if spec["run"]:
    o = fl.oracle(tree, model, fp, cap, seed, opts)
    assert same_bits(d.tri_llh(), o.tri_llh())
    Jd, Dd, nd = d.run_mcmc(1, 2, seed, sweep_base=0)
    Jo, Do, no, _ = o.run_mcmc(1, 2, sweep_base=0)
    assert nd == no and nd > 0, (nd, no)
    assert np.array_equal(Jd, Jo) and np.array_equal(Dd, Do)
    assert orc.paths_equal(d.paths(), o.paths()) and same_bits(d.tri_llh(), o.tri_llh())
    assert d.counters()["overflow"] == o.counters()["overflow"]
    assert d.phase_plan() == plan
d.close()
print("ok")
'''


def _run(code, spec, env):
    src = code % dict(root=_ROOT, tests=_TESTS, spec=json.dumps(spec))
    clean = dict((k, v) for k, v in os.environ.items() if k not in ("EPV_FUSED_PHASE", "EPV_FUSED_LANES"))
    r = subprocess.run([sys.executable, "-c", src], env=dict(clean, **env), capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("tree,nodes,lengths,env,opts,expect,seed", [r[1:] for r in TAILS], ids=[r[0] for r in TAILS])
def test_tails_match_rung_b(tree, nodes, lengths, env, opts, expect, seed):
    _run(_PARITY, dict(tree=tree, nodes=nodes, lengths=lengths, opts=opts, expect=expect, seed=seed), env)


@pytest.mark.gpu
@pytest.mark.parametrize("tree,nodes,lengths,env,opts,expect,seed", [r[1:] for r in SEPARATE],
                         ids=[r[0] for r in SEPARATE])
def test_separate_kernels_tails_match_rung_b(tree, nodes, lengths, env, opts, expect, seed):
    _run(_PARITY, dict(tree=tree, nodes=nodes, lengths=lengths, opts=opts, expect=expect, seed=seed), env)


@pytest.mark.gpu
@pytest.mark.parametrize("tree,nodes,n,env,expect,seed", [r[1:] for r in OVERFLOW], ids=[r[0] for r in OVERFLOW])
def test_overflow_decisions_match_rung_b(tree, nodes, n, env, expect, seed):
    _run(_OVERFLOW, dict(tree=tree, nodes=nodes, n=n, expect=expect, seed=seed), env)


@pytest.mark.gpu
@pytest.mark.parametrize("tree,nodes,width,env,expect,seed", [r[1:] for r in RANGES], ids=[r[0] for r in RANGES])
def test_update_ranges_match_the_oracle_site_by_site(tree, nodes, width, env, expect, seed):
    _run(_RANGES, dict(tree=tree, nodes=nodes, width=width, expect=expect, seed=seed), env)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [r[1] for r in HALO], ids=[r[0] for r in HALO])
def test_halo_mode_matches_one_unsharded_oracle(width):
    _run(_HALO, dict(width=width), {"EPV_FUSED_LANES": str(width)})


@pytest.mark.gpu
@pytest.mark.parametrize("n,lanes,run", [r[1:] for r in DEFAULT], ids=[r[0] for r in DEFAULT])
def test_default_rule_chooses_the_width(n, lanes, run):
    _run(_DEFAULT, dict(n=n, run=run, expect=fused(2, lanes), seed=19), {})


# ---- no GPU
def test_tables_are_well_formed():
    """every length yields the lane count and the per-colour site counts its comment claims, ids are unique, the
    workloads exist"""
    for n in TINY:
        assert threads(n) == 1 and colour_counts(n) == TINY_COUNTS[n], n
    for L in WIDTHS + (8, 64, 84, 256):
        for _, n, thr, counts in SHAPES:
            assert threads(n(L)) == thr(L) and colour_counts(n(L)) == counts(L), (L, n(L))
            assert sum(counts(L)) == n(L) - 2
    assert tail_lengths(64) == [3, 4, 5, 193, 194, 195, 388] and tail_lengths(32) == [3, 4, 5, 97, 98, 99, 196]
    assert threads(27) == 9 and colour_counts(27) == [8, 8, 9]
    rows = TAILS + SEPARATE + OVERFLOW + RANGES + HALO + DEFAULT
    assert len(set(r[0] for r in rows)) == len(rows)
    for r in TAILS + SEPARATE + OVERFLOW + RANGES:
        assert config(r[1]).n_nodes == r[2], r[0]
    # the fused rows name both widths for every body, with and without forward rejection where the issue asks
    seen = set((r[1], r[6]["fused_lanes"], bool(r[5])) for r in TAILS)
    for L in WIDTHS:
        for key in [("pair", L, False), ("tree", L, False), ("star5", L, False), ("pair", L, True), ("tree", L, True)]:
            assert key in seen, key
        assert all(int(r[4]["EPV_FUSED_LANES"]) == r[6]["fused_lanes"] for r in TAILS)
    assert ("tree", 8, False) in seen
    assert sorted(r[6]["propose"] + r[6]["jumps"] for r in SEPARATE) == ["V1jumps_all", "V2jumps_all", "V2segments",
                                                                          "V3jumps_all"]
    assert all(r[4]["EPV_FUSED_PHASE"] == "0" and r[6]["fused_lanes"] == 0 for r in SEPARATE)
    for L in WIDTHS:
        n, ranges = update_ranges(L)
        assert n == 9 * L + 5 and len(ranges) == 21 and all(1 <= a <= b <= n - 2 for a, b in ranges)
        assert set(a % 3 for a, _ in ranges) == {0, 1, 2} and any(b == n - 2 for _, b in ranges)
        assert set(b - a + 1 for a, b in ranges) == {1, 2, 3, 3 * L, 3 * L + 1}
        assert threads(3 * L + 2) == L and threads(3 * L + 1 + 2) == L + 1      # a full wave, and one lane more
    # the thresholds of the default rule
    assert [phase_cap(r[1]) for r in DEFAULT] == [32768, 32769, 65536, 65537]
    assert phase_cap(DEFAULT[0][1] + 1) == 32769 and phase_cap(DEFAULT[1][1] - 1) == 32768
    assert phase_cap(DEFAULT[2][1] + 1) == 65537 and phase_cap(DEFAULT[3][1] - 1) == 65536
    for _, n, lanes, _ in DEFAULT:
        want = 64                   # plan_p2: halve while the launch at half the width has at most 2048 waves
        while want > 16 and -(-phase_cap(n) // (want // 2)) <= 2048:
            want //= 2
        assert want == lanes, (n, want, lanes)
    assert HALO_N >= 3072


def _moves(tree_name, n, seed, opts, sweeps):
    """the oracle's chain on a row's input: (accepted proposals, the final paths differ from the input)"""
    model, tree, fp = make_input(tree_name, n)
    o = oracle(tree, model, fp, roomy(fp), seed, opts)
    nacc = sum(o.sweep(w) for w in range(sweeps))
    return nacc, not orc.paths_equal(o.paths(), fp)


@pytest.mark.parametrize("row", TAILS + SEPARATE, ids=[r[0] for r in TAILS + SEPARATE])
def test_no_tail_row_is_vacuous(row):
    """on the oracle alone: the chain every length is compared with accepts a proposal and leaves the input, so a
    device that never moved could not pass"""
    _, tree, _, lengths, _, opts, _, seed = row
    for n in lengths:
        nacc, moved = _moves(tree, n, seed, opts, sweeps_for(n))
        assert nacc >= 1 and moved, (n, nacc, moved)


def test_no_overflow_range_or_halo_row_is_vacuous():
    for _, tree_name, _, n, _, _, seed in OVERFLOW:
        model, tree, fp = make_input(tree_name, n)
        o = oracle(tree, model, fp, int(fp.counts().max()), seed, {})
        nacc = sum(o.sweep(w) for w in range(3))
        assert o.counters()["overflow"] > 0 and nacc >= 1 and not orc.paths_equal(o.paths(), fp), (tree_name, n)
    for _, tree_name, _, L, _, _, seed in RANGES:
        n, ranges = update_ranges(L)
        model, tree, fp = make_input(tree_name, n)
        short = 0
        for first, last in ranges:
            o = oracle(tree, model, fp, roomy(fp), seed, {})
            nacc = sum(oracle_range_sweep(o, first, last, w) for w in range(RANGE_SWEEPS))
            p = o.paths()
            moved = not columns_equal(p, fp, first, last + 1)
            assert columns_equal(p, fp, 0, first) and columns_equal(p, fp, last + 1, n)
            if last - first + 1 >= 3 * L:
                assert nacc >= 1 and moved, (tree_name, first, last)
            else:
                short += moved
        assert short >= 1, tree_name
    model, tree, fp = make_input("tree", HALO_N)
    o = oracle(tree, model, fp, roomy(fp), HALO_SEED, {})
    assert sum(o.sweep(w) for w in range(7, 12)) >= 1 and not orc.paths_equal(o.paths(), fp)


def test_site_by_site_order_equals_the_sweep():
    """the reference of the range rows: over the whole interior, colour by colour and site by site is the sweep"""
    model, tree, fp = make_input("tree", 9 * 32 + 5)
    a, b = oracle(tree, model, fp, roomy(fp), 19, {}), oracle(tree, model, fp, roomy(fp), 19, {})
    for w in range(2):
        assert a.sweep(w) == oracle_range_sweep(b, 1, fp.n_sites - 2, w)
    assert orc.paths_equal(a.paths(), b.paths()) and np.array_equal(a.tri_llh(), b.tri_llh())
