"""The acceptance stage of the fused small-tree phase merges a triple's jumps with ONE body per event
(merge3_sel in epv_kernels.h: the advancing path chosen by selects, one accumulator update, one predicated
load) instead of three divergent arms.  Events, their order, the tie rules and every sum stay what they were:

  * CPU: a restatement of the three-way merge in Python (floats are IEEE doubles, so its sums are
    bit-comparable), checked against answers worked out by hand, and the case generator the GPU part uses;
  * GPU, known answers (epv_merge_kat): merge3 with register accumulators (the untouched form) and merge3_sel
    with LDS accumulators behind the batched first-jump load must both equal the restatement bit for bit on
    every generated case.  Tied jump times are tested HERE ONLY: in a whole run a tie makes a zero-length
    segment, for which the end-conditioned sampler is not specified.  Like the other known-answer entries
    this runs the functions in a kernel of their own, not a call site inside the MCMC kernels;
  * GPU, whole runs against the parallel rung (oracle rung B), bit for bit -- paths, cached triple
    likelihoods, J, D, the accept count and the overflow counter -- with the small-tree body (the one that
    calls merge3_sel) and the generic one, each asserted to be the body that ran: a window of jumps on sites
    384 .. 479 at capacity 4, n = 1000 (contents below), and n = 193 simulated (a partial last wave, the
    skipped genome-edge triples), on tree.nwk (NB = 4) and the single branch (NB = 1)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))

INF = float("inf")


# ---------------------------------------------------------------------------------------------------------
# the restatement
def merge_ref(init, cols, blen):
    """D[8], J[8] of one branch of a triple: init = start states (left, middle, right), cols = the three
    paths' jump times, blen = the branch length.  Context = 4 left + 2 middle + right.  The earliest head
    advances; ties: left only if strictly below min(middle, right), else middle only if strictly below
    right, else right.  The time since the previous event goes to D[context], a middle jump counts in
    J[context], the path's state flips; the time from the last event to blen closes the branch."""
    D, J = [0.0] * 8, [0] * 8
    ctx = 4 * init[0] + 2 * init[1] + init[2]
    at = [0, 0, 0]
    prev = 0.0
    while any(at[c] < len(cols[c]) for c in range(3)):
        tl, tm, tr = (cols[c][at[c]] if at[c] < len(cols[c]) else INF for c in range(3))
        if tl < min(tm, tr):
            c, t = 0, tl
        elif tm < tr:
            c, t = 1, tm
        else:
            c, t = 2, tr
        D[ctx] += t - prev
        if c == 1:
            J[ctx] += 1
        prev = t
        ctx ^= (4, 2, 1)[c]
        at[c] += 1
    D[ctx] += blen - prev
    return D, J


# ---------------------------------------------------------------------------------------------------------
# the cases: (init, cols, blen)
def _interleavings():
    """every order in which up to 2 + 2 + 2 jumps can interleave: event r of the order happens at (r + 1) / 8"""
    out = []
    for counts in itertools.product(range(3), repeat=3):
        labels = [0] * counts[0] + [1] * counts[1] + [2] * counts[2]
        for order in sorted(set(itertools.permutations(labels))):
            cols = ([], [], [])
            for r, c in enumerate(order):
                cols[c].append((r + 1) / 8.0)
            out.append((cols, 1.0))
    return out


def _counts_0_to_8():
    rng = np.random.RandomState(11)
    out = []
    triples = [(k, (k + 3) % 9, (2 * k + 5) % 9) for k in range(9)] + [(8, 8, 8), (8, 0, 0), (0, 8, 0), (0, 0, 8),
                                                                       (1, 8, 8), (8, 1, 8), (8, 8, 1)]
    for counts in triples:
        cols = tuple([float(x) for x in np.sort(rng.uniform(0.01, 0.74, k))] for k in counts)
        out.append((cols, 0.75))
    return out


def _empty_columns():
    a, b = [0.125, 0.5, 0.625], [0.25, 0.375]
    return [(([], [], []), 0.75), ((a, [], []), 1.0), (([], a, []), 1.0), (([], [], a), 1.0),
            ((a, b, []), 1.0), ((a, [], b), 1.0), (([], a, b), 1.0), ((b, a, []), 1.0)]


def _ties():
    """every tie pattern, at the first jump and at a later one; the untied column jumps elsewhere, or not at all"""
    out = []
    for tied in ((0, 1), (0, 2), (1, 2), (0, 1, 2)):
        for later in (False, True):
            for rest in ("none", "before", "after"):
                cols = ([], [], [])
                for c in range(3):
                    if c in tied:
                        # (later: distinct first jumps, then the tie; one more jump behind it on the first tied column)
                        cols[c].extend([0.0625 * (c + 1), 0.5] if later else [0.5])
                        if c == tied[0]:
                            cols[c].append(0.8125)
                    elif rest == "before":
                        cols[c].extend([0.03125, 0.4375])
                    elif rest == "after":
                        cols[c].extend([0.5625, 0.875])
                out.append((cols, 1.0))
    # two ties in a row, and a tie of all three on every one of three jumps
    out.append((([0.25, 0.5], [0.25, 0.5], [0.75]), 1.0))
    out.append((([0.25, 0.5, 0.75], [0.25, 0.5, 0.75], [0.25, 0.5, 0.75]), 1.0))
    return out


def _closing():
    """a last jump AT the branch length (a zero closing interval), on each column, on two and on all three"""
    out = []
    for cs in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
        cols = ([0.25], [0.375], [0.5])
        for c in cs:
            cols[c].append(1.5)
        out.append((cols, 1.5))
    out.append((([1.5], [], []), 1.5))
    return out


def _tiny_gaps():
    sub = 5e-324           # the smallest subnormal
    return [
        (([sub], [2 * sub], [3 * sub]), 1.0),
        (([sub, 4 * sub], [2 * sub, 2e-310], [3 * sub, 1e-308]), 1e-307),
        (([1e-300], [2e-300], [3e-300]), 1.0),
        (([1e-300, 4e-300], [2e-300, 5e-300], [3e-300, 6e-300]), 7e-300),
        (([0.5, 0.5 + 2.0 ** -53], [0.5 + 2.0 ** -52], [0.5 - 2.0 ** -54]), 1.0),
        (([1e-300], [0.5], [0.5 + 1e-300]), 1.0),                    # (a gap that rounds away)
        (([2.2250738585072014e-308], [2.225073858507201e-308], []), 3e-308),   # (the smallest normal and the largest subnormal)
    ]


def merge_cases():
    """the list of (init, cols, blen): the start states cycle through all eight patterns along the list, and
    one case of each family is repeated under all eight"""
    fams = [_interleavings(), _counts_0_to_8(), _empty_columns(), _ties(), _closing(), _tiny_gaps()]
    out = []
    for fam in fams:
        for cols, blen in fam:
            i = len(out) % 8
            out.append(((i >> 2 & 1, i >> 1 & 1, i & 1), cols, blen))
        cols, blen = fam[-1]
        out.extend(((i >> 2 & 1, i >> 1 & 1, i & 1), cols, blen) for i in range(8))
    return out


# ---------------------------------------------------------------------------------------------------------
# CPU
def test_cases_cover_what_they_claim():
    cases = merge_cases()
    assert len(_interleavings()) == sum(
        len(set(itertools.permutations([0] * a + [1] * b + [2] * c))) for a in range(3) for b in range(3) for c in range(3))
    for c in range(3):
        assert {len(cols[c]) for _, cols, _ in cases} >= set(range(9))                 # 0 .. 8 jumps per column
        assert {init[c] for init, _, _ in cases} == {0, 1}                             # both start states
    empties = {tuple(len(x) == 0 for x in cols) for _, cols, _ in cases}
    assert len(empties) == 8                                                           # none, one, two or all three empty
    for _, cols, blen in cases:
        for col in cols:
            assert len(col) <= 8 and all(np.isfinite(col)) and list(col) == sorted(col) and (not col or col[-1] <= blen)

    def tie_kinds(cols):
        kinds = set()
        for a, b in ((0, 1), (0, 2), (1, 2)):
            for ia, x in enumerate(cols[a]):
                for ib, y in enumerate(cols[b]):
                    if x == y:
                        kinds.add((a, b, ia == 0 and ib == 0))
        return kinds
    seen = set()
    for _, cols, _ in cases:
        seen |= tie_kinds(cols)
    assert seen >= {(a, b, first) for a, b in ((0, 1), (0, 2), (1, 2)) for first in (True, False)}
    assert any(cols[0][:1] == cols[1][:1] == cols[2][:1] and cols[0] for _, cols, _ in cases)
    assert any(len(cols[0]) > 1 and cols[0][1:2] == cols[1][1:2] == cols[2][1:2] for _, cols, _ in cases)
    assert any(col and col[-1] == blen for _, cols, blen in cases for col in cols)     # a zero closing interval
    assert any(0.0 < col[0] < 2.3e-308 for _, cols, _ in cases for col in cols if col)  # subnormal
    assert any(col[0] == 1e-300 for _, cols, _ in cases for col in cols if col)


def _dj(**kw):
    D, J = [0.0] * 8, [0] * 8
    for k, v in kw.items():
        (D if k[0] == "d" else J)[int(k[1])] = v
    return D, J


# (binary fractions, so the sums worked out by hand are exact)
HAND = [
    # no jump at all: the whole branch in the start context 4 + 1
    (((1, 0, 1), ([], [], []), 0.75), _dj(d5=0.75)),
    # one left jump: context 0 until 0.25, then 4
    (((0, 0, 0), ([0.25], [], []), 1.0), _dj(d0=0.25, d4=0.75)),
    # one middle jump out of context 2: counted there
    (((0, 1, 0), ([], [0.5], []), 1.0), _dj(d2=0.5, j2=1, d0=0.5)),
    # left 0.125, right 0.25, middle 0.5, left 0.75 from (0, 0, 0): contexts 0, 4, 5, 7, 3
    (((0, 0, 0), ([0.125, 0.75], [0.5], [0.25]), 1.0), _dj(d0=0.125, d4=0.125, d5=0.25, j5=1, d7=0.25, d3=0.25)),
    # all three tied at 0.5: right goes first, then middle, then left, the last two after zero time
    (((0, 0, 0), ([0.5], [0.5], [0.5]), 1.0), _dj(d0=0.5, d1=0.0, j1=1, d3=0.0, d7=0.5)),
    # left and middle tied at 0.25 below right: middle first (counted in 7), left after zero time, right at 0.5
    (((1, 1, 1), ([0.25], [0.25], [0.5]), 1.0), _dj(d7=0.25, j7=1, d5=0.0, d1=0.25, d0=0.5)),
    # left and right tied: right first
    (((0, 1, 0), ([0.5], [], [0.5]), 2.0), _dj(d2=0.5, d3=0.0, d7=1.5)),
    # a jump at the branch length: a zero closing interval in context 1
    (((0, 0, 0), ([], [], [1.0]), 1.0), _dj(d0=1.0, d1=0.0)),
    # two middle jumps in a row return to the start context: 0.25 + 0.5 there
    (((1, 0, 0), ([], [0.25, 0.5], []), 1.0), _dj(d4=0.75, j4=1, d6=0.25, j6=1)),
]


@pytest.mark.parametrize("i", range(len(HAND)))
def test_restatement_against_hand_computed(i):
    (init, cols, blen), (D, J) = HAND[i]
    Dr, Jr = merge_ref(init, cols, blen)
    assert Jr == J
    assert np.array_equal(np.array(Dr).view(np.uint64), np.array(D).view(np.uint64)), (Dr, D)


def test_restatement_conserves_time_and_jumps():
    for init, cols, blen in merge_cases():
        D, J = merge_ref(init, cols, blen)
        assert sum(J) == len(cols[1]) and all(d >= 0.0 for d in D)
        # (at most 24 events + 1: a difference and a sum each, 8 more sums here, half an ulp of blen apiece)
        assert abs(sum(D) - blen) <= 32 * np.spacing(blen)


# ---------------------------------------------------------------------------------------------------------
# GPU: known answers
@pytest.mark.gpu
def test_merge_kat_both_forms_equal_the_restatement():
    from epievo_amd.sampler import DeviceSampler
    cases = merge_cases() + [h[0] for h in HAND]
    d = DeviceSampler(0)
    D, J = d.merge_kat(cases)
    d.close()
    assert D.shape == (len(cases), 2, 8) and J.shape == (len(cases), 2, 8)
    bad = []
    for i, (init, cols, blen) in enumerate(cases):
        Dr, Jr = merge_ref(init, cols, blen)
        Dr, Jr = np.array(Dr), np.array(Jr, np.uint32)
        for form, name in enumerate(("merge3<Acc8>", "merge3_sel<AccLds>")):
            if not (np.array_equal(D[i, form].view(np.uint64), Dr.view(np.uint64)) and np.array_equal(J[i, form], Jr)):
                bad.append((i, name, init, cols, blen, D[i, form].tolist(), Dr.tolist(), J[i, form].tolist(), Jr.tolist()))
    assert not bad, "%d of %d differ, first: %r" % (len(bad), 2 * len(cases), bad[0])


# ---------------------------------------------------------------------------------------------------------
# whole runs against rung B
SEEDS = (31, 0xFFFFFFFF9E3779B9)
WIN_N, WIN_LO, WIN_HI, WIN_CAP = 1000, 384, 479, 4

# jumps of (site, node) inside the window.  A site's colour is site % 3, and a colour phase merges the
# triples around the sites of one colour:
#   mixed      0 .. 3 jumps side by side: the lanes of a wave spread over all three paths, empty columns
#              (load predicated off, merge from +inf) next to ones with later jumps on demand;
#   outer      3 jumps on two colours, none on the third: in that colour's phase every centre triple
#              advances its two outer paths only, in the other two phases whole waves mix all three;
#   inner      the reverse: 3 jumps on one colour only -- in its phase every centre triple advances the
#              middle path only (the J increment on every event), the neighbours' triples one outer path;
#   full       4 jumps on three sites of four, none on the fourth: full columns, K up to 2 C + 1 = 9.
WINDOW_COUNTS = {
    "mixed": lambda site, node: (7 * site + 3 * node) % 4,
    "outer": lambda site, node: np.where(site % 3 != 1, 3, 0),
    "inner": lambda site, node: np.where(site % 3 == 1, 3, 0),
    "full": lambda site, node: np.where(site % 4 != 1, 4, 0),
}
CASES = [(cfg, kind, WIN_N) for cfg in ("tree", "pair") for kind in sorted(WINDOW_COUNTS)] + \
        [(cfg, "simulated", 193) for cfg in ("tree", "pair")]


def _inputs(cfg, kind, n):
    from common import simulate, config, ref_test_model
    from test_fused_dense_draws import window_paths
    if kind == "simulated":
        model, tree, fp = simulate(cfg, n, seed=8)
        return model, tree, fp, int(max(16, 2 * fp.counts().max() + 8))
    model, tree = ref_test_model(), config(cfg)
    fp = window_paths(tree, n, WIN_LO, WIN_HI, 5, WINDOW_COUNTS[kind])
    cnt = fp.counts().reshape(tree.n_nodes - 1, -1)
    assert cnt.max() <= WIN_CAP and cnt[:, WIN_LO:WIN_HI + 1].max() >= 3 and cnt[:, :WIN_LO].max() == 0
    return model, tree, fp, WIN_CAP


@pytest.mark.parametrize("cfg,kind,n", CASES)
def test_oracle_alone_accepts_and_does_not_overflow(cfg, kind, n):
    """what the whole runs below rest on, on the CPU: the rung they compare against accepts proposals on
    every case (a comparison of untouched paths would show nothing) and, on tree.nwk, never overflows"""
    import orc
    model, tree, fp, cap = _inputs(cfg, kind, n)
    for seed in SEEDS:
        o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
        o.reset()
        _, _, nacc, _ = o.run_mcmc(1, 2)
        assert nacc > 0, (cfg, kind, seed)
        if cfg == "tree":
            assert o.counters()["overflow"] == 0, (cfg, kind, seed)


_CODE = r'''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import orc
from epievo_amd.sampler import DeviceSampler
import test_fused_merge_select as T
model, tree, fp, cap = T._inputs(%(cfg)r, %(kind)r, %(n)d)
small = tree.n_nodes
assert small <= 5

def run(knob, seed):
    os.environ["EPV_P2_SMALL_TREE"] = knob       # read when a context is created
    d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap); d.reset()
    assert d.phase_mode() == 3                    # EPV_PHASE_FUSED
    plan = d.phase_plan()
    assert plan["propose"] == "fused" and plan["small_nn"] == (small if knob == "1" else 0), plan
    # (an overflow -- expected on the single branch at capacity 4 -- leaves a valid chain and complete
    # outputs; auto_grow only keeps run_mcmc from raising)
    d.auto_grow = True
    J, D, nacc = d.run_mcmc(1, 2, seed)
    out = dict(J=J, D=D, nacc=nacc, paths=d.paths(), tri=d.tri_llh(), cnt=d.counters())
    d.close()
    return out

for seed in T.SEEDS:
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed); o.reset()
    Jo, Do, no, _ = o.run_mcmc(1, 2)
    ovf = o.counters()["overflow"]
    print("seed %%x oracle: nacc %%d overflow %%d" %% (seed, no, ovf))
    assert no > 0
    if %(cfg)r == "tree":
        assert ovf == 0
    for knob in ("1", "0"):
        r = run(knob, seed)
        print("knob %%s: nacc %%d overflow %%d" %% (knob, r["nacc"], r["cnt"]["overflow"]))
        assert r["nacc"] == no, (knob, r["nacc"], no)
        assert r["cnt"]["overflow"] == ovf, (knob, r["cnt"], ovf)
        assert orc.paths_equal(r["paths"], o.paths()), knob
        assert np.array_equal(r["tri"].view(np.uint64), o.tri_llh().view(np.uint64)), knob
        assert np.array_equal(r["J"], Jo) and np.array_equal(r["D"].view(np.uint64), Do.view(np.uint64)), knob
print("ok")
'''


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,kind,n", CASES)
def test_whole_run_equals_rung_b(cfg, kind, n):
    code = _CODE % dict(root=_ROOT, tests=_TESTS, cfg=cfg, n=n, kind=kind)
    e = dict(os.environ, EPV_FUSED_PHASE="1")
    # "full" on tree.nwk: a jump density at which the default plan does not keep the record pool in LDS and
    # gives the phase to other kernels (tests/test_fused_dense_draws.py explains); the knob keeps it there
    if cfg == "tree" and kind == "full":
        e["EPV_FORCE_LDS_POOL"] = "1"
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
