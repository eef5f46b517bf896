"""The direct end-conditioned sampler (EPV_OPT_DIRECT_SAMPLER) on the device.  The CPU oracle has no such
mode; the yardstick is the restatement of tests/direct_ref.py (checked against the oracle's segment sampler and by hand
in tests/test_direct_sampler.py):

  1  epv_direct_kat == the restatement bit for bit, on the hand-worked cases and 2 000 random segments;
  2  a colour phase replays from the old paths: every new path is direct_segment over its segments;
  3  the kernel families agree bit for bit, the likelihood cache is a fresh reset()'s, time is conserved;
  4  the chain's stationary law against exact posterior draws (the criteria of tests/test_mcmc_posterior.py);
  5  the row model_cases.UNRUNNABLE records -- a kernel that does not return in the other modes -- runs (direct mode
     only, in a child process under a time limit);
  6  options: no two samplers at once, and the option reaches every context of a sharded driver.

Runs that need knobs in the environment, or a time limit, go through tests/direct_gpu_child.py."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import model_cases as mc
from direct_ref import GIVEUP, OK, OVERFLOW, direct_segment
from test_kernel_matrix import _SEP, v1, v2, v3
from test_trial_body import KAT_SEED

_TESTS = os.path.dirname(os.path.abspath(__file__))
DIRECT = {"direct_sampler": True}
DIRECT_REF = {"direct_sampler": True, "reference_proposal_ratio": True}


@functools.lru_cache(maxsize=None)
def _child(spec_json, env_json, timeout):
    r = subprocess.run([sys.executable, os.path.join(_TESTS, "direct_gpu_child.py"), spec_json],
                       env=dict(os.environ, **json.loads(env_json)), capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stderr[-3000:]
    return json.loads(r.stdout.splitlines()[-1][3:])


def child(spec, env=None, timeout=600):
    return _child(json.dumps(spec, sort_keys=True), json.dumps(env or {}, sort_keys=True), timeout)


# ---------------------------------------------------------------------------------------------------------
# 1  the body, bit for bit
def kat_cases():
    """(site, sweep, node, k, room, a0, end, T, r0, r1, start, first draw index): the hand-worked settings of the
    CPU part over many sites, then 2 000 random segments -- rates 1e-3 .. 1e5, lengths 1e-9 .. 1, room <= 64; consecutive items (the
    lanes of a wave) mix kept states with state changes"""
    rng = np.random.RandomState(77)
    cases = []
    for i in range(64):
        cases.append((i, 3, 2, 1, 64, 0, 0, 0.5, 1.3, 0.7, 0.0))
        cases.append((i, 3, 2, 1, 64, 0, 1, 0.5, 1.3, 0.7, 0.25))
        cases.append((i, 3, 2, 1, 64, 1, 1, 2.0, 3.0, 0.4, 0.0))
        cases.append((i, 3, 2, 1, (0, 1, 2, 3)[i % 4], i & 1, (i >> 1) & 1, 2.0, 3.0, 2.0, 0.5))
    cases.append((11, 3, 2, 1, 64, 0, 0, 1.0, 400.0, 400.0, 0.0))                 # overflows its 64 slots
    for a in (0, 1):
        for b in (0, 1):
            for r0, r1 in ((4.2e4, 8.7e-6), (8.7e-6, 4.2e4)):
                cases += [(s, 9, 4, 7, 64, a, b, 0.8, r0, r1, 0.125) for s in range(8)]
            cases.append((5, 9, 4, 7, 64, a, b, 1.0, 1e-9, 1e-9, 0.0))
    for i in range(2000):
        r0, r1 = (float(10.0 ** rng.uniform(-3, 5)) for _ in range(2))
        cases.append((int(rng.randint(0, 2 ** 31)), int(rng.randint(0, 2 ** 20)), int(rng.randint(1, 4096)),
                      int(rng.randint(0, 4096)), int(rng.randint(0, 65)), i & 1, int(rng.randint(2)),
                      float(10.0 ** rng.uniform(-9, 0)), r0, r1, float(rng.uniform(0.0, 2.0)) if i % 3 else 0.0))
    cases = [c + (0,) for c in cases]
    # the address row beyond trial word 1: no segment reaches draw 509 within 64 jumps, so these begin their draws
    # at an odd index just below a word's end (508 draws per word: words end at 508, 1016, ...) and cross it
    for i in range(192):
        first = (501, 503, 505, 507, 1009, 1013, 1015, 5 * 508 - 1, 509, 1017)[i % 10]
        cases.append((1000 + i, 4, 6, 2, 64, i & 1, (i >> 1) & 1, 2.0, 3.0, 2.0, 0.0, first))
    return cases


@pytest.mark.gpu
def test_direct_kat_equals_the_restatement():
    from epievo_amd.sampler import DeviceSampler
    cases = kat_cases()
    for w in range(0, len(cases) - 63, 64):
        assert {c[5] != c[6] for c in cases[w:w + 64]} == {True, False}
    items = np.array([[c[0], c[1], c[2], c[3], c[4], c[5] | c[6] << 1, c[11], 0] for c in cases], np.uint32)
    reals = np.array([[c[7], c[8], c[9], c[10]] for c in cases])
    d = DeviceSampler(0)
    w, t = d.direct_kat(KAT_SEED, items, reals)
    # arguments that no restatement could follow are refused on the host
    bad = reals[:1].copy()
    bad[0, 1] = float("nan")
    with pytest.raises(Exception):
        d.direct_kat(KAT_SEED, items[:1], bad)
    even = items[:1].copy()
    even[0, 6] = 508                    # a first draw in the second half of a block
    with pytest.raises(Exception):
        d.direct_kat(KAT_SEED, even, reals[:1])
    d.close()
    seen, crossed = set(), 0
    for i, c in enumerate(cases):
        oc, times, draws, longest = direct_segment(KAT_SEED, c[0], c[1], c[2], c[3], c[5], c[6], c[7], c[8], c[9], c[4], c[10],
                                                   first_draw_index=c[11])
        crossed += c[11] > 0 and (c[11] - 1) // 508 != (draws - 2) // 508        # first and last draw in different words
        assert oc != GIVEUP and longest <= 20
        assert (int(w[i, 0]), int(w[i, 1]), int(w[i, 2]), int(w[i, 3])) == (oc, len(times), draws, longest), (i, c, w[i])
        want = (times + [0.0] * 8)[:8]
        assert t[i].tolist() == want, (i, c, t[i], want)
        seen.add((oc, c[5] != c[6], min(len(times), 3)))
    assert {(OK, False, 0), (OK, False, 2), (OK, True, 1), (OK, True, 3), (OVERFLOW, False, 0), (OVERFLOW, True, 0),
            (OVERFLOW, False, 1)} <= seen, sorted(seen)
    assert crossed >= 50, crossed


# ---------------------------------------------------------------------------------------------------------
# 2  replay of a colour phase
_SEG0, _SEG1 = dict(_SEP, EPV_SEG_JUMPS="0"), dict(_SEP, EPV_SEG_JUMPS="1")
_LDS = {"EPV_FORCE_LDS_POOL": "1"}
_V2SEG, _V2SEQ = dict(v2(False, "segments"), direct=True), dict(v2(False, "jumps"), direct=True)
REPLAY = [
    # (id, workload, n, colours, only the pairs whose path changed, the least number of pairs compared, environment,
    # expected plan fields).  The least: every interior site of the colour on flat (all proposals are accepted);
    # elsewhere the sites of a colour times dense_cases' floor acceptance of 0.05, one branch each.
    # The homogeneous dense inputs leave the second proposal kernel whatever EPV_SEG_JUMPS says (test_dense_histories_gpu.py),
    # so the segment kernels' rows are the inputs thinned outside a window; mixed-tree300 has branches of more than
    # 64 segments, which leave the segment lists for the sequential kernel behind them.
    ("flat-tree300-seg0", "flat-tree300", 400, [1], False, 4 * 133, _SEG0, dict(direct=True, jumps="jumps")),
    ("flat-tree300-seg1", "flat-tree300", 400, [1], False, 4 * 133, _SEG1, dict(direct=True, jumps="jumps")),
    ("weak-tree40-seg0", "weak-tree40", 3000, [0], True, 50, _SEG0, dict(direct=True, jumps="jumps")),
    ("weak-tree40-seg1", "weak-tree40", 3000, [0], True, 50, _SEG1, dict(direct=True, jumps="jumps")),
    ("weak-pair10-seg0", "weak-pair10", 3000, [2], True, 50, _SEG0, dict(direct=True, jumps="jumps")),
    ("weak-pair10-seg1", "weak-pair10", 3000, [2], True, 50, _SEG1, dict(direct=True, jumps="jumps")),
    ("mixed-tree40-seg1", "mixed-tree40", None, [0, 1, 2], True, 30, dict(_SEG1, **_LDS), _V2SEG),
    ("mixed-tree40-seg0", "mixed-tree40", None, [0, 1, 2], True, 30, dict(_SEG0, **_LDS), _V2SEQ),
    ("mixed-tree300-seg1", "mixed-tree300", None, [0, 1, 2], True, 20, dict(_SEG1, **_LDS), _V2SEG),
]


@pytest.mark.gpu
@pytest.mark.parametrize("workload,n,colours,only_changed,least,env,expect", [r[1:] for r in REPLAY],
                         ids=[r[0] for r in REPLAY])
def test_colour_phase_replays_from_the_restatement(workload, n, colours, only_changed, least, env, expect):
    out = child(dict(kind="replay", input="dense", workload=workload, n=n, colours=colours, only_changed=only_changed,
                     opts=DIRECT, expect=expect), env)
    assert out["compared"] >= least, out
    assert out["plan"]["propose"] != "fused" and out["plan"]["jumps"] != "jumps_all"


# ---------------------------------------------------------------------------------------------------------
# 3  kernel families: (id, tree, n, environment, options, expected plan fields); the sizes of test_kernel_matrix's fr-* rows
FAMILY = [
    ("v2-jumps", "tree", 2000, dict(_SEP, EPV_SEG_JUMPS="0"), DIRECT, dict(v2(False, "jumps"), direct=True)),
    ("v2-seg", "tree", 2000, dict(_SEP, EPV_SEG_JUMPS="1"), DIRECT, dict(v2(False, "segments"), direct=True)),
    ("v1-lds-2000", "tree", 2000, dict(_SEP, EPV_PROPOSE_V1="1"), DIRECT,
     dict(v1(False, False, "jumps", "accept_cache"), direct=True)),
    ("v1-lds", "tree", 1500, dict(_SEP, EPV_PROPOSE_V1="1"), DIRECT, dict(v1(False, False, "jumps", "accept_cache"), direct=True)),
    ("v1-global", "tree", 1500, dict(_SEP, EPV_PROPOSE_V1="1", EPV_FORCE_GLOBAL_POOL="1"), DIRECT,
     dict(v1(True, False, "jumps", "accept_cache"), direct=True)),
    ("fused-asked", "tree", 1500, {}, DIRECT, dict(jumps="jumps", direct=True)),       # no knob: by default a launch this small fuses; direct mode must not
    ("ref-tree", "tree", 1500, {}, DIRECT_REF, dict(v1(False, True, "jumps", "accept_cache"), direct=True)),
    ("ref-tree-global", "tree", 1500, {"EPV_FORCE_GLOBAL_POOL": "1"}, DIRECT_REF,
     dict(v1(True, True, "jumps", "accept_cache"), direct=True)),
    ("bal16-v3", "bal16", 600, dict(_SEP, EPV_PROPOSE_V3="1"), DIRECT, dict(v3(1, False, "jumps"), direct=True)),
    ("bal16-v1", "bal16", 600, dict(_SEP, EPV_PROPOSE_V1="1"), DIRECT, dict(propose="V1", jumps="jumps", direct=True)),
    ("bal64-v3", "bal64", 400, dict(_SEP, EPV_PROPOSE_V3="1"), DIRECT, dict(v3(2, False, "jumps"), direct=True)),
    ("bal64-v1", "bal64", 400, dict(_SEP, EPV_PROPOSE_V1="1"), DIRECT, dict(propose="V1", jumps="jumps", direct=True)),
]


def _family(row):
    _, tree, n, env, opts, expect = row
    return child(dict(kind="family", input="matrix", tree=tree, n=n, opts=opts, expect=expect), env)


@pytest.mark.gpu
@pytest.mark.parametrize("row", FAMILY, ids=[r[0] for r in FAMILY])
def test_kernel_family_runs_and_agrees(row):
    out = _family(row)
    assert out["plan"]["propose"] != "fused" and out["plan"]["direct"]
    # every row of the same tree, size and options that has run so far (each runs once per session) gives the same bits
    for other in FAMILY:
        if other is row:
            break
        if other[1:3] == row[1:3] and other[4] == row[4]:
            o = _family(other)
            for key in ("paths", "stats", "nacc", "tri", "overflow"):
                assert o[key] == out[key], (row[0], other[0], key)


def test_family_rows_cover_what_they_claim():
    fams = {(r[5].get("propose"), r[5].get("gpool"), r[5].get("jumps"), r[5].get("p3_words"), bool(r[4].get(
        "reference_proposal_ratio"))) for r in FAMILY}
    for key in (("V2", False, "jumps", 0, False), ("V2", False, "segments", 0, False), ("V1", False, "jumps", 0, False),
                ("V1", True, "jumps", 0, False), ("V3", False, "jumps", 1, False), ("V3", False, "jumps", 2, False),
                ("V1", False, "jumps", 0, True)):
        assert key in fams, key
    groups = {}
    for r in FAMILY:
        groups.setdefault((r[1], r[2], json.dumps(r[4], sort_keys=True)), []).append(r[0])
    assert all(len(g) >= 2 for g in groups.values()), groups               # every row has a partner to agree with


# ---------------------------------------------------------------------------------------------------------
# 4  the stationary law
@pytest.mark.gpu
@pytest.mark.parametrize("seed", (21, 22))
def test_direct_chain_matches_exact_posterior_on_the_tree(seed):
    from common import ref_test_model
    from epievo_amd.sampler import DeviceSampler
    from test_mcmc_posterior import TROOT, _check_tree, _exact_tree, _tree_case
    model = ref_test_model()
    tree, leaf, fp = _tree_case()
    exact = _exact_tree(model, tree, leaf)
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, 32)
    d.set_direct_sampler(True)
    d.reset()
    assert d.phase_plan()["direct"] and d.phase_plan()["propose"] != "fused"
    J, D, nacc = d.run_mcmc(300, 12000, seed)
    _check_tree(J, D, 1200.0, exact, tree)
    p = d.paths()
    B, n = tree.n_nodes - 1, len(TROOT)
    es = (p.init.reshape(B, n) ^ (p.counts().reshape(B, n) & 1).astype(np.uint8))
    for b in range(1, tree.n_nodes):
        if tree.subtree_sizes[b] == 1:
            assert np.array_equal(es[b - 1], leaf[b])
    assert d.direct_giveups() == 0
    d.close()


# ---------------------------------------------------------------------------------------------------------
# 5  the unrunnable row.  NEVER in another mode: there it is a kernel that does not return.
# Measured in one session on an MI355X: the ratio-tree row of model_cases (the same model on its own data, n = 200,
# the same run_mcmc(2, 3) and checks, direct mode: direct_gpu_child.py with kind "family", input "row", rid
# "ratio-tree" under this test's environment) took 0.51, 0.42 and 0.31 s as a whole child process -- the
# interpreter's start, the imports and the context included; the yardstick is the slowest, the limit ten times
# that.  The unrunnable row itself took 0.55 s in that session, its replayed phase included.
UNRUNNABLE_YARDSTICK_S = 0.51
UNRUNNABLE_LIMIT_S = 10.0 * UNRUNNABLE_YARDSTICK_S


@pytest.mark.gpu
def test_the_unrunnable_row_runs():
    assert mc.UNRUNNABLE == (("ref", "ratio", "tree", 300),)
    out = child(dict(kind="unrunnable", input="model_space", row=list(mc.UNRUNNABLE[0]), opts=DIRECT,
                     expect=dict(direct=True, jumps="jumps")), dict(_SEP, EPV_SEG_JUMPS="0"), UNRUNNABLE_LIMIT_S)
    print("seconds", out["seconds"])
    assert out["compared"] > 0 and out["nacc"] > 0


# ---------------------------------------------------------------------------------------------------------
# 6  options
@pytest.mark.gpu
def test_direct_with_forward_rejection_is_refused():
    from common import simulate
    from epievo_amd.sampler import DeviceSampler, EpvError
    model, tree, fp = simulate("tree", 300, seed=8)
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, 16)
    d.set_options(forward_rejection=True)
    with pytest.raises(EpvError) as e:
        d.set_direct_sampler(True)
    assert e.value.code == 1 and "two samplers" in str(e.value)            # EPV_ERR_ARG
    d.set_options()
    d.set_direct_sampler(True)
    with pytest.raises(EpvError) as e:       # ... in either order
        d.set_options(forward_rejection=True)
    assert e.value.code == 1
    for other in ({"reference_proposal_ratio": True}, {"sample_root": True}, {}):
        d.set_options(**other)
        d.set_direct_sampler(True)
    d.reset()
    plan = d.phase_plan()
    assert plan["direct"] and plan["propose"] != "fused" and plan["jumps"] in ("jumps", "segments")
    d.set_options()                          # its three bits only: the direct sampler stays on
    assert d.phase_plan()["direct"]
    d.set_direct_sampler(False)
    assert not d.phase_plan()["direct"]
    assert d.direct_giveups() == 0
    d.close()


@pytest.mark.gpu
def test_option_reaches_every_context_of_a_driver():
    out = child(dict(kind="two_contexts", input="matrix", tree="tree", n=40000, opts=DIRECT, expect={}))
    assert out["one"]["paths"] == out["two"]["paths"] and out["one"]["stats"] == out["two"]["stats"], out
    assert out["one"]["acc"] == out["two"]["acc"]
    # ... and it is the direct sampler's result, not the default's on every part
    ref = child(dict(kind="two_contexts", input="matrix", tree="tree", n=40000, opts={}, expect={}))
    assert ref["one"]["paths"] == ref["two"]["paths"] and ref["one"]["paths"] != out["one"]["paths"]


# ---------------------------------------------------------------------------------------------------------
# 4, continued: a single branch under `weak` at T = 1.5 (test_direct_sampler.WEAK_T: chosen on the CPU so that the
# exact sampler keeps its 20 000 histories within its cap and 0.54 of their paths have two or more jumps -- the keep
# arm's rejection draws most of the jump times here).  test_gpu_chain_matches_exact_posterior with the direct sampler.
@pytest.mark.gpu
@pytest.mark.parametrize("seed", (99, 100))
def test_direct_chain_matches_exact_posterior_on_a_weak_branch(seed):
    from epievo_amd import host
    from epievo_amd.sampler import DeviceSampler
    from test_direct_sampler import WEAK_T, weak_check, weak_exact, weak_initial_paths, weak_model
    d = DeviceSampler(0)
    d.set_tree(host.Tree.single_branch(WEAK_T))
    d.set_model(weak_model())
    d.upload_paths(weak_initial_paths(), 48)
    d.set_direct_sampler(True)
    d.reset()
    assert d.phase_plan()["direct"] and d.phase_plan()["propose"] != "fused"
    J, D, nacc = d.run_mcmc(500, 20000, seed)
    weak_check(J, D, 2000.0, weak_exact())
    assert d.direct_giveups() == 0 and d.counters()["overflow"] == 0
    d.close()
