"""The fused colour phase's direct bodies (EPV_OPT_DIRECT_FUSED, set_direct_sampler(True, fused=True)).
The switch selects a kernel, never a result: everything is compared bit for bit, with the separate direct kernels and
with the restatement of tests/direct_ref.py.

  1  every fused body (small-tree NN = 2 .. 5, generic; 16, 32 and 64 sites per wave) == the separate direct kernels;
  2  a fused direct colour phase replays from the restatement;
  3  capacity overflows inside the fused body (the LDS flags of a small-tree body, S.prop_flag of the generic one);
  4  where the fused phase is not eligible the switch changes neither the plan nor a bit; the option's rules;
  5  the option reaches every context of a driver and of a LocalGroup, and --direct-fused of the two programs;
  6  the row model_cases.UNRUNNABLE records runs through the fused direct body, under a time limit;
  7  the chain's stationary law, with the plan asserted fused;
  8  (no GPU) the tables name what they claim.

Every GPU run that needs knobs in the environment, or a time limit, is a process of its own
(tests/direct_fused_gpu_child.py), which asserts its plan before it launches a colour phase."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import model_cases as mc
import test_direct_sampler_gpu as base
from test_kernel_matrix import REF, SR, _SEP, fused, make_tree

_TESTS = os.path.dirname(os.path.abspath(__file__))
CHILD_LIMIT_S = 300          # a direct-mode run always returns; the limit is for a broken build


@functools.lru_cache(maxsize=None)
def _child(spec_json, env_json, timeout):
    r = subprocess.run([sys.executable, os.path.join(_TESTS, "direct_fused_gpu_child.py"), spec_json],
                       env=dict(os.environ, **json.loads(env_json)), capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stderr[-3000:]
    return json.loads(r.stdout.splitlines()[-1][3:])


def child(spec, env=None, timeout=CHILD_LIMIT_S):
    return _child(json.dumps(spec, sort_keys=True), json.dumps(env or {}, sort_keys=True), timeout)


_FUSED_KNOBS = ("EPV_FUSED_PHASE", "EPV_FUSED_LANES", "EPV_P2_SMALL_TREE")
BITS = ("paths", "stats", "nacc", "tri", "overflow")


def partners(env):
    """the environments of a row's separate-kernel partners: its own knobs without those of the fused phase, the
    fused phase off, the sequential and the segment-parallel jump kernels"""
    keep = dict((k, v) for k, v in env.items() if k not in _FUSED_KNOBS)
    return [dict(keep, EPV_SEG_JUMPS=s, **_SEP) for s in ("0", "1")]


def agrees_with_the_separate_kernels(spec, env):
    out = child(dict(spec, fused=True), env)
    assert out["plan"]["direct"] and out["plan"]["propose"] == "fused"
    for penv in partners(env):
        sep = child(dict(spec, fused=False, expect={}), penv)
        assert sep["plan"]["direct"] and sep["plan"]["propose"] != "fused"
        for key in BITS:
            assert sep[key] == out[key], (key, penv, sep[key], out[key])
    return out


# ---------------------------------------------------------------------------------------------------------
# 1  every fused body: (id, tree, n, environment, expected plan).  The sizes of test_kernel_matrix's fr-* rows.
_L32 = {"EPV_FUSED_PHASE": "1", "EPV_FUSED_LANES": "32"}
_L64 = {"EPV_FUSED_PHASE": "1", "EPV_FUSED_LANES": "64"}
_GEN = {"EPV_P2_SMALL_TREE": "0"}
_FUSED_LDS = {"EPV_FUSED_PHASE": "1", "EPV_FORCE_LDS_POOL": "1"}
FAMILY = [
    ("pair", "pair", 1500, {}, fused(2)),
    ("cherry", "cherry", 1500, {}, fused(3)),
    ("star3", "star3", 1500, {}, fused(4)),
    ("tree", "tree", 1500, {}, fused(5)),
    ("star5", "star5", 1500, {}, fused(0)),
    ("tree-generic", "tree", 1500, _GEN, fused(0)),
    ("tree-lanes32", "tree", 1500, _L32, fused(5, 32)),
    ("tree-lanes64", "tree", 1500, _L64, fused(5, 64)),
    ("tree-generic-lanes32", "tree", 1500, dict(_L32, **_GEN), fused(0, 32)),
    ("tree-generic-lanes64", "tree", 1500, dict(_L64, **_GEN), fused(0, 64)),
    ("star5-lanes32", "star5", 1500, _L32, fused(0, 32)),
    ("star5-lanes64", "star5", 1500, _L64, fused(0, 64)),
    ("cat6", "cat6", 1500, _FUSED_LDS, fused(0)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("tree,n,env,expect", [r[1:] for r in FAMILY], ids=[r[0] for r in FAMILY])
def test_fused_body_agrees_with_the_separate_direct_kernels(tree, n, env, expect):
    out = agrees_with_the_separate_kernels(dict(kind="family", input="matrix", tree=tree, n=n, opts={}, expect=expect), env)
    assert out["giveups"] == 0 and out["coop_tasks"] > 0      # branches went through the fused jump stage
    assert out["search_finished"] == 0                          # ... and none through the default mode's grouped search


# ---------------------------------------------------------------------------------------------------------
# 2  replay: (id, workload, n, colours, only the changed pairs, least pairs compared, environment, capacity, expected
# plan or None).  Workloads, colours and floors are those of test_direct_sampler_gpu.REPLAY.  The fused phase holds
# at most 64 segments per branch, so 31 jump slots: the workloads dense_cases labels "fused" run at that capacity
# (dense_cases.FUSED_CAP, as in test_dense_histories_gpu.py), and so does weak-pair10, whose input has at most 31
# jumps on a path (test_replay_capacities_hold_their_inputs).  None: the workload CANNOT plan the fused phase --
# flat-tree300 and mixed-tree300 hold paths of more than 31 jumps (that is what makes their branches longer than 64
# segments), no capacity the fused phase takes can hold them.  Those rows run all the same: with the switch on, the
# plan is not fused and the phase replays as it does without it.
CANNOT = None
REPLAY = [
    ("flat-tree300", "flat-tree300", 400, [1], False, 4 * 133, _FUSED_LDS, 0, CANNOT),
    ("weak-tree40", "weak-tree40", 3000, [0], True, 50, _FUSED_LDS, 31, fused(5)),
    ("weak-tree40-generic", "weak-tree40", 3000, [0], True, 50, dict(_FUSED_LDS, **_GEN), 31, fused(0)),
    ("weak-pair10", "weak-pair10", 3000, [2], True, 50, _FUSED_LDS, 31, fused(2)),
    ("mixed-tree40", "mixed-tree40", None, [0, 1, 2], True, 30, _FUSED_LDS, 31, fused(5)),
    ("mixed-tree40-lanes64", "mixed-tree40", None, [0, 1, 2], True, 30, dict(_FUSED_LDS, EPV_FUSED_LANES="64"), 31,
     fused(5, 64)),
    ("mixed-tree300", "mixed-tree300", None, [0, 1, 2], True, 20, _FUSED_LDS, 0, CANNOT),
]


@pytest.mark.gpu
@pytest.mark.parametrize("workload,n,colours,only_changed,least,env,cap,expect", [r[1:] for r in REPLAY],
                         ids=[r[0] for r in REPLAY])
def test_fused_direct_phase_replays_from_the_restatement(workload, n, colours, only_changed, least, env, cap, expect):
    out = child(dict(kind="replay", input="dense", workload=workload, n=n, colours=colours, only_changed=only_changed,
                     fused=True, must_fuse=expect is not CANNOT, cap=cap, expect=expect or {}), env)
    assert out["compared"] >= least, out
    if expect is CANNOT:
        assert out["cap"] > 31 and out["plan"]["propose"] != "fused", out
    else:
        assert out["cap"] == 31 and out["plan"]["propose"] == "fused", out


def test_replay_capacities_hold_their_inputs():
    """no GPU: a row that runs at the fused phase's 31 slots has no longer path in its input; a row marked CANNOT has"""
    import dense_cases as dc
    for r in REPLAY:
        _, _, fp = dc.workload(r[1], r[2])
        most = int(fp.counts().max())
        assert (most <= 31) == (r[8] is not CANNOT), (r[0], most)
        assert (r[7] == 31) == (r[8] is not CANNOT), r[0]


# ---------------------------------------------------------------------------------------------------------
# 3  overflow inside the fused body: the `fast` model on the data of test.param, tree.nwk, 16 slots
OVERFLOW_ROW = "fast-tree"
OVERFLOW = [("small-tree", {}, fused(5)), ("generic", _GEN, fused(0))]


def test_the_overflow_row_overflows_under_the_direct_law():
    """no GPU.  The restatement over the row's own input: every interior (site, branch) of colour 0, its segments from
    the neighbours' paths, every segment conditioned on the states the site's own path has at the segment's ends (a
    proposal the sampler may well make: it is the current history), walked as the jump kernels walk a branch.
    Some branches must pass the room the capacity leaves -- under the direct law, which this is."""
    from direct_ref import OK, OVERFLOW as OVF, branch_segments, direct_segment
    model, tree, fp, cap = mc.workload(OVERFLOW_ROW)
    assert "model-overflow" in mc.row(OVERFLOW_ROW)[6] and cap <= 31
    n, B = fp.n_sites, fp.n_nodes - 1
    off, jumps = [int(x) for x in fp.offsets], fp.jumps.tolist()
    path = lambda e: jumps[off[e]:off[e + 1]]                                                        # noqa: E731
    walked = over = 0
    for site in range(3, n - 1, 3):
        for b in range(B):
            e = b * n + site
            own, segs = path(e), branch_segments(path(e - 1), fp.init[e - 1], path(e + 1), fp.init[e + 1],
                                                 float(tree.branches[b + 1]))
            cnt, passed, prev, outcome = 0, 0.0, int(fp.init[e]), OK
            for k, (length, trip0) in enumerate(segs):
                passed_end = passed + length
                upto = len(own) if k == len(segs) - 1 else sum(1 for t in own if t < passed_end)
                sampled = int(fp.init[e]) ^ (upto & 1)
                outcome, times, _, _ = direct_segment(23, site, 5, b + 1, k, prev, sampled, length, float(model.rates[trip0]),
                                                      float(model.rates[trip0 | 2]), cap - cnt, passed)
                if outcome != OK:
                    break
                cnt, prev, passed = cnt + len(times), sampled, passed_end
            walked += 1
            over += outcome == OVF
    print("branches walked", walked, "overflowed", over)
    assert walked >= 300 and over > 0, (walked, over)


@pytest.mark.gpu
@pytest.mark.parametrize("env,expect", [r[1:] for r in OVERFLOW], ids=[r[0] for r in OVERFLOW])
def test_overflow_inside_the_fused_body(env, expect):
    out = agrees_with_the_separate_kernels(dict(kind="family", input="row", rid=OVERFLOW_ROW, opts={}, expect=expect,
                                                overflows=True), env)
    assert out["overflow"] > 0, out


# ---------------------------------------------------------------------------------------------------------
# 4  the switch only changes the plan: (id, tree, n, options, what else the context holds).  None of these plans the
# fused phase in the default mode, so none may with the switch.
SWITCH = [
    ("unobserved", "tree", 1500, {}, dict(unobserved=True)),
    ("evidence", "tree", 1500, {}, dict(evidence=True)),
    ("reference-ratio", "tree", 1500, REF, {}),
    ("sample-root", "tree", 1500, SR, {}),
    ("bal16", "bal16", 600, {}, {}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("tree,n,opts,more", [r[1:] for r in SWITCH], ids=[r[0] for r in SWITCH])
def test_switch_changes_nothing_where_the_fused_phase_is_not_eligible(tree, n, opts, more):
    spec = dict(kind="family", input="matrix", tree=tree, n=n, opts=opts, expect={}, must_fuse=False, **more)
    on, off = child(dict(spec, fused=True)), child(dict(spec, fused=False))
    assert on["plan"] == off["plan"] and on["plan"]["direct"] and on["plan"]["propose"] != "fused", (on["plan"], off["plan"])
    for key in BITS:
        assert on[key] == off[key], key


@pytest.mark.gpu
def test_option_rules():
    import ctypes as C
    from common import simulate
    from epievo_amd.sampler import DeviceSampler, EpvError
    model, tree, fp = simulate("tree", 300, seed=8)
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, 16)

    def flags():
        v = C.c_uint32(0)
        d._ck(d.L.epv_get_options(d.h, C.byref(v)))
        return int(v.value)
    with pytest.raises(EpvError) as e:           # EPV_OPT_DIRECT_FUSED alone
        d._ck(d.L.epv_set_options(d.h, 16))
    assert e.value.code == 1 and "EPV_OPT_DIRECT_FUSED" in str(e.value) and "EPV_OPT_DIRECT_SAMPLER" in str(e.value)
    assert flags() == 0
    d.set_options(forward_rejection=True)        # with forward rejection, in either order of the calls
    with pytest.raises(EpvError) as e:
        d.set_direct_sampler(True, fused=True)
    assert e.value.code == 1 and flags() == 2
    d.set_options()
    d.set_direct_sampler(True, fused=True)
    assert flags() == 24
    with pytest.raises(EpvError) as e:
        d.set_options(forward_rejection=True)
    assert e.value.code == 1 and flags() == 24
    d.reset()
    plan = d.phase_plan()
    assert plan["direct"] and plan["propose"] == "fused" and plan["small_nn"] == 5, plan
    assert d.phase_mode() == 3
    d.set_options(reference_proposal_ratio=True)             # set_options keeps both bits
    assert flags() == 25 and d.phase_plan()["propose"] == "V1" and d.phase_plan()["direct"]
    d.set_options()
    assert flags() == 24 and d.phase_plan() == plan
    d.set_direct_sampler(True)                               # fused=False: the parent's direct mode
    assert flags() == 8 and d.phase_plan()["direct"] and d.phase_plan()["propose"] != "fused"
    d.set_direct_sampler(True, fused=True)
    d.set_direct_sampler(False)                              # clears both
    assert flags() == 0
    plan = d.phase_plan()
    assert not plan["direct"] and plan["propose"] == "fused"
    assert d.direct_giveups() == 0
    d.close()


# ---------------------------------------------------------------------------------------------------------
# 5  contexts
@pytest.mark.gpu
def test_switch_reaches_every_context_of_a_driver():
    spec = dict(kind="two_contexts", input="matrix", tree="tree", n=40000, expect={})
    on, off = child(dict(spec, fused=True)), child(dict(spec, fused=False))
    assert on["one"]["mode"] == 3 and on["two"]["mode"] == 3, on          # EPV_PHASE_FUSED on the largest part
    assert off["one"]["mode"] != 3 and off["two"]["mode"] != 3, off
    for key in ("paths", "stats", "acc"):
        assert on["one"][key] == on["two"][key], key
        assert on["one"][key] == off["one"][key] and off["one"][key] == off["two"][key], key


GROUP_N = 3301       # three contexts of 256-site halos fit; 1100 sites of a colour: a ragged last wave at 16, 32 and 64


@pytest.mark.gpu
def test_local_group_of_three_agrees_with_one_context():
    spec = dict(kind="group", input="matrix", tree="tree", n=GROUP_N, expect=fused(5))
    out = child(dict(spec, fused=True))
    assert out["one"] == out["three"], out
    sep = child(dict(kind="family", input="matrix", tree="tree", n=GROUP_N, opts={}, expect={}, fused=False),
                dict(_SEP, EPV_SEG_JUMPS="0"))
    for key in ("paths", "stats", "nacc"):
        assert sep[key] == out["one"][key], key


@pytest.mark.gpu
@pytest.mark.parametrize("program", ("epievo_est_histories", "epievo_est_params_histories"))
def test_cli_direct_fused_implies_direct_and_writes_the_same_files(tmp_path, program):
    """--direct-fused alone (it implies -j), -j -F and -j write the same bytes; the default mode writes others"""
    from common import simulate
    from epievo_amd import _build, host
    from epievo_amd.workloads import TEST_PARAM_TEXT, TREE_NWK_TEXT
    model, tree, fp = simulate("tree", 3000, seed=12)
    d = str(tmp_path)
    open(d + "/p.param", "w").write(TEST_PARAM_TEXT)
    open(d + "/t.nwk", "w").write(TREE_NWK_TEXT)
    host.write_paths(d + "/in.paths", tree.node_names, tree.branches, fp)
    outs = {}
    for tag, flags in (("default", []), ("direct", ["-j"]), ("fused", ["--direct-fused"]), ("both", ["-j", "-F"])):
        cmd = [os.path.join(_build.BIN_DIR, program), "-L", "2", "-B", "3", "-s", "17", "-o", "%s/%s.paths" % (d, tag)]
        if program == "epievo_est_params_histories":
            cmd += ["-i", "2", "-p", "%s/%s.param" % (d, tag)]
        r = subprocess.run(cmd + flags + [d + "/p.param", d + "/t.nwk", d + "/in.paths"], capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = open("%s/%s.paths" % (d, tag), "rb").read()
    assert outs["fused"] == outs["direct"] and outs["both"] == outs["direct"]
    assert outs["default"] != outs["direct"]


# ---------------------------------------------------------------------------------------------------------
# 6  the unrunnable row.  NEVER in another mode: there it is a kernel that does not return.
# Measured in one session on an MI355X (the session that added the fused direct bodies): the ratio-tree row of
# model_cases (the same model on its own data, n = 200, the same run_mcmc(2, 3) and checks, fused direct mode:
# direct_fused_gpu_child.py with kind "family", input "row", rid "ratio-tree", fused true, under EPV_FORCE_LDS_POOL=1,
# without which that row's denser data sends the record pool to global memory and the plan to the large-tree kernel)
# took 0.477, 0.336 and 0.307 s as a whole child process -- the interpreter's start, the imports and the context
# included; the yardstick is the slowest, the limit ten times that.
UNRUNNABLE_MEASURED_S = (0.477, 0.336, 0.307)
UNRUNNABLE_YARDSTICK_S = max(UNRUNNABLE_MEASURED_S)
UNRUNNABLE_LIMIT_S = 10.0 * UNRUNNABLE_YARDSTICK_S


@pytest.mark.gpu
def test_the_unrunnable_row_runs_in_the_fused_direct_body():
    assert mc.UNRUNNABLE == (("ref", "ratio", "tree", 300),)
    out = child(dict(kind="unrunnable", input="model_space", row=list(mc.UNRUNNABLE[0]), opts={}, fused=True,
                     expect=fused(5)), {}, UNRUNNABLE_LIMIT_S)
    print("seconds", out["seconds"])
    assert out["compared"] > 0 and out["nacc"] > 0 and out["plan"]["propose"] == "fused"


# ---------------------------------------------------------------------------------------------------------
# 7  the stationary law (the criteria of tests/test_mcmc_posterior.py and tests/test_direct_sampler.py); 31 jump slots,
# the most the fused phase takes -- the separate kernels' tests run 32 and 48, and no path here comes near either
@pytest.mark.gpu
@pytest.mark.parametrize("seed", (21, 22))
def test_fused_direct_chain_matches_exact_posterior_on_the_tree(seed):
    from common import ref_test_model
    from epievo_amd.sampler import DeviceSampler
    from test_mcmc_posterior import TROOT, _check_tree, _exact_tree, _tree_case
    model = ref_test_model()
    tree, leaf, fp = _tree_case()
    exact = _exact_tree(model, tree, leaf)
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, 31)
    d.set_direct_sampler(True, fused=True)
    d.reset()
    plan = d.phase_plan()
    assert plan["direct"] and plan["propose"] == "fused" and plan["small_nn"] == 5, plan
    J, D, nacc = d.run_mcmc(300, 12000, seed)
    _check_tree(J, D, 1200.0, exact, tree)
    p = d.paths()
    B, n = tree.n_nodes - 1, len(TROOT)
    es = (p.init.reshape(B, n) ^ (p.counts().reshape(B, n) & 1).astype(np.uint8))
    for b in range(1, tree.n_nodes):
        if tree.subtree_sizes[b] == 1:
            assert np.array_equal(es[b - 1], leaf[b])
    assert d.direct_giveups() == 0 and d.counters()["overflow"] == 0
    d.close()


@pytest.mark.gpu
def test_fused_direct_chain_matches_exact_posterior_on_a_weak_branch():
    from epievo_amd import host
    from epievo_amd.sampler import DeviceSampler
    from test_direct_sampler import WEAK_T, weak_check, weak_exact, weak_initial_paths, weak_model
    d = DeviceSampler(0)
    d.set_tree(host.Tree.single_branch(WEAK_T))
    d.set_model(weak_model())
    d.upload_paths(weak_initial_paths(), 31)
    d.set_direct_sampler(True, fused=True)
    d.reset()
    plan = d.phase_plan()
    assert plan["direct"] and plan["propose"] == "fused" and plan["small_nn"] == 2, plan
    J, D, nacc = d.run_mcmc(500, 20000, 99)
    weak_check(J, D, 2000.0, weak_exact())
    assert d.direct_giveups() == 0 and d.counters()["overflow"] == 0
    d.close()


# ---------------------------------------------------------------------------------------------------------
# 8  the tables
def test_rows_cover_what_they_claim():
    rows = [(r[0], r[4]) for r in FAMILY] + [(r[0], r[8]) for r in REPLAY if r[8] is not CANNOT]
    bodies = {e["small_nn"] for _, e in rows}
    lanes = {e["fused_lanes"] for _, e in rows}
    assert bodies == {0, 2, 3, 4, 5} and lanes == {16, 32, 64}, (bodies, lanes)
    assert {(e["small_nn"], e["fused_lanes"]) for _, e in rows} >= {(0, 16), (0, 32), (0, 64), (5, 16), (5, 32), (5, 64)}
    assert all(e["propose"] == "fused" and e["jumps"] == "fused" and e["accept"] == "fused" for _, e in rows)
    assert len({r[0] for r in FAMILY}) == len(FAMILY) and len({r[0] for r in REPLAY}) == len(REPLAY)
    # the body a row names is the one its tree and knobs select
    for r in FAMILY:
        nodes = make_tree(r[1]).n_nodes
        small = r[3].get("EPV_P2_SMALL_TREE", "1") != "0" and 2 <= nodes <= 5
        assert r[4]["small_nn"] == (nodes if small else 0), r[0]
        assert r[4]["fused_lanes"] == int(r[3].get("EPV_FUSED_LANES", 16)), r[0]
    # every row has its separate-kernel partners: a family row runs them itself, with the fused phase off and no knob
    # of the fused phase left; a replay row's workload is replayed through the separate kernels by the direct
    # sampler's own table, with the same colours and floor
    for r in FAMILY + [(o[0], OVERFLOW_ROW, 0, o[1], o[2]) for o in OVERFLOW]:
        ps = partners(r[3])
        assert [p["EPV_SEG_JUMPS"] for p in ps] == ["0", "1"], r[0]
        assert all(p["EPV_FUSED_PHASE"] == "0" and not set(p) & set(_FUSED_KNOBS[1:]) for p in ps), r[0]
    theirs = {(t[1], t[2], tuple(t[3]), t[4], t[5]) for t in base.REPLAY}
    for r in REPLAY:
        assert (r[1], r[2], tuple(r[3]), r[4], r[5]) in theirs, r[0]
    assert {r[1] for r in REPLAY} == {t[1] for t in base.REPLAY}          # no workload dropped
