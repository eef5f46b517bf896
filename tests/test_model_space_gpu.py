"""Every colour-phase kernel family under models far from test.param and under models that did not generate the
data (model_cases.py), against the oracle's parallel rung B bit for bit.

Each case of model_cases.gpu_cases() runs in a fresh process with its knobs in the environment, as the rows of
test_kernel_matrix.py do, with that module's plan helpers and its comparison: the plan is asserted after reset(),
then run_mcmc(2, 3, seed, sweep_base=4) is compared with rung B on J, D, the accept count, the paths, the cached
likelihoods as bit patterns and the overflow counter.  The first case of a row then runs the row once with
reference_proposal_ratio and, where the row is labelled fr, once with forward_rejection.

The rows come from model_cases.gpu_cases() only.  test_model_space.py asserts the work bound (trials / segments
<= 64 on the oracle) for every one of them in every mode; each child repeats that check on its own oracle run
BEFORE it creates a device context, so an input whose rejection search has no end cannot reach a kernel."""
import json
import os
import subprocess
import sys

import pytest

import model_cases as mc

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))

_HEAD = r'''
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import orc, model_cases as mc
spec = json.loads(%(spec)r)
'''

_CODE = _HEAD + r'''
rid, expect = spec["row"], spec["expect"]
model, tree, fp, cap = mc.workload(rid)
overflows = "model-overflow" in mc.row(rid)[6]
# the oracle first: nothing goes to the device unless its run of the same input meets the work bound
want = []
for opts in spec["modes"]:
    o = mc.oracle(rid, opts)
    llh0 = o.tri_llh()
    Jo, Do, no, _ = o.run_mcmc(2, 3, sweep_base=4)
    c = o.counters()
    assert mc.work(c) <= mc.WORK_BOUND, (rid, opts, c)
    want.append((llh0, Jo, Do, no, o.paths(), o.tri_llh(), c["overflow"]))
from epievo_amd.sampler import DeviceSampler
for opts, (llh0, Jo, Do, no, paths, llh, ovf) in zip(spec["modes"], want):
    d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap); d.set_options(**opts); d.reset()
    plan = d.phase_plan()
    if not opts:
        bad = dict((k, (v, plan[k])) for k, v in expect.items() if plan[k] != v)
        assert not bad, "plan differs (expected, got): %%r; plan %%r" %% (bad, plan)
    elif opts.get("reference_proposal_ratio"):
        assert plan["refq"] and plan["propose"] == "V1", plan
    else:
        assert plan["jumps"] != "jumps_all", plan        # forward rejection has kernels of its own
    assert np.array_equal(d.tri_llh().view(np.uint64), llh0.view(np.uint64))
    d.auto_grow = True      # (an overflow leaves a valid chain and complete outputs; this only keeps run_mcmc from raising)
    Jd, Dd, nd = d.run_mcmc(2, 3, mc.ORACLE_SEED, sweep_base=4)
    assert nd == no, (opts, nd, no)
    assert np.array_equal(Jd, Jo) and np.array_equal(Dd, Do), opts
    assert orc.paths_equal(d.paths(), paths), opts
    assert np.array_equal(d.tri_llh().view(np.uint64), llh.view(np.uint64)), opts
    assert d.counters()["overflow"] == ovf and (ovf > 0) == overflows, (opts, d.counters(), ovf)
    if not ovf:        # (an absorbed overflow doubles the capacity, and the wider slots may take another plan)
        assert d.phase_plan() == plan
    print("result", json.dumps(dict(row=rid, opts=opts, propose=plan["propose"], small_nn=plan["small_nn"], jumps=plan["jumps"],
          accept=plan["accept"], accepted=nd, overflow=ovf)), flush=True)
    d.close()
print("ok")
'''

# one context through set_model over ref -> fast -> slow -> mixed -> ref, scale_jump_times in between: the held
# matrix table, the logs of the rates and the host-side bounds are rebuilt
_CHANGING = _HEAD + r'''
import test_model_space as tms
tree, fp = tms.changing_models_input()
o = orc.Oracle(tree, mc.model("ref"), fp, "B", cap=tms.SEQUENCE_CAP, seed=mc.ORACLE_SEED)
want = tms.changing_models(o, tree)
assert mc.work(o.counters()) <= mc.WORK_BOUND, o.counters()
from epievo_amd.sampler import DeviceSampler
d = DeviceSampler(0); d.set_tree(tree); d.set_model(mc.model("ref")); d.upload_paths(fp, tms.SEQUENCE_CAP)
d.auto_grow = True
got = tms.changing_models(d, tree, mc.ORACLE_SEED)
assert len(got) == len(want) == len(tms.SEQUENCE)
for i, ((Jd, Dd, nd, pd, ld, cd), (Jo, Do, no, po, lo, co)) in enumerate(zip(got, want)):
    assert nd == no and cd == co, (i, nd, no, cd, co)
    assert np.array_equal(Jd, Jo) and np.array_equal(Dd, Do), i
    assert orc.paths_equal(pd, po), i
    assert np.array_equal(ld.view(np.uint64), lo.view(np.uint64)), i
assert d.counters()["overflow"] == o.counters()["overflow"] > 0
d.close()
print("ok")
'''

# the fast row at the input's own maximum jump count: the overflow decisions of the sequential sampler (the cap2
# block of test_kernel_matrix.py)
_TIGHT = _HEAD + r'''
rid = "fast-tree"
model, tree, fp, cap = mc.workload(rid)
cap2 = int(fp.counts().max())
o2 = mc.oracle(rid, cap=cap2, seed=23)
want = []
for w in range(2):
    o2.sweep(w)
    want.append((o2.paths(), o2.tri_llh()))
assert mc.work(o2.counters()) <= mc.WORK_BOUND and o2.counters()["overflow"] > 0, o2.counters()
from epievo_amd.sampler import DeviceSampler
d2 = DeviceSampler(0); d2.set_tree(tree); d2.set_model(model); d2.upload_paths(fp, cap2); d2.reset()
plan2 = d2.phase_plan()
bad = dict((k, (v, plan2[k])) for k, v in spec["expect"].items() if plan2[k] != v)
assert not bad, "plan differs (expected, got): %%r; plan %%r" %% (bad, plan2)
for w in range(2):
    try:
        d2.sweep(1, 23, sweep_base=w)
    except Exception as e:
        assert "rejected" in str(e) or "capacity" in str(e).lower(), e
    assert orc.paths_equal(d2.paths(), want[w][0]), "paths differ after overflow sweep %%d" %% w
    assert np.array_equal(d2.tri_llh().view(np.uint64), want[w][1].view(np.uint64)), w
assert d2.counters()["overflow"] == o2.counters()["overflow"] > 0
d2.close()
print("ok")
'''


def _run(code, spec, env):
    src = code % dict(root=_ROOT, tests=_TESTS, spec=json.dumps(spec))
    try:
        r = subprocess.run([sys.executable, "-c", src], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.exit("a child did not return within 300 s: nothing more is started on this GPU\n%s" % e, returncode=3)
    print(r.stdout[-3000:])
    if r.returncode < 0 or r.returncode in (134, 139):
        # killed by a signal, not a failed comparison: the device may be in a bad state, so the session ends here
        pytest.exit("a child died with status %d: nothing more is started on this GPU\n%s"
                    % (r.returncode, r.stderr[-3000:]), returncode=3)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


CASES = mc.gpu_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("rid,env,expect,modes", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_model_row_matches_rung_b(rid, env, expect, modes):
    _run(_CODE, dict(row=rid, expect=expect, modes=modes), env)


@pytest.mark.gpu
def test_changing_models_in_one_context():
    _run(_CHANGING, {}, {})


@pytest.mark.gpu
@pytest.mark.parametrize("family", [f[0] for f in mc.families("tree")])
def test_model_overflow_at_tight_capacity(family):
    fam, env, expect = [f for f in mc.families("tree") if f[0] == family][0]
    _run(_TIGHT, dict(expect=dict(propose=expect["propose"])), env)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("anti", "mixed"))
def test_gpu_chain_matches_exact_posterior(name):
    """the twin of test_mcmc_posterior.test_gpu_chain_matches_exact_posterior under a model other than test.param:
    same chain length, seed and criteria; the leaf pattern per model is test_model_space.LAW_LEAF"""
    import test_model_space as tms
    from epievo_amd import host
    from epievo_amd.sampler import DeviceSampler
    from test_mcmc_posterior import T_BRANCH, _check
    exact, start = tms.law_case(name)
    d = DeviceSampler(0)
    d.set_tree(host.Tree.single_branch(T_BRANCH))
    d.set_model(mc.model(name))
    d.upload_paths(start, 48)
    d.reset()
    J, D, nacc = d.run_mcmc(500, 20000, 99)
    d.close()
    _check(J, D, 2000.0, exact)
