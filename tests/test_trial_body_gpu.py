"""GPU part of tests/test_trial_body.py: the trial evaluator with one Philox block per first draw.

  * known answers (epv_trial_kat): first_draw, the single-trial scan the grouped search calls, run_trial and
    scan_trials over 1, 4 and 8 trials, in the form the fused bodies inline, in a kernel of their own on the
    generator's cases -- the lanes of a wave mix flips with keepers and t == 1 with t >= 2.
    Outcome, winning trial, jump count, the first two times and M equal the restatement bit for bit;
  * whole runs against the oracle's parallel rung (rung B), bit for bit -- paths, cached triple likelihoods,
    J, D, the accept count and the overflow counter -- on the fused small-tree body, the generic fused body
    and the separate kernels, each asserted to be what ran: tree.nwk n = 193 (a partial last wave), n = 1000
    with the dense jump window at capacity 4, and the single branch n = 257 (several jumps per trial, many
    trials);
  * forward-rejection mode on tree.nwk n = 193, one burn-in and one batch sweep (the oracle's trial count
    of that run is capped in the CPU part).
What these runs rest on (flips and keepers, second trials, overflow not everywhere) is asserted from the
oracle alone in tests/test_trial_body.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))


def test_trial_kat_equals_the_restatement():
    import test_trial_body as T
    from epievo_amd.sampler import DeviceSampler
    cases = T.trial_cases()
    items = np.array([[c["site"], c["sweep"], c["node"], c["k"], c["t0"], c["room"],
                       c["a0"] | c["end"] << 1 | int(c["nielsen"]) << 2, 0] for c in cases], np.uint32)
    reals = np.array([[c["T"], c["r0"], c["r1"], c["trunc"], c["u0"], c["start"]] for c in cases])
    d = DeviceSampler(0)
    W, first, times = d.trial_kat(T.KAT_SEED, items, reals)
    d.close()
    names = ("scan_trial1", "run_trial", "scan_trials W=1", "scan_trials W=4", "scan_trials W=8")
    bad = []

    def bits(x):
        return np.float64(x).view(np.uint64)
    for i, c in enumerate(cases):
        u, rows = T.expected(c)
        if bits(first[i]) != bits(u):
            bad.append((i, "first_draw", first[i], u))
        for e, (oc, t, nj, mm, t0, t1) in enumerate(rows):
            got = [int(x) for x in W[i, e]]
            ok = got[0] == oc and got[3] == mm
            if t is not None:        # (a scan that fails names no trial; its count and times are not read)
                ok = ok and got[1] == t and got[2] == nj
                ok = ok and all(bits(times[i, e, q]) == bits((t0, t1)[q]) for q in range(min(nj, 2)))
            if not ok:
                bad.append((i, names[e], got, times[i, e].tolist(), (oc, t, nj, mm, t0, t1), c))
    assert W.shape == (len(cases), 5, 4) and not bad, "%d differ, first: %r" % (len(bad), bad[0] if bad else None)


_CODE = r'''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import orc
from epievo_amd.sampler import DeviceSampler
import test_trial_body as T
model, tree, fp, cap = T.run_inputs(%(name)r)
path, fr = %(path)r, %(fr)r
seed = T.FR_SEED if fr else T.RUN_SEED
burn, batch = (1, 1) if fr else (1, 2)
d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap)
d.set_options(forward_rejection=fr)
d.reset()
plan = d.phase_plan()
if path == "separate":
    assert d.phase_mode() != 3 and plan["propose"] != "fused" and plan["jumps"] != "fused", (d.phase_mode(), plan)
else:
    assert d.phase_mode() == 3 and plan["propose"] == "fused" and plan["jumps"] == "fused", (d.phase_mode(), plan)
    assert plan["small_nn"] == (tree.n_nodes if path == "small" else 0), plan
d.auto_grow = True       # (an overflow leaves a valid chain and complete outputs; this only keeps run_mcmc from raising)
J, D, nacc = d.run_mcmc(burn, batch, seed)
o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
o.set_sampler(fr)
o.reset()
Jo, Do, no, _ = o.run_mcmc(burn, batch)
cnt = d.counters()
print("nacc", nacc, no, "overflow", cnt["overflow"], o.counters()["overflow"], "plan", plan, flush=True)
assert nacc == no and no > 0, (nacc, no)
assert cnt["overflow"] == o.counters()["overflow"], (cnt, o.counters())
assert orc.paths_equal(d.paths(), o.paths())
assert np.array_equal(d.tri_llh().view(np.uint64), o.tri_llh().view(np.uint64))
assert np.array_equal(J, Jo) and np.array_equal(D.view(np.uint64), Do.view(np.uint64))
d.close()
print("ok")
'''

_ENV = {"small": {"EPV_FUSED_PHASE": "1"}, "generic": {"EPV_FUSED_PHASE": "1", "EPV_P2_SMALL_TREE": "0"},
        "separate": {"EPV_FUSED_PHASE": "0"}}


def _run(name, path, fr):
    code = _CODE % dict(root=_ROOT, tests=_TESTS, name=name, path=path, fr=fr)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **_ENV[path]), capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1500:] + r.stderr[-2000:]


@pytest.mark.parametrize("path", ["small", "generic", "separate"])
@pytest.mark.parametrize("name", ["tree193", "tree-window", "pair257"])
def test_whole_run_equals_rung_b(name, path):
    _run(name, path, False)


def test_forward_rejection_run_equals_rung_b():
    _run("tree193", "small", True)
