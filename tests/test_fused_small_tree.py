"""The fused colour phase's small-tree body (epv_propose2.h, NN = node count, EPV_P2_SMALL_TREE) must
compute what the generic body computes, bit for bit, and both what the oracle's parallel rung computes
(trees of 2, 3, 4 and 5 nodes, each asserted to run the body it names):
paths, buffer selectors, cached triple likelihoods, J, D and the accept and overflow counters."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))

_CODE = r'''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import orc
from common import simulate
from epievo_amd.sampler import DeviceSampler
model, tree, fp = simulate(%(cfg)r, %(n)d, seed=8)
cap = int(max(16, 2 * fp.counts().max() + 8)) if not %(tiny)r else int(fp.counts().max())

def run(knob):
    os.environ["EPV_P2_SMALL_TREE"] = knob       # read when a context is created
    d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap); d.reset()
    assert d.phase_mode() == 3
    plan = d.phase_plan()       # the body that runs: NN = the node count, or 0 for the generic body
    assert plan["propose"] == "fused" and plan["small_nn"] == (tree.n_nodes if knob == "1" else 0), plan
    if %(tiny)r:
        for w in range(3):
            try:
                d.sweep(1, 29, sweep_base=w)
            except Exception:
                pass
        out = dict(paths=d.paths(), tri=d.tri_llh(), cnt=d.counters())
    else:
        J, D, nacc = d.run_mcmc(2, 3, 29, sweep_base=3)
        out = dict(J=J, D=D, nacc=nacc, paths=d.paths(), tri=d.tri_llh(), cnt=d.counters())
    d.close()
    return out

a, b = run("0"), run("1")
assert orc.paths_equal(a["paths"], b["paths"])
assert np.array_equal(a["tri"].view(np.uint64), b["tri"].view(np.uint64))
assert a["cnt"] == b["cnt"], (a["cnt"], b["cnt"])
o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=29); o.reset()
if %(tiny)r:
    for w in range(3):
        o.sweep(w)
    assert b["cnt"]["overflow"] == o.counters()["overflow"] and b["cnt"]["overflow"] > 0
else:
    assert np.array_equal(a["J"], b["J"]) and np.array_equal(a["D"], b["D"]) and a["nacc"] == b["nacc"]
    Jo, Do, no, _ = o.run_mcmc(2, 3, sweep_base=3)
    assert b["nacc"] == no and np.array_equal(b["J"], Jo) and np.array_equal(b["D"], Do)
    assert np.array_equal(b["tri"], o.tri_llh())
assert orc.paths_equal(b["paths"], o.paths())
print("ok")
'''


@pytest.mark.parametrize("cfg,n,tiny,env", [
    ("tree", 3000, False, {}),
    ("tree", 20011, False, {}),                      # n not a multiple of 192
    ("tree", 20011, False, {"EPV_FUSED_LANES": "16"}),
    ("tree", 5000, True, {}),                        # a capacity that overflows
    ("pair", 9001, False, {}),
    ("pair", 4000, True, {}),
    ("star4", 3001, False, {}),
    ("star4", 3000, False, {"EPV_FUSED_LANES": "16"}),
    ("star4", 3000, True, {}),
    ("cherry", 3001, False, {}),                     # 3 nodes
    ("cherry", 3000, False, {"EPV_FUSED_LANES": "16"}),
    ("cherry", 12001, True, {}),
    ("star3", 3001, False, {}),                      # 4 nodes
    ("star3", 3000, False, {"EPV_FUSED_LANES": "16"}),
    ("star3", 20000, True, {}),
])
def test_small_tree_body_equals_generic_and_oracle(cfg, n, tiny, env):
    code = _CODE % dict(root=_ROOT, tests=_TESTS, cfg=cfg, n=n, tiny=tiny)
    e = dict(os.environ, EPV_FUSED_PHASE="1", **env)
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
