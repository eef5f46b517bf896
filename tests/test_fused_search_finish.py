"""The fused colour phase lets the grouped segment search finish a branch whose sole dirty segment it has
settled (epv_jumps2.h) and skips the assembly stage for a wave all of whose branches were finished that
way.  That may not change a bit: every case runs the GPU against the oracle's parallel rung and
compares paths (read through each site's buffer selector, so the selectors are compared with them),
cached triple likelihoods, J, D, and the accept and overflow counters, and asserts the kernels that ran.  The cases cover what sends a branch to the search's
own finish and what must fall back to the assembly: several dirty segments per branch and replays
of long trials (pair), a capacity that overflows (M > C), short lists with eight lanes per segment,
lists the grouped search gives up on after it has finished some branches (forward rejection), every
small-tree body and the generic one."""
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
tiny, fr, small = %(tiny)r, %(fr)r, %(small)r
cap = int(fp.counts().max()) if tiny else int(max(16, 2 * fp.counts().max() + 8))

d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap)
d.set_options(forward_rejection=fr)
d.reset()
plan = d.phase_plan()
assert d.phase_mode() == 3 and plan["propose"] == "fused" and plan["jumps"] == "fused" and plan["accept"] == "fused", plan
assert plan["small_nn"] == (tree.n_nodes if small else 0), plan
o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=29)
o.set_sampler(fr)
o.reset()
if tiny:
    for w in range(3):
        try:
            d.sweep(1, 29, sweep_base=w)
        except Exception:
            pass
        o.sweep(w)
else:
    J, D, nacc = d.run_mcmc(2, 3, 29, sweep_base=3)
    Jo, Do, no, _ = o.run_mcmc(2, 3, sweep_base=3)
    assert nacc == no, (nacc, no)
    assert np.array_equal(J.view(np.uint64), Jo.view(np.uint64)) and np.array_equal(D.view(np.uint64), Do.view(np.uint64))
cnt = d.counters()
print("counters", cnt, flush=True)
assert orc.paths_equal(d.paths(), o.paths())
assert np.array_equal(d.tri_llh().view(np.uint64), o.tri_llh().view(np.uint64))
assert cnt["overflow"] == o.counters()["overflow"], (cnt, o.counters())
assert (cnt["overflow"] > 0) == bool(tiny), cnt
assert cnt["search_finished"] <= cnt["coop_tasks"], cnt
if %(some)r:      # the search finishes branches, and not all of them
    assert 0 < cnt["search_finished"] < cnt["coop_tasks"], cnt
d.close()
print("ok")
'''

_SMALL_OFF = {"EPV_P2_SMALL_TREE": "0"}


@pytest.mark.parametrize("cfg,n,tiny,fr,small,env,some", [
    ("tree", 3000, False, False, True, {}, True),
    ("tree", 20011, False, False, True, {}, False),                 # n not a multiple of 192
    ("tree", 20011, False, False, True, {"EPV_FUSED_LANES": "16"}, False),   # short lists, G = 8
    ("tree", 5000, True, False, True, {}, False),                   # M > C: the assembly overflows as the oracle does
    ("pair", 9001, False, False, True, {}, False),                  # T = 1: several dirty segments, cnt > 2 replays
    ("pair", 4000, True, False, True, {}, False),
    ("star4", 3001, False, False, True, {}, False),
    ("cherry", 3001, False, False, True, {}, False),
    # generic body (more than five nodes).  cat6's worst-case record pool is beyond the plan's LDS
    # bound, which would send it to the large-tree kernels: the pool is forced into LDS, as in
    # test_kernel_matrix.py's fused cat6 row; star5 (six nodes) takes the generic body by default
    ("cat6", 3001, False, False, False, {"EPV_FORCE_LDS_POOL": "1"}, False),
    ("star5", 3001, False, False, False, {}, False),
    ("tree", 3000, False, False, False, _SMALL_OFF, False),         # generic body on the 5-node tree
    ("tree", 3000, False, True, True, {}, False),                   # forward rejection: long trial tails
])
def test_search_finish_equals_oracle(cfg, n, tiny, fr, small, env, some):
    code = _CODE % dict(root=_ROOT, tests=_TESTS, cfg=cfg, n=n, tiny=tiny, fr=fr, small=small, some=some)
    e = dict(os.environ, EPV_FUSED_PHASE="1", **env)
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1500:] + r.stderr[-2000:]
