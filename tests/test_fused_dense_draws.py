"""The fused colour phase with the acceptance stage's first-jump loads issued in one batch (small-tree body:
triple_llh_cached<NB > 0> loads the first jump of all 3 NB columns before the first merge; later jumps stay
on demand): every result must still be the parallel rung's (oracle rung B), bit for bit -- paths, cached
triple likelihoods, J, D, the accept count and the overflow counter -- with the small-tree body and with the
generic one, each asserted to be the body that ran.

  * a window of sites 384 .. 479 carrying jumps, at capacity 4, n = 1000, run_mcmc(1, 2), three contents:
      - 2 or 3 jumps on every branch: every column of a triple has later jumps behind its batched first one,
        K = 5 .. 7 segments, several rounds of the LDS pool;
      - 4 jumps on three sites of four, none on the fourth: full columns next to empty ones, K up to
        2 C + 1 = 9;
      - 0, 1, 2 or 3 jumps side by side: batched first loads with later jumps on demand, and triples in
        which a column is empty (its load is predicated off and the merge starts from +inf);
    on tree.nwk (5 nodes, NB = 4), the single branch (2 nodes, NB = 1) and the 6-leaf caterpillar (11 nodes:
    the generic body and the uncached acceptance whatever the knob says).  The overflow counter is 0 on
    tree.nwk and several hundred on the single branch: equal to the oracle's everywhere, which pins the
    overflow decision and the acceptance's skip of an overflowed site;
  * n = 193 with simulated histories: a partial last wave and the genome-edge triples that are skipped.

(The dense evaluation of the heavy branches' end-state draws that was tried together with this change was
not kept -- DESIGN.md section 4.1 -- and its exact-zero case went with it.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))

SEEDS = (31, 0xFFFFFFFF9E3779B9)
WIN_N, WIN_LO, WIN_HI, WIN_CAP = 1000, 384, 479, 4

# jumps of (site, node) inside the window
WINDOW_COUNTS = {
    "rounds": lambda site, node: 2 + (site + node) % 2,
    "full": lambda site, node: np.where(site % 4 != 1, 4, 0),
    "mixed": lambda site, node: (7 * site + 3 * node) % 4,
}


def window_paths(tree, n, lo, hi, seed, count):
    """FlatPaths with count(site, node) jumps on the branches of the sites lo .. hi and none elsewhere, at
    sorted uniform times inside the branch; the start state of a branch is the
    end state of its parent's, the root states are random"""
    from epievo_amd import host
    rng = np.random.RandomState(seed)
    N = tree.n_nodes
    parent = [int(p) for p in tree.parent_ids]
    T = [float(x) for x in tree.branches]
    site = np.arange(n)
    root = rng.randint(0, 2, n).astype(np.uint8)
    init = np.zeros((N - 1, n), np.uint8)
    cnt = np.zeros((N - 1, n), np.int64)
    end = {0: root}
    for node in range(1, N):
        init[node - 1] = end[parent[node]]
        cnt[node - 1] = np.where((site >= lo) & (site <= hi), count(site, node), 0)
        end[node] = init[node - 1] ^ (cnt[node - 1] & 1).astype(np.uint8)
    off = np.zeros((N - 1) * n + 1, np.uint64)
    off[1:] = np.cumsum(cnt.reshape(-1))
    jumps = []
    for node in range(1, N):
        for s in range(n):
            k = int(cnt[node - 1, s])
            if k:
                jumps.extend(np.sort(rng.uniform(0.05, 0.95, k)) * T[node])
    return host.FlatPaths(n, N, init.reshape(-1), off, np.array(jumps))


_CODE = r'''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import orc
from common import simulate, config, ref_test_model
from epievo_amd.sampler import DeviceSampler
import test_fused_dense_draws as T
seed, kind, n = %(seed)d, %(kind)r, %(n)d
model, tree = ref_test_model(), config(%(cfg)r)
if kind == "simulated":
    model, tree, fp = simulate(%(cfg)r, n, seed=8)
    cap = int(max(16, 2 * fp.counts().max() + 8))
else:
    fp = T.window_paths(tree, n, T.WIN_LO, T.WIN_HI, 5, T.WINDOW_COUNTS[kind])
    cap = T.WIN_CAP
    cnt = fp.counts().reshape(tree.n_nodes - 1, -1)
    assert cnt.max() <= cap and cnt[:, T.WIN_LO:T.WIN_HI + 1].max() >= 3 and cnt[:, :T.WIN_LO].max() == 0
small = tree.n_nodes if tree.n_nodes <= 5 else 0

def run(knob):
    os.environ["EPV_P2_SMALL_TREE"] = knob       # read when a context is created
    d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap); d.reset()
    assert d.phase_mode() == 3                    # EPV_PHASE_FUSED
    plan = d.phase_plan()
    assert plan["propose"] == "fused" and plan["small_nn"] == (small if knob == "1" else 0), plan
    # (an overflow -- expected on the single branch and the caterpillar at capacity 4 -- leaves a valid chain and
    # complete outputs; auto_grow only keeps run_mcmc from raising, the wider slots would serve later calls)
    d.auto_grow = True
    J, D, nacc = d.run_mcmc(1, 2, seed)
    out = dict(J=J, D=D, nacc=nacc, paths=d.paths(), tri=d.tri_llh(), cnt=d.counters())
    d.close()
    return out

o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed); o.reset()
Jo, Do, no, _ = o.run_mcmc(1, 2)
ovf = o.counters()["overflow"]
print("oracle: nacc %%d overflow %%d" %% (no, ovf))
if %(cfg)r == "tree":
    assert ovf == 0
for knob in ("1", "0"):
    r = run(knob)
    print("knob %%s: nacc %%d overflow %%d coop %%d" %% (knob, r["nacc"], r["cnt"]["overflow"], r["cnt"]["coop_tasks"]))
    assert r["nacc"] == no and no > 0, (knob, r["nacc"], no)
    assert r["cnt"]["overflow"] == ovf, (knob, r["cnt"], ovf)
    assert orc.paths_equal(r["paths"], o.paths()), knob
    assert np.array_equal(r["tri"].view(np.uint64), o.tri_llh().view(np.uint64)), knob
    assert np.array_equal(r["J"], Jo) and np.array_equal(r["D"].view(np.uint64), Do.view(np.uint64)), knob
print("ok")
'''


# inputs whose record pool the default plan does not keep in LDS (jump density of "full" on tree.nwk, node
# count of cat6) and which it therefore gives to other kernels: EPV_FORCE_LDS_POOL
# keeps the pool in LDS, as test_kernel_matrix.py and test_dense_histories_gpu.py do for the same reason.  Every
# other case runs under the default plan, whose smaller pool is what makes a wave take several rounds.
def _needs_lds_knob(cfg, kind):
    return cfg == "cat6" or (cfg == "tree" and kind == "full")


def _run(cfg, n, seed, kind):
    code = _CODE % dict(root=_ROOT, tests=_TESTS, cfg=cfg, n=n, seed=seed, kind=kind)
    e = dict(os.environ, EPV_FUSED_PHASE="1")
    if _needs_lds_knob(cfg, kind):
        e["EPV_FORCE_LDS_POOL"] = "1"
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind", sorted(WINDOW_COUNTS))
@pytest.mark.parametrize("cfg", ["tree", "pair", "cat6"])
def test_window_of_jumps(cfg, kind, seed):
    _run(cfg, WIN_N, seed, kind)


@pytest.mark.parametrize("cfg", ["tree", "pair"])
def test_partial_wave_and_genome_edges(cfg):
    _run(cfg, 193, SEEDS[0], "simulated")
