"""Memory round trips taken off the chain of the fused colour phase's small-tree bodies (epv_propose2.h), each
held to the oracle's parallel rung B bit for bit -- paths, J and D of every batch sweep and their sum, the accept
count -- with the plan asserted in every process (fused phase, the body, the width):

  pruning    the tree's shape comes from the topology word (leaf bit, parent field), not from S.subtree[]: every
             small-tree topology with a different child walk -- cherry, star3, star4, tree and the mirror of tree, whose
             internal node comes last in pre-order (its children are the last two nodes, node 1 is a leaf) -- at 64
             and 16 sites per wave
  accept     the overflow flag stays in the wave's LDS and the acceptance reads the meta words where the head put
             them: capacities that overflow in the assembly (rejected sites next to others in one wave, the overflow
             counter equal to the oracle's and non-zero), dense histories (weak-tree40) at 16 and 64 lanes, genomes
             of 4 and 5 sites (the left or right outer triple is skipped), and star5 with the generic body, which
             keeps the copy of the words into the lane's own cache

Without a GPU the oracle's side of every case runs here, with the conditions on the inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
import test_fused_head_batch as hb
from common import _tmp, config, ref_test_model, simulate
from epievo_amd import host

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))

MIRROR_NWK = "(F:0.1,(C:0.03,D:0.06)E:0.02)G:0.0;\n"
# (tree, node count = the small-tree body)
SHAPES = (("cherry", 3), ("star3", 4), ("star4", 5), ("tree", 5), ("mirror", 5))
SHAPE_N = 257                 # 85 sites per colour: one full wave and a part of one at 64 lanes, six waves at 16
OVERFLOW_N, OVERFLOW_SWEEPS, OVERFLOW_SIM_SEED = 600, 3, 8
GENERIC = ("star5", 0, 257)


def tree_of(name):
    if name == "mirror":
        return host.Tree.read(_tmp("mirror.nwk", MIRROR_NWK))
    return config(name)


def make_input(tree_name, n):
    model, tree = ref_test_model(), tree_of(tree_name)
    fp = host.simulate(model, tree, n, hb.SIM_SEED)
    return model, tree, fp, int(max(16, 2 * fp.counts().max() + 8))


def overflow_input():
    """the rule of the overflowing rows of test_fused_small_tree.py: the capacity is the input's own largest count"""
    model, tree, fp = simulate("tree", OVERFLOW_N, seed=OVERFLOW_SIM_SEED)
    return model, tree, fp, int(fp.counts().max())


def overflow_oracle(tree, model, fp, cap, seed):
    """OVERFLOW_SWEEPS sweeps site by site in the order of the colour phases -> (paths, overflow counter, per phase
    the list of (site, overflowed))"""
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    o.reset()
    phases = []
    for w in range(OVERFLOW_SWEEPS):
        for c in range(3):
            rows = []
            for s in hb.colour_sites(fp.n_sites, c):
                before = o.counters()["overflow"]
                o.mh_site(s, w)
                rows.append((s, o.counters()["overflow"] > before))
            phases.append(rows)
    out = o.paths(), o.counters()["overflow"], phases
    o.close()
    return out


def mixed_waves(phases, L):
    """phases in which some wave of L sites has an overflowed site next to one that did not overflow"""
    hits = 0
    for rows in phases:
        f = [x for _, x in rows]
        hits += any(f[i] != f[i + 1] and i // L == (i + 1) // L for i in range(len(f) - 1))
    return hits


_CHILD = r'''
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import orc
import test_fused_head_batch as hb
import test_fused_chain_trips as ct
from epievo_amd.sampler import DeviceSampler
spec = json.loads(%(spec)r)

def device(model, tree, fp, cap, small_nn, L):
    os.environ["EPV_FUSED_LANES"] = str(L)       # read when a context is created
    d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap)
    d.reset()
    plan = d.phase_plan()
    assert plan["propose"] == "fused" and plan["small_nn"] == small_nn and plan["fused_lanes"] == L, plan
    return d

def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)

def check(label, d, expect):
    J, D, nacc, paths, per_sweep = expect
    counts, got = d.run_mcmc_counts(hb.BURN_IN, hb.BATCH, spec["seed"], sweep_base=hb.BASE)[:2]
    print(label, "accepted", got, "oracle", nacc, flush=True)
    assert got == nacc, (label, got, nacc)
    assert orc.paths_equal(d.paths(), paths), (label, "paths")
    for k, (Jk, Dk) in enumerate(per_sweep):
        Jd, Dd = d.counts_to_stats(counts[k:k + 1], 1)
        assert np.array_equal(Jd, Jk) and np.array_equal(bits(Dd), bits(Dk)), (label, "batch sweep", k)
    Jd, Dd = d.counts_to_stats(counts, hb.BATCH)
    assert np.array_equal(Jd, J) and np.array_equal(bits(Dd), bits(D)), (label, "totals")
    d.close()

for case in spec["cases"]:
    kind, name, nn, L = case["kind"], case["tree"], case["small_nn"], case["width"]
    label = "%%s %%s L=%%d n=%%s" %% (kind, name, L, case.get("n"))
    if kind == "plain":
        model, tree, fp, cap = ct.make_input(name, case["n"])
        check(label, device(model, tree, fp, cap, nn, L), hb.oracle_run(tree, model, fp, cap, spec["seed"]))
    elif kind == "dense":
        model, tree, fp, cap = hb.dense_input()
        check(label, device(model, tree, fp, cap, nn, L), hb.oracle_run(tree, model, fp, cap, spec["seed"]))
    elif kind == "overflow":
        model, tree, fp, cap = ct.overflow_input()
        paths, n_ovf, _ = ct.overflow_oracle(tree, model, fp, cap, spec["seed"])
        d = device(model, tree, fp, cap, nn, L)
        for w in range(ct.OVERFLOW_SWEEPS):
            try:
                d.sweep(1, spec["seed"], sweep_base=w)
            except Exception:
                pass                                   # (a sweep with overflows reports them; the counter is the check)
        got = d.counters()["overflow"]
        print(label, "overflow", got, "oracle", n_ovf, flush=True)
        assert got == n_ovf and got > 0, (label, got, n_ovf)
        assert orc.paths_equal(d.paths(), paths), (label, "paths")
        d.close()
    else:
        raise KeyError(kind)
print("ok")
'''


def plain(tree, nn, L, n):
    return dict(kind="plain", tree=tree, small_nn=nn, width=L, n=n)


ROWS = {}
for _L in (64, 16):
    ROWS["pruning-%d" % _L] = [plain(t, nn, _L, SHAPE_N) for t, nn in SHAPES]
for _L in (64, 16):
    ROWS["accept-%d" % _L] = [dict(kind="overflow", tree="tree", small_nn=5, width=_L),
                              dict(kind="dense", tree="tree", small_nn=5, width=_L),
                              plain("tree", 5, _L, 4), plain("tree", 5, _L, 5),
                              plain(GENERIC[0], GENERIC[1], _L, GENERIC[2])]


@pytest.mark.gpu
@pytest.mark.parametrize("row", sorted(ROWS))
def test_chain_trips_match_rung_b(row):
    spec = dict(seed=hb.SEED, cases=ROWS[row])
    src = _CHILD % dict(root=_ROOT, tests=_TESTS, spec=json.dumps(spec))
    clean = dict((k, v) for k, v in os.environ.items() if k not in ("EPV_FUSED_PHASE", "EPV_FUSED_LANES", "EPV_FORCE_LDS_POOL"))
    env = dict(clean, EPV_FUSED_PHASE="1", EPV_FORCE_LDS_POOL="1")
    r = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


# ---- without a GPU
def _moves(tree, model, fp, cap):
    J, D, nacc, paths, per_sweep = hb.oracle_run(tree, model, fp, cap, hb.SEED)
    T = np.asarray(tree.branches)[1:]
    for Jk, Dk in per_sweep:
        assert np.all(Jk >= 0) and np.allclose(Dk.reshape(-1, 8).sum(axis=1), (fp.n_sites - 2) * T, rtol=1e-9, atol=0)
    return nacc, not orc.paths_equal(paths, fp)


def test_shapes_and_the_mirror_tree():
    """the five topologies differ in the child walk; the mirror's internal node is node 2 and owns the last two nodes"""
    m = tree_of("mirror")
    assert list(m.subtree_sizes) == [5, 1, 3, 1, 1] and list(m.parent_ids)[1:] == [0, 0, 2, 2]
    t = tree_of("tree")
    assert list(t.subtree_sizes) == [5, 3, 1, 1, 1] and list(t.parent_ids)[1:] == [0, 1, 1, 0]
    assert np.allclose(sorted(m.branches), sorted(t.branches))
    walks = set()
    for name, nn in SHAPES:
        tr = tree_of(name)
        assert tr.n_nodes == nn
        walks.add((tuple(tr.subtree_sizes), tuple(tr.parent_ids)[1:]))
    assert len(walks) == len(SHAPES)
    assert 200 <= SHAPE_N <= 400 and len(hb.colour_sites(SHAPE_N, 0)) > 64
    assert tree_of(GENERIC[0]).n_nodes > 5
    assert all(len(json.dumps(c)) for cases in ROWS.values() for c in cases)


@pytest.mark.parametrize("name", [t for t, _ in SHAPES] + [GENERIC[0]])
def test_oracle_side_of_the_shapes(name):
    model, tree, fp, cap = make_input(name, GENERIC[2] if name == GENERIC[0] else SHAPE_N)
    nacc, moved = _moves(tree, model, fp, cap)
    assert nacc >= 1 and moved, (name, nacc, moved)


def test_oracle_side_of_the_overflow_case():
    model, tree, fp, cap = overflow_input()
    paths, n_ovf, phases = overflow_oracle(tree, model, fp, cap, hb.SEED)
    assert n_ovf > 0 and len(phases) == 3 * OVERFLOW_SWEEPS
    # the site-by-site walk is the sweep
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=hb.SEED)
    o.reset()
    for w in range(OVERFLOW_SWEEPS):
        o.sweep(w)
    assert orc.paths_equal(o.paths(), paths) and o.counters()["overflow"] == n_ovf
    o.close()
    # some wave holds an overflowed site next to one that did not overflow, at either width
    for L in (64, 16):
        assert mixed_waves(phases, L) >= 1, L
    flagged = sum(x for rows in phases for _, x in rows)
    assert 0 < flagged < sum(len(rows) for rows in phases)


def test_oracle_side_of_the_dense_case():
    model, tree, fp, cap = hb.dense_input()
    nacc, moved = _moves(tree, model, fp, cap)
    assert nacc >= 1 and moved
