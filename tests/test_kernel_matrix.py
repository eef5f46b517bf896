"""Every kernel variant of a colour phase under every option, each asserted to be the variant that ran.

Each row names a tree, a genome length, the EPV_* knobs that steer the plan, the options (EPV_OPT_*) and
the plan fields it expects (DeviceSampler.phase_plan, epv_phase_plan of include/epievo_mi355x.h).  The
row runs in a fresh process with its knobs in the environment (a context reads them when it is
created): the plan is asserted after reset(), then run_mcmc is compared with the oracle's parallel
rung B in the same mode -- J, D, the accept count, the paths and the cached triple likelihoods bit
for bit.  Rows with the default options also run two sweeps at a capacity that overflows.
Without a GPU, test_plan_without_a_gpu asserts every row's expected fields on host.phase_plan -- the device
library's planner (csrc/epv_plan.h) through libepv_host.so; the GPU child asserts that the context's own plan
equals it word for word.

Coverage (variant x options -> rows):
  fused small-tree body NN = 2 / 3 / 4 / 5    forward rejection: fr-pair, fr-cherry, fr-star3, fr-tree;
                                             default: cherry, star3 (and test_fused_small_tree.py)
  fused generic body                         forward rejection: fr-star5, fr-cat6; default: star5 (6 nodes)
  V2, LDS pool, jumps_all / jumps           forward rejection: fr-v2-lds
  V2, LDS pool, segment jumps                forward rejection: fr-v2-lds-seg
  V3, one-word masks / two-word / slab pool  forward rejection: fr-bal16-v3, fr-bal64-v3, fr-bal16-v3-slab;
                                             default: n64, n65, n128, cat64, unary-q63
  V1, LDS pool                               forward rejection: fr-v1-lds; reference ratio, forward
                                             rejection + reference ratio, SAMPLE_ROOT: ref-tree, frref-tree,
                                             sr-tree
  V1, global pool (accept3 over all sites)   forward rejection: fr-v1-global; ref-tree-global, ref-bal16,
                                             frref-bal16, sr-bal16; default: n129, multi-no-v3, unary-q64
  V1's LEAF template axis (mask, evidence)   test_leaf_matrix.py: all eight (pool, ratio, leaf mode)
                                             instantiations against rung B with its own leaf vector
  fused, 32 and 64 sites per wave            forward rejection: fr-pair-lanes64, fr-tree-lanes64, fr-star5-lanes64; every
  (every other fused row here runs 16,       other option, the launch tails, update ranges, the halo mode and the
  the width a context chooses below          width a context chooses by itself: test_fused_lanes.py; dense histories
  98302 sites)                               at 32 and 64: the -lanes rows of test_dense_histories_gpu.py
  dense histories (tens of jumps per path,   test_dense_histories_gpu.py: every row here draws its histories from
  where the rows above have two or three)    test.param on branches of 0.02 - 0.8, which the reference model
                                             forces (it accepts nothing on dense input); the rows there use two
                                             other models (dense_cases.py) and cover more than 64 segments on a
                                             branch, two and more words of proposal states, the fused phase at
                                             C = 31 with every branch heavy, the statistics kernels' merge rings
                                             and the accumulate kernels
  models other than test.param, and models   test_model_space_gpu.py: every family above under the models and rows of
  that did not generate the data             model_cases.py (rate T from 1e-12 to 2e5, rate ratios up to 5e9)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))


# ---- trees as pre-order arrays (host.Tree(subtree_sizes, parent_ids, branches))
def _join(subtrees, blen):
    """a root whose children are the given subtrees (host.Tree each), every new branch of length blen"""
    sizes, parents, br = [1], [0], [0.0]
    for t in subtrees:
        off = len(sizes)
        sizes += [int(s) for s in t.subtree_sizes]
        parents += [0] + [int(p) + off for p in t.parent_ids[1:]]
        br += [blen] + [float(b) for b in t.branches[1:]]
    sizes[0] = len(sizes)
    return sizes, parents, br


def _caterpillar(leaves, blen):
    """((((L0, L1), L2), L3) ...): leaves - 1 internal nodes, one per level"""
    if leaves == 1:
        return [1], [0], [0.0]
    s, p, b = _caterpillar(leaves - 1, blen)
    # root of the new tree: the old tree (shifted by one) and a leaf
    sizes = [len(s) + 2] + s
    parents = [0] + [0] + [x + 1 for x in p[1:]] + [0]
    br = [0.0, blen * 1.3] + b[1:] + [blen]
    return sizes + [1], parents, br


def _unary_chain(k, leaves, blen):
    """root -> k unary nodes -> a balanced subtree of `leaves` leaves, and a leaf at the root: k + leaves - 1
    internal nodes below the root (the large-tree kernel's q rows)"""
    from epievo_amd import host
    sub = host.Tree.balanced(leaves, blen)
    n = 1 + k + len(sub.subtree_sizes) + 1
    sizes, parents, br = [n], [0], [0.0]
    for i in range(k):
        sizes.append(n - 2 - i)
        parents.append(i)
        br.append(blen * (1.0 + 0.1 * (i % 3)))
    off = len(sizes)
    sizes += [int(s) for s in sub.subtree_sizes]
    parents += [k] + [int(p) + off for p in sub.parent_ids[1:]]
    br += [blen] + [float(b) for b in sub.branches[1:]]
    sizes.append(1)
    parents.append(0)
    br.append(0.3)
    return sizes, parents, br


def make_tree(name):
    from epievo_amd import host
    from common import config
    if name == "n64":            # trifurcating root, binary below: 64 nodes, one-word node masks
        arrays = _join([host.Tree.balanced(11, 0.03)] * 3, 0.02)
    elif name == "n65":          # binary, 33 leaves: 65 nodes, two-word node masks
        return host.Tree.balanced(33, 0.03)
    elif name == "n128":         # trifurcating root: 128 nodes, the largest tree the large-tree kernel takes
        arrays = _join([host.Tree.balanced(22, 0.02), host.Tree.balanced(22, 0.02), host.Tree.balanced(21, 0.02)], 0.02)
    elif name == "n129":         # binary, 65 leaves: 129 nodes, one too many
        return host.Tree.balanced(65, 0.02)
    elif name == "cat64":        # a caterpillar of 64 leaves: 127 nodes, 63 levels
        arrays = _caterpillar(64, 0.02)
    elif name == "unary-q63":    # 63 q rows: the most the node word's six-bit field holds
        arrays = _unary_chain(48, 16, 0.03)
    elif name == "unary-q64":
        arrays = _unary_chain(49, 16, 0.03)
    else:
        return config(name)
    t = host.Tree(*arrays)
    assert t.subtree_sizes[0] == t.n_nodes
    return t


_CODE = r'''
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import orc
from common import ref_test_model
from epievo_amd import host
from epievo_amd.sampler import DeviceSampler
from test_kernel_matrix import make_tree
spec = json.loads(%(spec)r)
opts, expect = spec["opts"], spec["expect"]
model, tree = ref_test_model(), make_tree(spec["tree"])
assert tree.n_nodes == spec["nodes"], tree.n_nodes
fp = host.simulate(model, tree, spec["n"], 6)
cap = int(max(16, 2 * fp.counts().max() + 8))
d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap); d.set_options(**opts); d.reset()
plan = d.phase_plan()
bad = dict((k, (v, plan[k])) for k, v in expect.items() if plan[k] != v)
assert not bad, "plan differs (expected, got): %%r; plan %%r" %% (bad, plan)
# the planner without a GPU, given what this context holds, decides the same word for word
kbar = fp.counts().sum() / (spec["n"] * (tree.n_nodes - 1))
assert host.phase_plan(tree, spec["n"], d.capacity(), kbar, d.options(), knobs=spec["env"]) == plan

def oracle(c, seed):
    o = orc.Oracle(tree, model, fp, "B", cap=c, seed=seed)
    o.set_sampler(bool(opts.get("forward_rejection")))
    o.set_proposal_mode(bool(opts.get("reference_proposal_ratio")))
    o.set_sample_root(bool(opts.get("sample_root")))
    o.reset()
    return o

o = oracle(cap, 19)
Jd, Dd, nd = d.run_mcmc(2, 3, 19, sweep_base=4)
Jo, Do, no, _ = o.run_mcmc(2, 3, sweep_base=4)
assert nd == no, (nd, no)
assert np.array_equal(Jd, Jo) and np.array_equal(Dd, Do)
assert orc.paths_equal(d.paths(), o.paths())
# (SAMPLE_ROOT: the two end sites' cached likelihoods are never read and not kept current, test_sample_root.py)
lo, hi = (1, -1) if opts.get("sample_root") else (0, None)
assert np.array_equal(d.tri_llh()[lo:hi].view(np.uint64), o.tri_llh()[lo:hi].view(np.uint64))
assert d.counters()["overflow"] == o.counters()["overflow"]
assert d.phase_plan() == plan
if not opts:
    # a capacity that overflows: the overflow decisions must be the sequential sampler's too
    cap2 = int(fp.counts().max())
    d2 = DeviceSampler(0); d2.set_tree(tree); d2.set_model(model); d2.upload_paths(fp, cap2); d2.reset()
    plan2 = d2.phase_plan()
    assert plan2["propose"] == plan["propose"], (plan2, plan)
    o2 = oracle(cap2, 23)
    for w in range(2):
        try:
            d2.sweep(1, 23, sweep_base=w)
        except Exception as e:
            assert "rejected" in str(e) or "capacity" in str(e).lower(), e
        o2.sweep(w)
        assert orc.paths_equal(d2.paths(), o2.paths()), "paths differ after overflow sweep %%d" %% w
    assert d2.counters()["overflow"] == o2.counters()["overflow"] > 0
    d2.close()
d.close()
print("ok", json.dumps(plan))
'''

_SEP = {"EPV_FUSED_PHASE": "0"}              # the separate kernels (small launches take the fused phase)
_L64 = {"EPV_FUSED_PHASE": "1", "EPV_FUSED_LANES": "64"}     # the sites per wave of a genome above 196605 sites
FR, REF, SR = {"forward_rejection": True}, {"reference_proposal_ratio": True}, {"sample_root": True}
FRREF = {"forward_rejection": True, "reference_proposal_ratio": True}


def fused(nn, lanes=16):
    return dict(propose="fused", small_nn=nn, jumps="fused", accept="fused", gpool=False, listed=False,
                fused_lanes=lanes)


def v2(gpool, jumps, accept="accept_cache"):
    return dict(propose="V2", gpool=gpool, jumps=jumps, accept=accept, listed=True, small_nn=0, p3_words=0)


def v3(words, slab, jumps):
    return dict(propose="V3", p3_words=words, p3_slab_pool=slab, jumps=jumps, accept="accept3", listed=True,
                gpool=False)


def v1(gpool, refq, jumps, accept):
    return dict(propose="V1", gpool=gpool, refq=refq, jumps=jumps, accept=accept, listed=False, p3_words=0)


# (id, tree, nodes, n, env, options, expected plan fields)
ROWS = [
    # forward rejection on every proposal variant
    ("fr-pair", "pair", 2, 1500, {}, FR, fused(2)),
    ("fr-cherry", "cherry", 3, 1500, {}, FR, fused(3)),
    ("fr-star3", "star3", 4, 1500, {}, FR, fused(4)),
    ("fr-tree", "tree", 5, 1500, {}, FR, fused(5)),
    ("fr-star5", "star5", 6, 1500, {}, FR, fused(0)),
    ("fr-pair-lanes64", "pair", 2, 1500, _L64, FR, fused(2, 64)),
    ("fr-tree-lanes64", "tree", 5, 1500, _L64, FR, fused(5, 64)),
    ("fr-star5-lanes64", "star5", 6, 1500, _L64, FR, fused(0, 64)),
    ("fr-cat6", "cat6", 11, 1500, {"EPV_FUSED_PHASE": "1", "EPV_FORCE_LDS_POOL": "1"}, FR, fused(0)),
    ("fr-v2-lds", "tree", 5, 2000, dict(_SEP, EPV_SEG_JUMPS="0"), FR, v2(False, "jumps")),
    ("fr-v2-lds-seg", "tree", 5, 2000, dict(_SEP, EPV_SEG_JUMPS="1"), FR, v2(False, "segments")),
    ("fr-bal16-v3", "bal16", 31, 600, dict(_SEP, EPV_PROPOSE_V3="1"), FR, v3(1, False, "jumps")),
    ("fr-bal64-v3", "bal64", 127, 400, dict(_SEP, EPV_PROPOSE_V3="1"), FR, v3(2, False, "jumps")),
    ("fr-bal16-v3-slab", "bal16", 31, 600, dict(_SEP, EPV_PROPOSE_V3="1", EPV_P3_SLAB_POOL="2"), FR,
     v3(1, True, "jumps")),
    ("fr-v1-lds", "tree", 5, 1500, dict(_SEP, EPV_PROPOSE_V1="1"), FR, v1(False, False, "jumps", "accept_cache")),
    ("fr-v1-global", "tree", 5, 1500, dict(_SEP, EPV_PROPOSE_V1="1", EPV_FORCE_GLOBAL_POOL="1"), FR,
     v1(True, False, "jumps", "accept_cache")),
    # the reference ratio, forward rejection with it, and SAMPLE_ROOT: the first proposal kernel
    ("ref-tree", "tree", 5, 1500, {}, REF, v1(False, True, "jumps_all", "accept_cache")),
    ("frref-tree", "tree", 5, 1500, {}, FRREF, v1(False, True, "jumps", "accept_cache")),
    ("sr-tree", "tree", 5, 1500, {}, SR, v1(False, True, "jumps_all", "accept_cache")),
    ("ref-tree-global", "tree", 5, 1500, {"EPV_FORCE_GLOBAL_POOL": "1"}, REF, v1(True, True, "jumps_all", "accept_cache")),
    ("ref-bal16", "bal16", 31, 600, {}, REF, v1(True, True, "jumps_all", "accept3")),
    ("frref-bal16", "bal16", 31, 600, {}, FRREF, v1(True, True, "jumps", "accept3")),
    ("sr-bal16", "bal16", 31, 600, {}, SR, v1(True, True, "jumps_all", "accept3")),
    # the small-tree bodies' limit: 3 and 4 nodes take theirs, 6 nodes the generic body
    ("cherry", "cherry", 3, 3000, {}, {}, fused(3)),
    ("star3", "star3", 4, 3000, {}, {}, fused(4)),
    ("star5", "star5", 6, 3000, {}, {}, fused(0)),
    # the large-tree kernel's limits (plan_p3): node masks of one and two words, 128 nodes, q rows
    ("n64", "n64", 64, 1500, dict(_SEP, EPV_PROPOSE_V3="1"), {}, v3(1, False, "jumps_all")),
    ("n65", "n65", 65, 600, dict(_SEP, EPV_PROPOSE_V3="1"), {}, v3(2, False, "jumps_all")),
    ("n128", "n128", 128, 400, dict(_SEP, EPV_PROPOSE_V3="1"), {}, v3(2, False, "jumps_all")),
    ("n129", "n129", 129, 400, dict(_SEP, EPV_PROPOSE_V3="1"), {}, v1(True, False, "jumps_all", "accept3")),
    ("multi-no-v3", "multi", 9, 1500, dict(_SEP, EPV_PROPOSE_V3="1", EPV_SEG_JUMPS="0"), {},
     v1(True, False, "jumps_all", "accept_cache")),       # a node below the root with three children
    ("cat64", "cat64", 127, 400, dict(_SEP, EPV_PROPOSE_V3="1"), {}, v3(2, False, "jumps_all")),
    ("unary-q63", "unary-q63", 81, 600, dict(_SEP, EPV_PROPOSE_V3="1"), {}, v3(2, False, "jumps_all")),
    ("unary-q64", "unary-q64", 82, 600, dict(_SEP, EPV_PROPOSE_V3="1"), {}, v1(True, False, "jumps_all", "accept3")),
]


@pytest.mark.gpu
@pytest.mark.parametrize("tree,nodes,n,env,opts,expect", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_kernel_variant_matches_rung_b(tree, nodes, n, env, opts, expect):
    spec = json.dumps(dict(tree=tree, nodes=nodes, n=n, env=env, opts=opts, expect=expect))
    code = _CODE % dict(root=_ROOT, tests=_TESTS, spec=spec)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=900)
    print(r.stdout[-2000:])         # the plan that ran, fused_lanes included
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]


OPTION_BITS = dict(reference_proposal_ratio=1, forward_rejection=2, sample_root=4)     # EPV_OPT_*


@pytest.mark.parametrize("tree,nodes,n,env,opts,expect", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_plan_without_a_gpu(tree, nodes, n, env, opts, expect):
    """no GPU: the planner of the device library (csrc/epv_plan.h, through libepv_host.so) routes every row's tree,
    capacity, mean jump count, knobs and options to the kernels the row expects -- the inputs built as the GPU
    child builds them"""
    from common import ref_test_model
    from epievo_amd import host
    model, t = ref_test_model(), make_tree(tree)
    assert t.n_nodes == nodes
    fp = host.simulate(model, t, n, 6)
    cap = int(max(16, 2 * fp.counts().max() + 8))
    kbar = fp.counts().sum() / (n * (t.n_nodes - 1))
    options = sum(bit for name, bit in OPTION_BITS.items() if opts.get(name))
    plan = host.phase_plan(t, n, cap, kbar, options, knobs=env)
    bad = dict((k, (v, plan[k])) for k, v in expect.items() if plan[k] != v)
    assert not bad, "plan differs (expected, got): %r; plan %r" % (bad, plan)


def test_plan_without_a_gpu_checks_what_it_is_given():
    """no GPU: arrays that are no pre-order tree and sizes no context can hold are refused, and a tree too large for the
    LDS node table gets the device library's error text"""
    from epievo_amd import host
    with pytest.raises(RuntimeError, match="pre-order"):
        host.phase_plan(host.Tree([3, 1, 1], [0, 2, 0], [0.0, 0.1, 0.1]), 400, 16, 0.05)      # a parent behind its child
    with pytest.raises(RuntimeError, match="pre-order"):
        host.phase_plan(host.Tree([3, 3, 1], [0, 0, 1], [0.0, 0.1, 0.1]), 400, 16, 0.05)      # a subtree past the end
    for n, cap in [(2, 16), (400, 0), (400, 2048)]:
        with pytest.raises(RuntimeError, match="bad paths"):
            host.phase_plan(make_tree("tree"), n, cap, 0.05)
    with pytest.raises(RuntimeError, match="tree too large for the 160 KiB LDS node table"):
        host.phase_plan(host.Tree.balanced(400, 0.02), 400, 16, 0.05)


def test_rows_cover_the_matrix():
    """no GPU: the table names every variant under forward rejection -- the fused bodies by their sites per wave --
    and the trees it claims"""
    seen = set((r[6]["propose"], r[6].get("small_nn"), r[6].get("gpool"), r[6].get("jumps"), r[6].get("p3_words"),
                r[6].get("p3_slab_pool"), r[6].get("fused_lanes")) for r in ROWS if r[5] == FR)
    for key in [("fused", 2, False, "fused", None, None, 16), ("fused", 3, False, "fused", None, None, 16),
                ("fused", 4, False, "fused", None, None, 16), ("fused", 5, False, "fused", None, None, 16),
                ("fused", 0, False, "fused", None, None, 16), ("fused", 2, False, "fused", None, None, 64),
                ("fused", 5, False, "fused", None, None, 64), ("fused", 0, False, "fused", None, None, 64),
                ("V2", 0, False, "jumps", 0, None, None),
                ("V2", 0, False, "segments", 0, None, None),
                ("V3", None, False, "jumps", 1, False, None), ("V3", None, False, "jumps", 2, False, None),
                ("V3", None, False, "jumps", 1, True, None), ("V1", None, False, "jumps", 0, None, None),
                ("V1", None, True, "jumps", 0, None, None)]:
        assert key in seen, key
    assert all(r[6]["fused_lanes"] == int(r[4].get("EPV_FUSED_LANES", 16)) for r in ROWS if r[6]["propose"] == "fused")
    assert len(set(r[0] for r in ROWS)) == len(ROWS)
    for r in ROWS:
        t = make_tree(r[1])
        assert t.n_nodes == r[2], r[0]
        # a valid pre-order tree: every subtree size is one plus its children's, parents precede children
        size = np.ones(t.n_nodes, np.int64)
        for v in range(t.n_nodes - 1, 0, -1):
            assert t.parent_ids[v] < v and t.branches[v] > 0.0
            size[t.parent_ids[v]] += size[v]
        assert np.array_equal(size, t.subtree_sizes), r[0]
    kids = lambda t: np.bincount(t.parent_ids[1:], minlength=t.n_nodes)
    internal = lambda t: int(sum(1 for v in range(1, t.n_nodes) if t.subtree_sizes[v] > 1))
    assert kids(make_tree("n64"))[0] == 3 and kids(make_tree("n128"))[0] == 3
    assert max(kids(make_tree("multi"))[1:]) == 3
    assert internal(make_tree("unary-q63")) == 63 and internal(make_tree("unary-q64")) == 64
    assert sorted(set(kids(make_tree("unary-q64"))[1:]) - {0}) == [1, 2]
