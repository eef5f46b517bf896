"""The rows of EPV_OPT_LEAF_FAST, shared by test_leaf_fast.py (no GPU: the plan, and the
oracle leg that makes a row say something) and test_leaf_fast_gpu.py (the leaf variants of the fused bodies, of the
second and of the third proposal kernel against the oracle's rung B, bit for bit).

A row: a tree and a genome length, the leaf content of test_leaf_matrix.leaf_content ("mask", "ev" = evidence and
mask, "all" = evidence on every leaf cell), the options, the EPV_* knobs of its child process and the plan fields it
expects with option 32 and the content held.  The oracle takes the mask and the table itself and does not depend on
the kernel path, so a row's oracle leg depends on (tree, n, content, options, mode, seed) alone: oracle_leg_of caches
it under that key."""
import numpy as np

from test_leaf_matrix import leaf_content, make_tree, oracle_leg     # noqa: F401  (re-exported to the child)
from common import ref_test_model
from epievo_amd import host

LEAF_FAST = 32                                                           # EPV_OPT_LEAF_FAST
OPTION_BITS = dict(reference_proposal_ratio=1, forward_rejection=2, sample_root=4)
FR = {"forward_rejection": True}
_SEP = {"EPV_FUSED_PHASE": "0"}
_V3 = dict(_SEP, EPV_PROPOSE_V3="1")


def fused(nn, lanes=16):
    return dict(propose="fused", small_nn=nn, jumps="fused", accept="fused", gpool=False, listed=False, fused_lanes=lanes)


def v2(jumps):
    return dict(propose="V2", gpool=False, jumps=jumps, accept="accept_cache", listed=True, small_nn=0, p3_words=0)


def v3(words, slab, jumps="jumps_all"):
    return dict(propose="V3", p3_words=words, p3_slab_pool=slab, jumps=jumps, accept="accept3", listed=True, gpool=False)


def _row(id, tree, n, content, expect, env=None, opts=None, mode="mcmc", seed=19):
    return dict(id=id, tree=tree, n=n, content=content, opts=opts or {}, env=env or {}, expect=expect, mode=mode, seed=seed)


def _lanes(k):
    return {"EPV_FUSED_PHASE": "1", "EPV_FUSED_LANES": str(k)}


ROWS = [
    # the fused small-tree bodies, NN = 2 .. 5
    _row("pair", "pair", 1501, "ev", fused(2)),
    _row("cherry", "cherry", 1501, "ev", fused(3)),
    _row("star3", "star3", 1501, "ev", fused(4)),
    _row("tree", "tree", 1999, "ev", fused(5)),
    _row("tree-mask", "tree", 1999, "mask", fused(5)),
    _row("tree-lanes32", "tree", 1999, "ev", fused(5, 32), env=_lanes(32)),
    _row("tree-lanes64", "tree", 1999, "ev", fused(5, 64), env=_lanes(64)),
    # the fused generic body
    _row("star5", "star5", 1501, "ev", fused(0)),
    _row("star5-mask", "star5", 1501, "mask", fused(0)),
    _row("cat6", "cat6", 1501, "ev", fused(0), env={"EPV_FUSED_PHASE": "1", "EPV_FORCE_LDS_POOL": "1"}),
    _row("star5-lanes64", "star5", 1501, "ev", fused(0, 64), env=_lanes(64)),
    _row("tree-generic", "tree", 1999, "ev", fused(0), env={"EPV_P2_SMALL_TREE": "0"}),
    # the second kernel, separate
    _row("v2", "tree", 1999, "ev", v2("jumps_all"), env=dict(_SEP, EPV_SEG_JUMPS="0")),
    _row("v2-mask", "tree", 1999, "mask", v2("jumps_all"), env=dict(_SEP, EPV_SEG_JUMPS="0")),
    _row("v2-seg", "tree", 1999, "ev", v2("segments"), env=dict(_SEP, EPV_SEG_JUMPS="1")),
    # the third: node masks of one word and of two, slabs from the pool, a heavy list of one lane's worst case
    _row("v3", "bal16", 599, "ev", v3(1, False), env=_V3),
    _row("v3-mask", "bal16", 599, "mask", v3(1, False), env=_V3),
    _row("v3-two-words", "bal64", 400, "ev", v3(2, False), env=_V3),
    _row("v3-slab", "bal16", 599, "ev", v3(1, True), env=dict(_V3, EPV_P3_SLAB_POOL="2")),
    _row("v3-min-list", "bal16", 599, "ev", v3(1, False), env=dict(_V3, EPV_P3_MIN_LIST="1")),
    # forward rejection on one row of each family
    _row("fr-tree", "tree", 1999, "ev", fused(5), opts=FR),
    _row("fr-star5", "star5", 1501, "ev", fused(0), opts=FR),
    _row("fr-v2", "tree", 1999, "ev", v2("jumps"), env=dict(_SEP, EPV_SEG_JUMPS="0"), opts=FR),
    _row("fr-v3", "bal16", 599, "ev", v3(1, False, "jumps"), env=_V3, opts=FR),
    # the genome-end special cases: evidence on every leaf cell
    _row("tiny-tree3", "tree", 3, "all", fused(5)),
    _row("tiny-tree4", "tree", 4, "all", fused(5)),
    _row("tiny-tree5", "tree", 5, "all", fused(5)),
    _row("tiny-pair6", "pair", 6, "all", fused(2)),
    # a capacity that overflows: two single sweeps
    _row("tree-overflow", "tree", 1999, "ev", fused(5), mode="overflow", seed=31),
    _row("v3-overflow", "bal16", 599, "ev", v3(1, False), env=_V3, mode="overflow", seed=31),
]
ROW = {r["id"]: r for r in ROWS}


def option_word(row, leaf_fast=True):
    return sum(bit for name, bit in OPTION_BITS.items() if row["opts"].get(name)) | (LEAF_FAST if leaf_fast else 0)


def make_case(row):
    """as test_leaf_matrix.make_case -> (model, tree, paths, mask, table, capacity)"""
    model, tree = ref_test_model(), make_tree(row["tree"])
    fp = host.simulate(model, tree, row["n"], 6)
    mask, r = leaf_content(tree, fp, row["content"], 7)
    cap = int(fp.counts().max()) if row["mode"] == "overflow" else int(max(16, 2 * fp.counts().max() + 8))
    return model, tree, fp, mask, r, cap


def host_plan(row, case, options, held=True):
    """host.phase_plan of what a context of this row holds"""
    model, tree, fp, mask, r, cap = case
    kbar = fp.counts().sum() / (fp.n_sites * (tree.n_nodes - 1))
    um = int(np.count_nonzero(mask)) if held and mask is not None else 0
    ev = int(np.count_nonzero(~np.isnan(r))) if held and r is not None else 0
    return host.phase_plan(tree, fp.n_sites, cap, kbar, options, um, ev, knobs=row["env"])


_LEGS = {}


def oracle_leg_of(row, case=None):
    key = (row["tree"], row["n"], row["content"], tuple(sorted(row["opts"].items())), row["mode"], row["seed"])
    if key not in _LEGS:
        _LEGS[key] = oracle_leg(row, case or make_case(row))
    return _LEGS[key]
