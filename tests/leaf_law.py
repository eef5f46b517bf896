"""The exact target of the leaf-vector law tests, shared by test_unobserved_leaves_gpu.py,
test_leaf_evidence_gpu.py and test_leaf_oracle.py (a helper, not a test module).

test_mcmc_posterior's 14-site tree case with two leaf cells that are not data: (D, 3), where leaf D flips,
and (C, 6), where nothing does.  The target mixes the exact posterior of each completion c of the two cells
with weight kept_c * e_c, where kept_c is what a fixed number of forward simulations keeps (the prior weight
of the completion's data) and e_c = prod (r_i or 1 - r_i) the evidence (1 under the plain mask).  Standard
errors come from the reference's counts alone: the Kish effective count (sum k_c e_c)^2 / sum k_c e_c^2
stands where the number of kept draws does for one target; under the plain mask it is their total."""
import ctypes as C
import time

import numpy as np

import orc
from common import ref_test_model
import test_mcmc_posterior as post

MISSING = [("D", 3), ("C", 6)]
TRIALS = 20000000
EVIDENCE = [np.float32(0.8), np.float32(0.02)]        # r of MISSING[0] = (D, 3) and MISSING[1] = (C, 6)

_cache = {}


def _exact_completions(model, tree, leaf):
    """(kept per completion, moments per completion) of the 2^len(MISSING) completions; computed once per
    process and input"""
    key = (model.rates.tobytes(), tree.parent_ids.tobytes(), tree.branches.tobytes(), leaf.tobytes())
    if key in _cache:
        return _cache[key]
    t0 = time.perf_counter()
    L = orc.orc_lib()
    u8p, u32p, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    L.orc_exact_posterior_tree.restype = C.c_uint64
    L.orc_exact_posterior_tree.argtypes = [dp, C.c_uint64, C.c_int, u32p, u32p, dp, u8p, u8p, C.c_uint64, C.c_uint64,
                                           C.c_uint64, dp, dp, dp, dp]
    B = tree.n_nodes - 1
    kept, mom = [], []
    for c in range(1 << len(MISSING)):
        lf = leaf.copy()
        for i, (name, s) in enumerate(MISSING):
            lf[tree.node_names.index(name), s] = c >> i & 1
        Jm, Dm, J2, D2 = (np.zeros(B * 8) for _ in range(4))
        flat = np.ascontiguousarray(lf.reshape(-1))
        k = L.orc_exact_posterior_tree(orc._p(model.rates, C.c_double), lf.shape[1], tree.n_nodes,
                                       orc._p(tree.parent_ids, C.c_uint32), orc._p(tree.subtree_sizes, C.c_uint32),
                                       orc._p(tree.branches, C.c_double), orc._p(post.TROOT, C.c_uint8),
                                       orc._p(flat, C.c_uint8), 7 + c, TRIALS, TRIALS, orc._p(Jm, C.c_double),
                                       orc._p(Dm, C.c_double), orc._p(J2, C.c_double), orc._p(D2, C.c_double))
        kept.append(k)
        mom.append((Jm, Dm, J2, D2))
    _cache[key] = (np.array(kept, np.float64), mom)
    print("exact completions: kept", kept, "in %.1f s" % (time.perf_counter() - t0))
    return _cache[key]


def _mixture(kept, mom, evidence):
    """(Jm, Dm, Jse, Dse), P(state 1) per cell, Kish effective count; evidence None = the plain mask"""
    e = np.ones(len(kept))
    if evidence is not None:
        for c in range(len(kept)):
            for i, r in enumerate(evidence):
                e[c] *= float(r) if c >> i & 1 else 1.0 - float(r)
    w = kept * e
    tot = w.sum()
    kish = tot ** 2 / (kept * e ** 2).sum()
    Jm, Dm, J2, D2 = (sum(w[c] * mom[c][i] for c in range(len(w))) / tot for i in range(4))
    p1 = [sum(w[c] for c in range(len(w)) if c >> i & 1) / tot for i in range(len(MISSING))]
    return (Jm, Dm, np.sqrt(np.maximum(J2 - Jm ** 2, 1e-12) / kish), np.sqrt(np.maximum(D2 - Dm ** 2, 1e-12) / kish)), p1, kish


def _sigma(p, kish):
    return np.sqrt(max(p * (1 - p), 1e-4) * (1.0 / kish + 1.0 / 1200.0))


def exact_case():
    """model, tree, leaf data, start paths, the target under EVIDENCE and under the plain mask"""
    model = ref_test_model()
    tree, leaf, fp = post._tree_case()
    kept, mom = _exact_completions(model, tree, leaf)
    return model, tree, leaf, fp, _mixture(kept, mom, EVIDENCE), _mixture(kept, mom, None)
