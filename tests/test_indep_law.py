"""The yardstick of the soft-leaf tests (indep_law.py) checked against itself, and the option and file errors of
epievo_initialization -m / -l, which return before any device call.  No GPU."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import indep_law as law
from common import TREE_NWK_TEXT, config
from epievo_amd import _build

RATES = np.array([0.7, 1.9])
BIN = os.path.join(_build.BIN_DIR, "epievo_initialization")


def _case(cfg, n=40, seed=3):
    """random leaf data with evidence r in [0.02, 0.98], hard (0 / 1) cells, 0.5 cells and masked cells"""
    tree = config(cfg)
    N = tree.n_nodes
    rng = np.random.default_rng(seed)
    state = rng.integers(0, 2, (N, n)).astype(np.uint8)
    r = np.full((N - 1, n), np.nan, np.float32)
    mask = np.zeros((N - 1, n), np.uint8)
    for v in range(1, N):
        if tree.subtree_sizes[v] != 1:
            continue
        kind = rng.integers(0, 5, n)
        r[v - 1] = np.where(kind == 0, rng.uniform(0.02, 0.98, n), np.nan).astype(np.float32)
        r[v - 1][kind == 1] = state[v][kind == 1]            # hard evidence
        r[v - 1][kind == 2] = 0.5
        mask[v - 1] = kind == 3                              # kind 4: data
    return tree, state, r, mask


@pytest.mark.parametrize("cfg", ["tree", "star4", "multi", "cat6"])
def test_two_routes_agree_on_every_node_marginal(cfg):
    """two independent derivations, each a few dozen positive-term fp64 operations on numbers in [0, 1]"""
    tree, state, r, mask = _case(cfg)
    q = law.leaf_q(tree, state, r, mask)
    p1, l1 = law.marginals_enum(tree, RATES, q)
    p2, l2 = law.marginals_pruning(tree, RATES, q)
    assert np.abs(p1 - p2).max() <= 1e-13
    np.testing.assert_allclose(l1, l2, rtol=1e-13)
    # the leaf vector's two identities: 0.5 is the mask, evidence 0 / 1 is data
    r_half = np.where(mask != 0, np.float32(0.5), r)
    assert np.abs(law.marginals_pruning(tree, RATES, law.leaf_q(tree, state, r_half))[0] - p2).max() <= 1e-15
    hard = np.where(np.isnan(r) & (mask == 0), state[1:].astype(np.float32), r)
    assert np.array_equal(law.leaf_q(tree, state, hard, mask), q)


@pytest.mark.parametrize("cfg", ["tree", "multi"])
def test_completion_mixture_is_the_leaf_marginal(cfg):
    """sum over the hard completions c of the leaves with weight L(c) prod (r_i or 1 - r_i): the weight the GPU
    test of the expectation uses"""
    tree, state, r, mask = _case(cfg, n=12)
    q = law.leaf_q(tree, state, r, mask)
    p, _ = law.marginals_pruning(tree, RATES, q)
    leaves = [v for v in range(1, tree.n_nodes) if tree.subtree_sizes[v] == 1]
    n = state.shape[1]
    w = []
    comps = list(itertools.product((0, 1), repeat=len(leaves)))
    for c in comps:
        st = np.zeros_like(state)
        for v, x in zip(leaves, c):
            st[v] = x
        like = law.marginals_enum(tree, RATES, law.leaf_q(tree, st))[1]
        w.append(like * np.prod([q[v, :, x] for v, x in zip(leaves, c)], axis=0))
    w = np.array(w)                                             # (completions, n)
    for i, v in enumerate(leaves):
        mix = w[[k for k, c in enumerate(comps) if c[i] == 1]].sum(0) / w.sum(0)
        assert np.abs(mix - p[v]).max() <= 1e-13, (v, n)


# ---- epievo_initialization -m / -l: what fails on the host, before a device is opened

def _files(d, rows, header="#C\tD\tF"):
    open(d + "/t.nwk", "w").write(TREE_NWK_TEXT)
    with open(d + "/f", "w") as f:
        f.write(header + "\n")
        for i, row in enumerate(rows):
            f.write("%d\t%s\n" % (i, "\t".join(row)))
    return [BIN, "-i", "1", "-B", "1", "-s", "5", "-o", d + "/o.paths", "-p", d + "/o.param"]


GOOD = [("0", "1", "N"), ("1", "1", "0"), ("N", "0", "0"), ("0", "0", "1")]


def _fails(cmd, needle):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert needle in r.stderr, r.stderr
    assert "HIP" not in r.stderr and "device" not in r.stderr, r.stderr     # (it never got that far)


def test_initialization_option_errors(tmp_path):
    d = str(tmp_path)
    base = _files(d, GOOD)
    for flag in ("-m", "-l"):
        _fails(base + [flag, d + "/f", d + "/t.nwk", d + "/f"], "takes the place of <states-file>")
        _fails(base + [flag, d + "/f"], "takes the place of <states-file>")                 # no tree, no -T
        _fails(base + [flag, d + "/f", "-T", "1.0", d + "/f"], "takes the place of <states-file>")
    _fails(base + ["-m", d + "/f", "-l", d + "/f", d + "/t.nwk"], "cannot be given together")


@pytest.mark.parametrize("flag", ["-m", "-l"])
def test_initialization_file_errors(tmp_path, flag):
    d = str(tmp_path)
    base = _files(d, [r[:2] for r in GOOD], header="#C\tD")          # a leaf column missing
    _fails(base + [flag, d + "/f", d + "/t.nwk"], "no data in leaf node: F")
    base = _files(d, GOOD[:2] + [("1", "0")] + GOOD[3:])              # a row with too few cells
    _fails(base + [flag, d + "/f", d + "/t.nwk"], "bad line in")
    base = _files(d, [])                                              # no rows at all
    _fails(base + [flag, d + "/f", d + "/t.nwk"], "no sites read")
    _fails(base + [flag, d + "/nope", d + "/t.nwk"], "cannot read")


def test_initialization_leaf_probs_token_outside_unit_interval(tmp_path):
    d = str(tmp_path)
    for bad in ("1.5", "-0.25", "x", "nan", "inf"):
        base = _files(d, GOOD[:1] + [("0.3", bad, "1")] + GOOD[1:])
        _fails(base + ["-l", d + "/f", d + "/t.nwk"], "D at site 1 is neither a probability in [0, 1] nor N")
