"""Leaf evidence, the parts that run without a GPU: the -l/--leaf-probs file of the E-step programs is
checked against the input paths before any device call."""
import os
import subprocess

import pytest

from epievo_amd import _build
from test_unobserved_leaves import leaf_ends, write_states, leaves, make_inputs

BIN = _build.BIN_DIR


def write_probs(path, tree, cols, ends, tokens=None):
    """a -l file with the columns `cols` (node names): str(end state) per cell, or tokens[(name, site)]"""
    tokens = tokens or {}
    idx = [tree.node_names.index(c) for c in cols]
    with open(path, "w") as f:
        f.write("#" + "\t".join(cols) + "\n")
        for s in range(ends.shape[1]):
            f.write("%d\t%s\n" % (s, "\t".join(tokens.get((c, s), str(int(ends[i, s]))) for c, i in zip(cols, idx))))


def est_histories(d, *extra):
    cmd = [os.path.join(BIN, "epievo_est_histories"), "-B", "2", "-L", "1", "-s", "3", "-o", d + "/out.paths"] + \
        list(extra) + [d + "/p.param", d + "/t.nwk", d + "/in.paths"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def test_a_data_token_that_contradicts_the_paths_is_refused(tmp_path):
    d = str(tmp_path)
    model, tree, fp = make_inputs(d)
    ends = leaf_ends(tree, fp)
    leaf = leaves(tree)[1]
    ends[tree.node_names.index(leaf), 57] ^= 1
    write_probs(d + "/l.probs", tree, leaves(tree), ends, {(leaves(tree)[0], 10): "0.25"})
    r = est_histories(d, "-l", d + "/l.probs")
    assert r.returncode != 0
    assert ("leaf %s at site 57" % leaf) in r.stderr and "input paths end in" in r.stderr, r.stderr
    assert not os.path.exists(d + "/out.paths")


def test_a_file_without_a_leaf_column_is_refused(tmp_path):
    d = str(tmp_path)
    model, tree, fp = make_inputs(d)
    write_probs(d + "/l.probs", tree, leaves(tree)[:-1], leaf_ends(tree, fp))
    r = est_histories(d, "-l", d + "/l.probs")
    assert r.returncode != 0
    assert "no column for leaf %s" % leaves(tree)[-1] in r.stderr, r.stderr
    assert not os.path.exists(d + "/out.paths")


def test_a_file_with_too_few_rows_is_refused(tmp_path):
    d = str(tmp_path)
    model, tree, fp = make_inputs(d)
    write_probs(d + "/l.probs", tree, leaves(tree), leaf_ends(tree, fp)[:, :-1])
    r = est_histories(d, "-l", d + "/l.probs")
    assert r.returncode != 0 and "sites" in r.stderr, r.stderr
    assert not os.path.exists(d + "/out.paths")


@pytest.mark.parametrize("token", ["1.5", "-0.25", "x0.3", "0.3x", "inf", "nan"])
def test_a_token_that_is_no_probability_is_refused(tmp_path, token):
    d = str(tmp_path)
    model, tree, fp = make_inputs(d)
    leaf = leaves(tree)[2]
    write_probs(d + "/l.probs", tree, leaves(tree), leaf_ends(tree, fp), {(leaf, 33): token})
    r = est_histories(d, "-l", d + "/l.probs")
    assert r.returncode != 0
    assert ("leaf %s at site 33" % leaf) in r.stderr, r.stderr
    assert not os.path.exists(d + "/out.paths")


def test_leaf_probs_together_with_missing_is_refused(tmp_path):
    d = str(tmp_path)
    model, tree, fp = make_inputs(d)
    ends = leaf_ends(tree, fp)
    write_probs(d + "/l.probs", tree, leaves(tree), ends, {(leaves(tree)[0], 10): "0.25"})
    write_states(d + "/m.states", tree, leaves(tree), ends, missing=[(leaves(tree)[0], 10)])
    r = est_histories(d, "-l", d + "/l.probs", "-m", d + "/m.states")
    assert r.returncode != 0 and "-l" in r.stderr and "-m" in r.stderr, r.stderr
    assert not os.path.exists(d + "/out.paths")


def test_evidence_in_an_internal_column_is_ignored_and_the_count_comes_first(tmp_path):
    """the count is printed before the first device call, so this runs with or without a GPU"""
    d = str(tmp_path)
    model, tree, fp = make_inputs(d)
    internal = [tree.node_names[b] for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] > 1]
    cols = leaves(tree) + internal
    ends = leaf_ends(tree, fp)
    # internal columns: contradicting data, soft values and rubbish; three soft leaf cells, one N, one n
    ends[[tree.node_names.index(c) for c in internal]] ^= 1
    tokens = {(c, s): ("0.7" if s % 3 else "N" if s % 2 else "7.5") for c in internal for s in range(fp.n_sites)}
    tokens.update({(leaves(tree)[0], 4): "0.125", (leaves(tree)[2], 150): "N", (leaves(tree)[1], 9): "n",
                   (leaves(tree)[1], 10): "1e-3", (leaves(tree)[1], 11): "0.999"})
    # 0.0, 1.0 and friends are data as well
    s0 = 20
    leaf = leaves(tree)[0]
    tokens[(leaf, s0)] = "1.0" if ends[tree.node_names.index(leaf), s0] else "0.0"
    write_probs(d + "/l.probs", tree, cols, ends, tokens)
    r = est_histories(d, "-l", d + "/l.probs", "-v")
    assert "[LEAF CELLS WITH EVIDENCE: 5 of %d]" % (len(leaves(tree)) * fp.n_sites) in r.stderr, r.stderr
    assert "no column" not in r.stderr and "input paths end in" not in r.stderr and "probability" not in r.stderr
    # ... and before the first device call
    if "GPU LAYOUT" in r.stderr:
        assert r.stderr.index("LEAF CELLS WITH EVIDENCE") < r.stderr.index("GPU LAYOUT")


def test_est_params_histories_checks_the_file_too(tmp_path):
    d = str(tmp_path)
    model, tree, fp = make_inputs(d)
    ends = leaf_ends(tree, fp)
    leaf = leaves(tree)[0]
    ends[tree.node_names.index(leaf), 3] ^= 1
    write_probs(d + "/l.probs", tree, leaves(tree), ends)
    cmd = [os.path.join(BIN, "epievo_est_params_histories"), "-i", "1", "-B", "2", "-L", "1", "-o", d + "/o.paths",
           "-p", d + "/o.param", "-l", d + "/l.probs", d + "/p.param", d + "/t.nwk", d + "/in.paths"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and ("leaf %s at site 3" % leaf) in r.stderr, r.stderr
    assert not os.path.exists(d + "/o.paths")
    write_probs(d + "/l2.probs", tree, leaves(tree), leaf_ends(tree, fp), {(leaf, 5): "1.5"})
    r = subprocess.run(cmd[:cmd.index("-l") + 1] + [d + "/l2.probs"] + cmd[cmd.index("-l") + 2:],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and ("leaf %s at site 5" % leaf) in r.stderr, r.stderr
    write_states(d + "/m.states", tree, leaves(tree), leaf_ends(tree, fp))
    r = subprocess.run(cmd[:-3] + ["-m", d + "/m.states"] + cmd[-3:], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "-l" in r.stderr and "-m" in r.stderr, r.stderr
    assert not os.path.exists(d + "/o.paths")


def test_abi_declares_the_evidence_entries():
    from epievo_amd.sampler import ABI_SYMBOLS
    from epievo_amd import driver
    assert "epv_set_leaf_evidence" in ABI_SYMBOLS and "epv_leaf_evidence_cells" in ABI_SYMBOLS
    assert "epvd_set_leaf_evidence" in driver.DRIVER_SYMBOLS
    text = open(os.path.join(_build.INCLUDE, "epievo_mi355x.h")).read()
    assert "int epv_set_leaf_evidence(epv_ctx *ctx, const float *p_state1);" in text
    assert "int epv_leaf_evidence_cells(epv_ctx *ctx, uint64_t *n_cells);" in text
    assert "bit  18" in text
