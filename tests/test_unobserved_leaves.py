"""Missing leaf data, the parts that run without a GPU: the -m/--missing states file of the E-step
programs is checked against the input paths before any device call."""
import os
import subprocess

import numpy as np
import pytest

from common import simulate, TEST_PARAM_TEXT, TREE_NWK_TEXT
from epievo_amd import _build, host

BIN = _build.BIN_DIR


def leaf_ends(tree, fp):
    """[node][site] end state of every branch's path (row 0 unused)"""
    B, n = tree.n_nodes - 1, fp.n_sites
    es = fp.init.reshape(B, n) ^ (fp.counts().reshape(B, n) & 1).astype(np.uint8)
    return np.vstack([np.zeros((1, n), np.uint8), es])


def write_states(path, tree, cols, ends, missing=()):
    """a states file with the columns `cols` (node names) holding `ends`; (name, site) in `missing` -> N"""
    miss = set(missing)
    idx = [tree.node_names.index(c) for c in cols]
    with open(path, "w") as f:
        f.write("#" + "\t".join(cols) + "\n")
        for s in range(ends.shape[1]):
            f.write("%d\t%s\n" % (s, "\t".join("N" if (c, s) in miss else str(int(ends[i, s])) for c, i in zip(cols, idx))))


def make_inputs(d, n=200, seed=5):
    model, tree, fp = simulate("tree", n, seed=seed)
    open(d + "/p.param", "w").write(TEST_PARAM_TEXT)
    open(d + "/t.nwk", "w").write(TREE_NWK_TEXT)
    host.write_paths(d + "/in.paths", tree.node_names, tree.branches, fp)
    return model, tree, fp


def est_histories(d, missing, *extra):
    cmd = [os.path.join(BIN, "epievo_est_histories"), "-B", "2", "-L", "1", "-s", "3", "-o", d + "/out.paths",
           "-m", missing] + list(extra) + [d + "/p.param", d + "/t.nwk", d + "/in.paths"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def leaves(tree):
    return [tree.node_names[b] for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1]


def test_missing_file_that_contradicts_the_paths_is_refused(tmp_path):
    d = str(tmp_path)
    model, tree, fp = make_inputs(d)
    ends = leaf_ends(tree, fp)
    leaf = leaves(tree)[1]
    ends[tree.node_names.index(leaf), 57] ^= 1
    write_states(d + "/m.states", tree, leaves(tree), ends, missing=[(leaves(tree)[0], 10)])
    r = est_histories(d, d + "/m.states")
    assert r.returncode != 0
    assert ("leaf %s at site 57" % leaf) in r.stderr, r.stderr
    assert not os.path.exists(d + "/out.paths")


def test_missing_file_without_a_leaf_column_is_refused(tmp_path):
    d = str(tmp_path)
    model, tree, fp = make_inputs(d)
    cols = leaves(tree)[:-1]
    write_states(d + "/m.states", tree, cols, leaf_ends(tree, fp))
    r = est_histories(d, d + "/m.states")
    assert r.returncode != 0
    assert "no column for leaf %s" % leaves(tree)[-1] in r.stderr, r.stderr


def test_missing_file_with_too_few_rows_is_refused(tmp_path):
    d = str(tmp_path)
    model, tree, fp = make_inputs(d)
    write_states(d + "/m.states", tree, leaves(tree), leaf_ends(tree, fp)[:, :-1])
    r = est_histories(d, d + "/m.states")
    assert r.returncode != 0 and "sites" in r.stderr, r.stderr


def test_n_in_an_internal_node_column_is_ignored(tmp_path):
    """the count is printed before the first device call, so this runs with or without a GPU"""
    d = str(tmp_path)
    model, tree, fp = make_inputs(d)
    internal = [tree.node_names[b] for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] > 1]
    cols = leaves(tree) + internal
    ends = leaf_ends(tree, fp)
    # internal columns: garbage and N everywhere; two leaf cells missing, one of them at a leaf lowercase
    ends[[tree.node_names.index(c) for c in internal]] ^= 1
    miss = [(c, s) for c in internal for s in range(fp.n_sites)] + [(leaves(tree)[0], 4), (leaves(tree)[2], 150)]
    write_states(d + "/m.states", tree, cols, ends, missing=miss)
    text = open(d + "/m.states").read().replace("\tN\n", "\tn\n", 1)
    open(d + "/m.states", "w").write(text)
    r = est_histories(d, d + "/m.states", "-v")
    assert "[UNOBSERVED LEAF CELLS: 2 of %d]" % (len(leaves(tree)) * fp.n_sites) in r.stderr, r.stderr
    assert "no column" not in r.stderr and "input paths end in" not in r.stderr


def test_est_params_histories_checks_the_file_too(tmp_path):
    d = str(tmp_path)
    model, tree, fp = make_inputs(d)
    ends = leaf_ends(tree, fp)
    leaf = leaves(tree)[0]
    ends[tree.node_names.index(leaf), 3] ^= 1
    write_states(d + "/m.states", tree, leaves(tree), ends)
    cmd = [os.path.join(BIN, "epievo_est_params_histories"), "-i", "1", "-B", "2", "-L", "1", "-o", d + "/o.paths",
           "-m", d + "/m.states", d + "/p.param", d + "/t.nwk", d + "/in.paths"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and ("leaf %s at site 3" % leaf) in r.stderr, r.stderr


def test_abi_declares_the_mask_entries():
    from epievo_amd.sampler import ABI_SYMBOLS
    from epievo_amd import driver
    assert "epv_set_unobserved" in ABI_SYMBOLS and "epv_unobserved_cells" in ABI_SYMBOLS
    assert "epvd_set_unobserved" in driver.DRIVER_SYMBOLS
    text = open(os.path.join(_build.INCLUDE, "epievo_mi355x.h")).read()
    assert "bit  17" in text
