"""EPV_OPT_LEAF_FAST on the GPU: the leaf variants of the fused bodies, of the second and of
the third proposal kernel against the oracle's rung B, which takes masks and evidence itself (its own law is checked
without a GPU in test_leaf_oracle.py) -- never the new kernels against themselves.

Every case runs in a fresh child process (leaf_fast_gpu_child.py) with the EPV_* knobs of its row (leaf_fast_cases.py)
in the environment.  A row asserts the plan after reset() and that it equals host.phase_plan of what the context
holds, runs run_mcmc(2, 3, seed, sweep_base=4) and compares J, D, the accept count, the paths, tri_llh as uint64 and
the overflow counter bit for bit.  test_leaf_fast.py shows without a GPU that the oracle's leg of every row moves a
soft cell."""
import os
import subprocess
import sys

import numpy as np
import pytest

import leaf_fast_cases as lf
from common import simulate, TEST_PARAM_TEXT, TREE_NWK_TEXT
from epievo_amd import _build, host
from test_unobserved_leaves import leaf_ends, write_states, leaves
from test_leaf_evidence import write_probs

pytestmark = pytest.mark.gpu

_CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "leaf_fast_gpu_child.py")


def child(case, row_id):
    r = subprocess.run([sys.executable, _CHILD, case, row_id], env=dict(os.environ, **lf.ROW[row_id]["env"]),
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]


@pytest.mark.parametrize("row_id", [r["id"] for r in lf.ROWS])
def test_leaf_variant_matches_rung_b(row_id):
    child("row", row_id)


def test_contradicting_hard_cell_on_the_fused_phase():
    child("contradict", "tree")


@pytest.mark.parametrize("row_id", ["v2", "v3"])
def test_direct_sampler_equals_the_first_kernel(row_id):
    child("direct", row_id)


@pytest.mark.parametrize("row_id", ["tree", "v3"])
def test_cleared_content_and_the_option_toggled(row_id):
    child("identities", row_id)


def test_life_cycle_under_a_held_table():
    child("lifecycle", "tree")


def test_two_contexts_with_halos_equal_one_context():
    child("halos", "tree")


def test_sharded_driver_with_leaf_fast_equals_one_context():
    child("driver", "tree")


def test_programs_with_leaf_fast_write_the_same_files(tmp_path):
    """-m ... -f and -l ... -f: byte for byte the output files of the runs without -f (the first kernel, on rung B);
    -v names the proposal kernel beside the held cells, and -f alone is harmless"""
    d = str(tmp_path)
    model, tree, fp = simulate("tree", 600, seed=5)
    open(d + "/p.param", "w").write(TEST_PARAM_TEXT)
    open(d + "/t.nwk", "w").write(TREE_NWK_TEXT)
    host.write_paths(d + "/in.paths", tree.node_names, tree.branches, fp)
    ends = leaf_ends(tree, fp)
    rng = np.random.default_rng(9)
    cells = [(c, s) for c in leaves(tree) for s in range(1, fp.n_sites - 1) if rng.random() < 0.3]
    write_states(d + "/m.states", tree, leaves(tree), ends, missing=cells)
    write_probs(d + "/s.probs", tree, leaves(tree), ends, {c: "%.6f" % rng.uniform(0.05, 0.95) for c in cells})
    inputs = [d + "/p.param", d + "/t.nwk", d + "/in.paths"]

    def est(tag, *extra):
        r = subprocess.run([os.path.join(_build.BIN_DIR, "epievo_est_histories"), "-B", "20", "-L", "20", "-s", "3", "-v",
                            "-o", d + "/%s.paths" % tag, "-a", d + "/%s.avg" % tag, "-n", "2"] + list(extra) + inputs,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stderr, open(d + "/%s.paths" % tag, "rb").read(), open(d + "/%s.avg" % tag, "rb").read()

    def em(tag, *extra):
        r = subprocess.run([os.path.join(_build.BIN_DIR, "epievo_est_params_histories"), "-i", "2", "-B", "3", "-L", "2",
                            "-s", "4", "-v", "-o", d + "/%s.paths" % tag, "-p", d + "/%s.param" % tag] + list(extra) + inputs,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stderr, open(d + "/%s.paths" % tag, "rb").read(), open(d + "/%s.param" % tag, "rb").read()

    for prog in (est, em):
        for flag, path in (("-m", d + "/m.states"), ("-l", d + "/s.probs")):
            off, on = prog("off", flag, path), prog("on", flag, path, "-f")
            assert off[1:] == on[1:], (prog.__name__, flag)
            assert "LEAF CELLS: first]" in off[0] and "LEAF CELLS: fused phase, leaf variant]" in on[0], on[0][-1500:]
        plain, alone = prog("plain"), prog("alone", "--leaf-fast")
        assert plain[1:] == alone[1:] and "PROPOSAL KERNEL WITH" not in alone[0]
