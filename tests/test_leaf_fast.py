"""EPV_OPT_LEAF_FAST without a GPU: what the planner of the device library (csrc/epv_plan.h,
through libepv_host.so) decides with option 32, the precondition of the GPU rows of test_leaf_fast_gpu.py on the
oracle alone, and the programs' help.

With the bit on a held mask or table no longer plans the first proposal kernel: the plan is the one the same context
would get with no cell held, with bits 17 / 18 added.  With the bit off it is the first kernel, as
test_leaf_matrix.py pins."""
import os
import subprocess

import numpy as np
import pytest

import test_kernel_matrix as km
import leaf_fast_cases as lf
from common import ref_test_model
from epievo_amd import _build, host
from test_leaf_matrix import check_leaf_states

DIRECT, DIRECT_FUSED, LEAF_FAST = 8, 16, 32
UNOBS_BIT, EVIDENCE_BIT, DIRECT_BIT = 1 << 17, 1 << 18, 1 << 23


def _inputs(tree, n):
    model, t = ref_test_model(), km.make_tree(tree)
    fp = host.simulate(model, t, n, 6)
    cap = int(max(16, 2 * fp.counts().max() + 8))
    return t, n, cap, fp.counts().sum() / (n * (t.n_nodes - 1))


def _word(inputs, options, env, unobs=0, evidence=0):
    return host.phase_plan(*inputs, options, unobs, evidence, knobs=env)["word"]


_PLAIN = [r for r in km.ROWS if not (r[5].get("reference_proposal_ratio") or r[5].get("sample_root"))]
_REFQ = [r for r in km.ROWS if r[5].get("reference_proposal_ratio") or r[5].get("sample_root")]


@pytest.mark.parametrize("row", _PLAIN, ids=[r[0] for r in _PLAIN])
def test_plan_with_held_cells_is_the_plan_without_them(row):
    """every row of test_kernel_matrix with default or forward-rejection options, and the same row under the direct
    sampler (which excludes forward rejection)"""
    id, tree, nodes, n, env, opts, expect = row
    inputs = _inputs(tree, n)
    base = sum(bit for name, bit in km.OPTION_BITS.items() if opts.get(name))
    for options in (base, (base & ~2) | DIRECT):
        plain = _word(inputs, options, env)
        assert _word(inputs, options | LEAF_FAST, env) == plain                      # no cell held: word for word
        for unobs, evidence in ((1, 0), (0, 1), (1, 1)):
            bits = (UNOBS_BIT if unobs else 0) | (EVIDENCE_BIT if evidence else 0)
            assert _word(inputs, options | LEAF_FAST, env, unobs, evidence) == plain | bits, (id, options, unobs, evidence)
            off = host.phase_plan(*inputs, options, unobs, evidence, knobs=env)
            assert off["propose"] == "V1" and off["word"] & (UNOBS_BIT | EVIDENCE_BIT) == bits, (id, options)
    if base == 0:
        assert host.plan_fields(_word(inputs, LEAF_FAST, env, 1, 1))["propose"] == expect["propose"]


@pytest.mark.parametrize("row", _REFQ, ids=[r[0] for r in _REFQ])
def test_reference_ratio_and_sample_root_keep_the_first_kernel(row):
    id, tree, nodes, n, env, opts, expect = row
    inputs = _inputs(tree, n)
    options = sum(bit for name, bit in km.OPTION_BITS.items() if opts.get(name))
    for unobs, evidence in ((0, 0), (1, 0), (0, 1), (1, 1)):
        plan = host.phase_plan(*inputs, options | LEAF_FAST, unobs, evidence, knobs=env)
        assert plan["propose"] == "V1" and plan["refq"], (id, plan)
        assert plan == host.phase_plan(*inputs, options, unobs, evidence, knobs=env)


@pytest.mark.parametrize("row", _PLAIN, ids=[r[0] for r in _PLAIN])
def test_direct_fused_with_a_held_cell_is_plain_direct_mode(row):
    """8 | 16 | 32 with a held cell: never the fused phase (its direct bodies have no leaf variant), bit 23 set, the
    plan of 8 | 32"""
    id, tree, nodes, n, env, opts, expect = row
    inputs = _inputs(tree, n)
    for unobs, evidence in ((1, 0), (0, 1), (1, 1)):
        plan = host.phase_plan(*inputs, DIRECT | DIRECT_FUSED | LEAF_FAST, unobs, evidence, knobs=env)
        assert plan["propose"] != "fused" and plan["word"] & DIRECT_BIT, (id, plan)
        assert plan == host.phase_plan(*inputs, DIRECT | LEAF_FAST, unobs, evidence, knobs=env)
    # (and with no cell held the fused direct bodies stay where they were)
    assert _word(inputs, DIRECT | DIRECT_FUSED | LEAF_FAST, env) == _word(inputs, DIRECT | DIRECT_FUSED, env)


def test_rows_name_every_leaf_variant():
    """the GPU rows reach the nine new instantiations, each with both contents where the issue asks for it"""
    seen = set((r["expect"]["propose"], r["expect"].get("small_nn"), r["expect"].get("jumps"), r["expect"].get("p3_words"))
               for r in lf.ROWS)
    for key in [("fused", 2, "fused", None), ("fused", 3, "fused", None), ("fused", 4, "fused", None),
                ("fused", 5, "fused", None), ("fused", 0, "fused", None), ("V2", 0, "jumps_all", 0),
                ("V2", 0, "segments", 0), ("V3", None, "jumps_all", 1), ("V3", None, "jumps_all", 2)]:
        assert key in seen, key
    assert set(r["expect"].get("fused_lanes") for r in lf.ROWS if r["expect"]["propose"] == "fused") == {16, 32, 64}
    assert len(lf.ROW) == len(lf.ROWS)
    for fam in ("fused", "V2", "V3"):
        assert any(r["opts"] == lf.FR and r["expect"]["propose"] == fam for r in lf.ROWS)
        assert any(r["content"] == "mask" and r["expect"]["propose"] == fam for r in lf.ROWS)
    assert all(r["n"] % 32 != 0 for r in lf.ROWS)


@pytest.mark.parametrize("row", lf.ROWS, ids=[r["id"] for r in lf.ROWS])
def test_row_plan_and_oracle_leg(row):
    """a GPU row's plan, decided here, and its precondition: the oracle's leg alone moves at least one soft cell and
    keeps every hard cell and both end sites"""
    case = lf.make_case(row)
    plan = lf.host_plan(row, case, lf.option_word(row))
    bad = dict((k, (v, plan[k])) for k, v in row["expect"].items() if plan[k] != v)
    assert not bad, "plan differs (expected, got): %r; plan %r" % (bad, plan)
    assert (plan["unobs"], plan["evidence"]) == (row["content"] != "all", row["content"] != "mask")
    assert lf.host_plan(row, case, lf.option_word(row, leaf_fast=False))["propose"] == "V1"
    assert plan["word"] == lf.host_plan(row, case, lf.option_word(row), held=False)["word"] | \
        (UNOBS_BIT if plan["unobs"] else 0) | (EVIDENCE_BIT if plan["evidence"] else 0)
    J, D, nacc, paths, tri, overflow = lf.oracle_leg_of(row, case)
    last = paths[-1] if row["mode"] == "overflow" else paths
    assert check_leaf_states(row, case, last) >= 1, row["id"]
    assert (overflow > 0) == (row["mode"] == "overflow")


@pytest.mark.parametrize("prog", ["epievo_est_histories", "epievo_est_params_histories"])
def test_programs_list_leaf_fast(prog):
    exe = os.path.join(_build.BIN_DIR, prog)
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert "leaf-fast" in r.stdout + r.stderr, (r.stdout + r.stderr)[-2000:]
