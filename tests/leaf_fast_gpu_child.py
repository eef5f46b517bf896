"""Child process of test_leaf_fast_gpu.py: one case of EPV_OPT_LEAF_FAST on the GPU, with the EPV_* knobs of its row in
the environment (a context reads them when it is created).  argv: the case's name, then a row id of leaf_fast_cases.
Prints "ok" and the plan that ran."""
import json
import os
import sys

_TESTS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_TESTS))
sys.path.insert(0, _TESTS)

import numpy as np

import orc
import leaf_fast_cases as lf
from epievo_amd import host
from epievo_amd.sampler import DeviceSampler
from test_leaf_matrix import apply_options, check_leaf_states, make_oracle

DIRECT, DIRECT_FUSED, LEAF_FAST = 8, 16, 32


def device(row, case, cap=None, leaf_fast=True, held=True, sites=None, halo=None):
    model, tree, fp, mask, r, cap0 = case
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    if sites:
        lo, hi = sites
        d.upload_paths(fp.slice_sites(lo, hi), cap or cap0, lo, fp.n_sites)
        d.set_halo(*halo)
        mask, r = (None if mask is None else mask[:, lo:hi]), (None if r is None else r[:, lo:hi])
    else:
        d.upload_paths(fp, cap or cap0)
    d.set_options(**row["opts"])
    d.set_leaf_fast(leaf_fast)
    if held:
        d.set_unobserved(mask)
        d.set_leaf_evidence(r)
    d.reset()
    return d


def check_plan(row, case, d, expect=None):
    """the row's fields, bits 17 / 18 of what is held, and the planner without a GPU on what the context holds"""
    plan = d.phase_plan()
    expect = row["expect"] if expect is None else expect
    bad = dict((k, (v, plan[k])) for k, v in expect.items() if plan[k] != v)
    assert not bad, "plan differs (expected, got): %r; plan %r" % (bad, plan)
    model, tree, fp, mask, r, cap = case
    kbar = fp.counts().sum() / (fp.n_sites * (tree.n_nodes - 1))
    assert host.phase_plan(tree, fp.n_sites, d.capacity(), kbar, d.options(), d.unobserved_cells(), d.leaf_evidence_cells(),
                           knobs=row["env"]) == plan
    return plan


def same_as_oracle(d, o):
    assert orc.paths_equal(d.paths(), o.paths())
    assert np.array_equal(d.tri_llh().view(np.uint64), o.tri_llh().view(np.uint64))
    assert d.counters()["overflow"] == o.counters()["overflow"]


def run_row(row):
    case = lf.make_case(row)
    d = device(row, case)
    plan = check_plan(row, case, d)
    assert d.options() & LEAF_FAST and d.phase_mode() != 0
    assert (plan["unobs"], plan["evidence"]) == (row["content"] != "all", row["content"] != "mask")
    Jo, Do, no, po, to, ovo = lf.oracle_leg_of(row, case)
    if row["mode"] == "overflow":
        for w in range(2):
            try:
                d.sweep(1, row["seed"], sweep_base=w)
            except Exception as e:
                assert "rejected" in str(e) or "capacity" in str(e).lower(), e
            assert orc.paths_equal(d.paths(), po[w]), "paths differ after overflow sweep %d" % w
        assert ovo > 0 and d.counters()["overflow"] == ovo
        assert np.array_equal(d.tri_llh().view(np.uint64), to.view(np.uint64))
        assert check_leaf_states(row, case, po[-1]) >= 1
        check_leaf_states(row, case, d.paths())
        return plan
    Jd, Dd, nd = d.run_mcmc(2, 3, row["seed"], sweep_base=4)
    assert nd == no, (nd, no)
    assert np.array_equal(Jd, Jo) and np.array_equal(Dd, Do)
    pd = d.paths()
    assert orc.paths_equal(pd, po)
    assert np.array_equal(d.tri_llh().view(np.uint64), to.view(np.uint64))
    assert d.counters()["overflow"] == ovo
    assert d.phase_plan() == plan
    assert check_leaf_states(row, case, po) >= 1
    check_leaf_states(row, case, pd)
    d.close()
    return plan


def run_contradict(row):
    """a hard cell against the resident path: the GPU decides what the oracle decides, sweep by sweep"""
    from test_leaf_oracle import contradicting_case, check_repair
    model, tree, fp, r, cells = contradicting_case()
    cap = int(max(16, 2 * fp.counts().max() + 8))
    case = (model, tree, fp, None, r, cap)
    d = device(row, case)
    plan = check_plan(row, case, d)
    assert plan["evidence"] and not plan["unobs"]
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=29)
    apply_options(o, row["opts"])
    o.set_leaf_evidence(r)
    o.reset()
    snaps = []
    for w in range(5):
        assert d.sweep(1, 29, sweep_base=w) == o.sweep(w)
        snaps.append(d.paths())
        same_as_oracle(d, o)
    Jd, Dd = d.suffstats()
    Jo, Do = o.suffstats()
    assert np.array_equal(Jd, Jo) and np.array_equal(Dd, Do) and np.isfinite(d.tri_llh()).all()
    assert check_repair(tree, fp, snaps, cells) == len(cells)
    return plan


def run_direct(row):
    """the direct sampler (the oracle has none): 8 | 32 against 8 alone, which is the first kernel with the direct
    jump kernels; 8 | 16 | 32 is unfused and gives the same bits"""
    case = lf.make_case(row)
    res = {}
    for tag, bits in (("v1", DIRECT), ("fast", DIRECT | LEAF_FAST), ("fast-fused", DIRECT | DIRECT_FUSED | LEAF_FAST)):
        d = device(row, case, leaf_fast=bool(bits & LEAF_FAST))
        d.set_direct_sampler(True, fused=bool(bits & DIRECT_FUSED))
        d.reset()
        assert d.options() == bits
        plan = d.phase_plan()
        assert plan["direct"] and plan["evidence"] and plan["unobs"]
        if tag == "v1":
            assert plan["propose"] == "V1"
        else:
            check_plan(row, case, d, dict(row["expect"], jumps="segments" if row["expect"]["jumps"] == "segments" else "jumps"))
            assert plan["propose"] == row["expect"]["propose"] != "fused"
        J, D, nacc = d.run_mcmc(2, 3, row["seed"], sweep_base=4)
        res[tag] = (J, D, nacc, d.paths(), d.direct_giveups(), plan["word"])
        d.close()
    a = res["v1"]
    for tag in ("fast", "fast-fused"):
        b = res[tag]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[4] == b[4], tag
        assert orc.paths_equal(a[3], b[3]), tag
    assert res["fast"][5] == res["fast-fused"][5]
    assert check_leaf_states(row, case, a[3]) >= 1
    return res["fast"][5]


def run_identities(row):
    """option on, mask and table cleared = no option; option toggled off after a run = the first kernel, and the
    continued chain stays on the oracle"""
    case = lf.make_case(row)
    plain = device(row, case, leaf_fast=False, held=False)
    on = device(row, case)
    on.set_unobserved(None)
    on.set_leaf_evidence(None)
    on.reset()
    assert on.options() & LEAF_FAST and on.phase_plan()["word"] == plain.phase_plan()["word"]
    ra, rb = plain.run_mcmc(2, 3, row["seed"], sweep_base=4), on.run_mcmc(2, 3, row["seed"], sweep_base=4)
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2]
    assert orc.paths_equal(plain.paths(), on.paths())
    assert np.array_equal(plain.tri_llh().view(np.uint64), on.tri_llh().view(np.uint64))
    plain.close()
    on.close()
    d, o = device(row, case), make_oracle(row, case)
    check_plan(row, case, d)

    def step(base):
        Jd, Dd, nd = d.run_mcmc(1, 2, row["seed"], sweep_base=base)
        Jo, Do, no, _ = o.run_mcmc(1, 2, sweep_base=base)
        assert nd == no and np.array_equal(Jd, Jo) and np.array_equal(Dd, Do)
        same_as_oracle(d, o)

    step(0)
    d.set_leaf_fast(False)
    plan = d.phase_plan()
    assert plan["propose"] == "V1" and plan["evidence"] and plan["unobs"] and d.phase_mode() == 0
    step(3)
    d.set_leaf_fast(True)
    check_plan(row, case, d)
    step(6)
    return plan


def run_lifecycle(row):
    """set_capacity, scale_jump_times and set_model under a held table with the option on"""
    case = lf.make_case(row)
    model, tree, fp, mask, r, cap = case
    d, o = device(row, case), make_oracle(row, case)
    plan = check_plan(row, case, d)

    def step(base):
        Jd, Dd, nd = d.run_mcmc(1, 2, row["seed"], sweep_base=base)
        Jo, Do, no, _ = o.run_mcmc(1, 2, sweep_base=base)
        assert nd == no and np.array_equal(Jd, Jo) and np.array_equal(Dd, Do)
        same_as_oracle(d, o)
        assert d.phase_plan() == plan            # (the row's kernel, bits 17 / 18: kept)

    step(0)
    cells = (d.unobserved_cells(), d.leaf_evidence_cells())
    d.set_capacity(cap + 4)                      # (2 C + 1 <= 64 segments on a branch: the fused phase's limit)
    o.set_rung("B", cap + 4)
    apply_options(o, row["opts"])
    assert (d.unobserved_cells(), d.leaf_evidence_cells()) == cells and 2 * (cap + 4) + 1 <= 64
    step(3)
    nb = tree.branches * 1.03
    d.scale_jump_times(nb)
    o.scale_jump_times(nb)
    d.reset()
    o.reset()
    step(6)
    m2 = host.Model(model.rates * np.array([1.0, 1.1, 0.9, 1.0, 1.05, 1.0, 0.95, 1.0]), model.T, model.baseline)
    d.set_model(m2)
    o.set_model(m2)
    d.reset()
    o.reset()
    assert (d.unobserved_cells(), d.leaf_evidence_cells()) == cells and d.options() & LEAF_FAST
    step(9)
    assert check_leaf_states(row, case, o.paths()) >= 1
    return plan


def run_halos(row):
    """one genome cut by hand at a site that is no multiple of 32 into two contexts with halos"""
    from epievo_amd.parallel import concat_sites
    case = lf.make_case(row)
    model, tree, fp, mask, r, cap = case
    n, cut, H = fp.n_sites, 1013, 34               # 5 sweeps = 15 colour phases need 30 halo columns
    one = device(row, case)
    plan = check_plan(row, case, one)
    counts, nacc = one.run_mcmc_counts(2, 3, row["seed"], sweep_base=4)
    parts = [device(row, case, sites=(0, cut + H), halo=(0, H)), device(row, case, sites=(cut - H, n), halo=(H, 0))]
    for d in parts:
        p = d.phase_plan()
        assert p["propose"] == row["expect"]["propose"] and p["evidence"] and p["unobs"] and d.halo_phases_left() >= 15
    res = [d.run_mcmc_counts(2, 3, row["seed"], sweep_base=4) for d in parts]
    assert np.array_equal(res[0][0] + res[1][0], counts) and res[0][1] + res[1][1] == nacc
    got = concat_sites([parts[0].paths().slice_sites(0, cut), parts[1].paths().slice_sites(H, n - cut + H)])
    assert orc.paths_equal(got, one.paths())
    Jo, Do, no, po, to, _ = lf.oracle_leg_of(row, case)
    J, D = one.counts_to_stats(counts, 3)
    assert np.array_equal(J, Jo) and np.array_equal(D, Do) and nacc == no and orc.paths_equal(got, po)
    return plan


def run_driver(row):
    """the C++ driver with three contexts and set_leaf_fast, mask and table sliced by the driver, against one context
    and the oracle; the option stays over a later reset"""
    from epievo_amd import driver
    case = lf.make_case(row)
    model, tree, fp, mask, r, cap = case
    exp, o = [], make_oracle(row, case)
    for it in range(2):
        o.reset()
        J, D, nacc, _ = o.run_mcmc(1, 2, sweep_base=it * 3)
        exp.append((J, D, nacc / float(2 * (fp.n_sites - 2))))
    modes = []
    for devices in ([0], [0, 0, 0]):
        s = driver.CppSampler(1, 2, devices=devices, capacity=cap)
        s.set_leaf_fast(True)
        s.set_options(**row["opts"])               # (leaves bit 32 alone)
        s.set_unobserved(mask)
        s.set_leaf_evidence(r)
        s.reset(model, tree, fp)
        for it in range(2):
            if it:
                s.reset(model)
            assert s.phase_mode() != 0
            J, D, acc = s.run_mcmc(row["seed"], it)
            assert np.array_equal(J, exp[it][0]) and np.array_equal(D, exp[it][1]) and acc == exp[it][2], devices
        assert orc.paths_equal(s.paths(), o.paths()), devices
        modes.append(s.phase_mode())
        s.set_leaf_fast(False)
        assert s.phase_mode() == 0
        s.close()
    return modes


CASES = dict(row=run_row, contradict=run_contradict, direct=run_direct, identities=run_identities, lifecycle=run_lifecycle,
             halos=run_halos, driver=run_driver)

if __name__ == "__main__":
    print("ok", json.dumps(CASES[sys.argv[1]](lf.ROW[sys.argv[2]])))
