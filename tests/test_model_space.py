"""The model space on the CPU: the rows of model_cases.py are what they claim, none of them is an unbounded
rejection search, and the parallel rung keeps the stationary law and the reference's arithmetic under models
other than test.param.  test_model_space_gpu.py then holds the device to rung B on the same rows."""
import functools

import numpy as np
import pytest

import model_cases as mc
import orc
import refvec
from epievo_amd import host
from test_mcmc_posterior import LEAF, ROOT, T_BRANCH, _check, _exact, _initial_paths

IDS = [r[0] for r in mc.ROWS]


@functools.lru_cache(maxsize=None)
def _run(rid, mode=()):
    """the oracle's rung B run of exactly what the GPU test runs -> the figures the tests below judge"""
    o = mc.oracle(rid, dict(mode))
    llh0 = o.tri_llh()
    J, D, nacc, acc = o.run_mcmc(2, 3, sweep_base=4)
    return dict(llh0=llh0, llh1=o.tri_llh(), nacc=nacc, acc=acc, counters=o.counters(), J=J, D=D)


def test_table_is_complete():
    """every model on every kernel family, every family with at least two models, unique ids, n within 130 .. 600,
    the trees the issue names, and nothing of UNRUNNABLE among the rows"""
    assert len(set(IDS)) == len(IDS)
    seen = {}
    for case, rid, env, expect, modes in mc.gpu_cases():
        r = mc.row(rid)
        fam = case[len(rid) + 1:]
        assert fam in mc.FAMILIES, case
        seen.setdefault(fam, set()).add(r[2])
        assert modes[0] == {} and all(m in ({}, mc.REF, mc.FR) for m in modes)
    for fam in mc.FAMILIES:
        assert seen[fam] >= {"anti", "mixed", "slow", "fast", "skewm", "skew", "ratio"}, (fam, seen[fam])
    for r in mc.ROWS:
        assert 130 <= r[5] <= 600 and r[1] in mc.MODELS and r[2] in mc.MODELS, r[0]
        assert set(r[6]) <= set(mc.LABELS), r[0]
        assert (r[1], r[2], r[3], r[5]) not in mc.UNRUNNABLE
        # the models whose mismatch rows fail the work bound sample only their own data
        assert r[2] not in ("skew", "ratio") or r[1] == r[2], r[0]
        assert mc.REF in mc.row_modes(r[0]), r[0]
    assert set(r[3] for r in mc.ROWS) == {"pair", "tree", "star5", "cat6", "bal16", "bal64"}
    for lab in ("silent", "underflow", "tiny", "ratio6", "mismatch", "model-overflow"):
        assert sum(lab in r[6] for r in mc.ROWS) >= 2, lab


def test_models_are_the_regimes_they_name():
    rate = {m: mc.model(m).rates for m in mc.MODELS}
    assert np.array_equal(rate["slow"], rate["ref"] * 1e-9) and np.array_equal(rate["fast"], rate["ref"] * 100.0)
    assert rate["slow"].max() < 1.1e-8 and rate["fast"].max() > 1000
    assert rate["anti"].max() / rate["anti"].min() > 300 and rate["anti"][0] == rate["anti"][7] > 75
    assert 5e5 < rate["mixed"].max() / rate["mixed"].min() < 1e6
    assert rate["skew"].max() > 2e5 and rate["skew"].max() / rate["skew"].min() > 1e7
    assert 2000 < rate["skewm"].max() < 2500
    assert rate["ratio"].max() / rate["ratio"].min() > 1e9
    # the pairs (r0, r1) of the single-segment matrix table, eight orders apart in ratio
    r = rate["ratio"]
    assert sorted(r[t] / r[t | 2] for t in (0, 1, 4, 5))[2] > 1e6
    for m in mc.MODELS:
        assert np.all(np.isfinite(np.log(rate[m]))) and np.all(rate[m] > 0)


@pytest.mark.parametrize("rid", IDS)
def test_row_preconditions(rid):
    r = mc.row(rid)
    labels, (acc, tps, ovf) = set(r[6]), r[7]
    res = _run(rid)
    c = res["counters"]
    want = mc.computed_labels(rid)
    if c["overflow"]:
        want.add("model-overflow")
    assert labels - {"accept-all", "fr"} == want, (labels, want)
    # the cached triple likelihoods of the interior sites, before and after
    assert np.all(np.isfinite(res["llh0"][1:-1])) and np.all(np.isfinite(res["llh1"][1:-1]))
    proposals = 3 * (r[5] - 2)
    assert res["nacc"] > 0
    if "accept-all" in labels:
        assert res["nacc"] == proposals
    else:
        assert res["nacc"] < proposals       # accepted and rejected proposals are both compared
    assert (c["overflow"] > 0) == ("model-overflow" in labels)
    # the figures the table records are those of this run
    print(rid, "acceptance %.3f trials / segment %.2f overflow %d" % (res["acc"], mc.work(c), c["overflow"]))
    assert round(res["acc"], 3) == acc and round(mc.work(c), 2) == tps and c["overflow"] == ovf
    assert np.all(np.isfinite(res["J"])) and np.all(np.isfinite(res["D"]))


@pytest.mark.parametrize("rid", IDS)
def test_row_meets_the_work_bound(rid):
    """a condition, not a measurement: trials / segments <= 64 in every mode in which the row reaches the device.
    This is what keeps an unbounded rejection search off the GPU."""
    labels = set(mc.row(rid)[6])
    for mode in mc.row_modes(rid):
        if mode.get("forward_rejection"):
            # a flip under forward rejection needs about 1 / P trials
            assert "tiny" not in labels and mc.row(rid)[2] != "slow", rid
        c = _run(rid, tuple(sorted(mode.items())))["counters"]
        print(rid, mode, "trials / segment %.2f" % mc.work(c))
        assert c["segments"] > 0 and mc.work(c) <= mc.WORK_BOUND, (rid, mode, c)


def test_tight_capacity_row_overflows():
    """the tight-capacity GPU test's precondition: fast on tree at the input's own maximum jump count overflows in
    both sweeps, within the work bound"""
    mod, tree, fp, roomy = mc.workload("fast-tree")
    cap2 = int(fp.counts().max())
    assert 0 < cap2 < roomy
    o = mc.oracle("fast-tree", cap=cap2, seed=23)
    for w in range(2):
        before = o.counters()["overflow"]
        o.sweep(w)
        assert o.counters()["overflow"] > before
    assert mc.work(o.counters()) <= mc.WORK_BOUND


# ---------------------------------------------------------------- changing models
SEQUENCE = ("ref", "fast", "slow", "mixed", "ref")
SEQUENCE_SCALE = (2, 0.5)         # after the model of this index: every branch times this (scale_jump_times)
SEQUENCE_CAP = 24


def changing_models(ctx, tree, seed=None):
    """one context (an Oracle, or a DeviceSampler with its seed) through set_model over SEQUENCE, scale_jump_times
    after SEQUENCE_SCALE[0], run_mcmc(1, 2) after each -> per step (J, D, accepted, paths, tri_llh, capacity).
    A run_mcmc that overflowed doubles the capacity for the calls after it: the device by auto_grow (what
    SingleSiteSampler sets), the oracle here by the same rule."""
    from epievo_amd.sampler import MAX_CAPACITY
    out, cap = [], SEQUENCE_CAP
    for i, name in enumerate(SEQUENCE):
        ctx.set_model(mc.model(name))
        ctx.reset()
        if seed is None:
            before = ctx.counters()["overflow"]
            J, D, nacc, _ = ctx.run_mcmc(1, 2, sweep_base=3 * i)
            if ctx.counters()["overflow"] > before and cap < MAX_CAPACITY:
                cap = min(MAX_CAPACITY, 2 * cap)
                ctx.set_rung("B", cap)
        else:
            assert ctx.auto_grow
            J, D, nacc = ctx.run_mcmc(1, 2, seed, sweep_base=3 * i)
            cap = ctx.capacity()
        out.append((J, D, nacc, ctx.paths(), ctx.tri_llh(), cap))
        if i == SEQUENCE_SCALE[0]:
            ctx.scale_jump_times(tree.branches * SEQUENCE_SCALE[1])
    return out


def changing_models_input():
    tree = mc.scaled_tree("tree", 1)
    return tree, host.simulate(mc.model("ref"), tree, 300, mc.SIM_SEED)


def test_changing_models_sequence_is_runnable():
    """the oracle through the sequence the GPU test takes: finite throughout, something accepted at every step,
    within the work bound, and the model in force is the one set last (the first and last steps, both test.param,
    differ only by the paths they start from)"""
    tree, fp = changing_models_input()
    o = orc.Oracle(tree, mc.model("ref"), fp, "B", cap=SEQUENCE_CAP, seed=mc.ORACLE_SEED)
    steps = changing_models(o, tree)
    assert mc.work(o.counters()) <= mc.WORK_BOUND
    for J, D, nacc, paths, llh, cap in steps:
        assert nacc > 0 and np.all(np.isfinite(llh[1:-1])) and np.all(np.isfinite(D))
    # the fast step overflows the 24 slots: the steps after it run at the doubled capacity
    assert [s[5] for s in steps] == [SEQUENCE_CAP] + [2 * SEQUENCE_CAP] * 4
    # the same steps on fresh oracles that were given each model at creation
    o2 = orc.Oracle(tree, mc.model("ref"), fp, "B", cap=SEQUENCE_CAP, seed=mc.ORACLE_SEED)
    o2.reset()
    J, D, nacc, _ = o2.run_mcmc(1, 2, sweep_base=0)
    assert nacc == steps[0][2] and np.array_equal(J, steps[0][0]) and np.array_equal(D, steps[0][1])
    o3 = orc.Oracle(tree, mc.model("fast"), o2.paths(), "B", cap=SEQUENCE_CAP, seed=mc.ORACLE_SEED)
    o3.reset()
    J, D, nacc, _ = o3.run_mcmc(1, 2, sweep_base=3)
    assert nacc == steps[1][2] and np.array_equal(J, steps[1][0]) and np.array_equal(D, steps[1][1])
    assert orc.paths_equal(o3.paths(), steps[1][3])


# ---------------------------------------------------------------- the law
# the single-branch case of test_mcmc_posterior.py (ROOT, T = 0.4), its criteria, chain lengths and seeds unchanged
LAW_LEAF = {
    "anti": LEAF,
    # mixed: orc_exact_posterior keeps 7660 of its 20 000 draws within its budget of 4e8 simulations with LEAF (an
    # isolated 1 dies at rate 125), so the leaf pattern is another one with two interior flips and the ends unchanged
    "mixed": np.array([0, 1, 1, 1, 0, 0, 0, 1], np.uint8),
}
LAW_MODELS = tuple(LAW_LEAF)


def law_case(name):
    """-> (exact posterior moments, initial paths) of the single-branch case under the model, with its leaf pattern
    in the place of test_mcmc_posterior.LEAF while _exact and _initial_paths read it"""
    import test_mcmc_posterior as tp
    old = tp.LEAF
    tp.LEAF = LAW_LEAF[name]
    try:
        return _law_exact(name), _initial_paths()
    finally:
        tp.LEAF = old


@functools.lru_cache(maxsize=None)
def _law_exact(name):
    return _exact(mc.model(name))


@pytest.mark.parametrize("name", LAW_MODELS)
def test_rung_b_chain_matches_exact_posterior(name):
    """rung B against 20 000 exact posterior draws under a model other than test.param: chain length, seed and
    criteria of test_mcmc_posterior.test_oracle_chains_match_exact_posterior.

    Measured, rung B, worst deviation as a share of the tolerance: anti 0.33 (seed 17, 30 000 sweeps) and 0.30
    (seed 99, 20 000, the GPU twin's chain); mixed at most 0.18 over eight seeds at either length.
    The criteria assume one effective draw per ten sweeps.  Under these models single-site updates mix more slowly
    than that where neighbouring sites are strongly coupled, which is why the reference-schedule rung is not
    held to them here: under anti its seed 17 gives J[000] = 0.165 against 0.110 (tolerance 0.053) at 30 000 sweeps
    and 0.120 at 300 000, its seeds 18 and 19 give 0.098; under mixed with leaf 0 1 1 0 0 0 0 1 a chain sat for
    thousands of sweeps in a mode where both sites of the 1 1 block die and are born again.  Chains of 200 000 and
    300 000 sweeps of both rungs agree with 100 000 exact draws (model limits)."""
    exact, start = law_case(name)
    assert len(ROOT) == len(LAW_LEAF[name]) == 8 and LAW_LEAF[name][0] == ROOT[0] and LAW_LEAF[name][-1] == ROOT[-1]
    assert int((LAW_LEAF[name] != ROOT).sum()) == 2
    o = orc.Oracle(host.Tree.single_branch(T_BRANCH), mc.model(name), start, "B", cap=48, seed=17)
    o.reset()
    J, D, nacc, acc = o.run_mcmc(500, 30000)
    _check(J, D, 3000.0, exact)
    # what lets the GPU twins run: the chain they repeat bit for bit stays within the work bound and the capacity
    o = orc.Oracle(host.Tree.single_branch(T_BRANCH), mc.model(name), start, "B", cap=48, seed=99)
    o.reset()
    o.run_mcmc(500, 20000)
    assert mc.work(o.counters()) <= mc.WORK_BOUND and o.counters()["overflow"] == 0


# ---------------------------------------------------------------- rung A against the linked reference
@pytest.mark.parametrize("sampler", ("anti", "fast"))
def test_rung_a_vs_linked_reference_on_mismatched_data(sampler):
    """data of test.param (tree.nwk, n = 60) under another model: the reference-schedule rung against the LINKED
    reference, live (against its stored outputs, tests/golden/ref/, where oracle/_ref is absent) -- the
    mechanism of test_fuzz.py"""
    tree = mc.scaled_tree("tree", 1)
    model = mc.model(sampler)
    fp = host.simulate(mc.model("ref"), tree, 60, mc.SIM_SEED)
    seed = 20240 + len(sampler)

    def reference():
        R = orc.Reference(tree, model, fp, seed=seed)
        R.reset(1, 2)
        llh0 = R.tri_llh()
        Jr, Dr, accr = R.run_mcmc()
        return dict(llh0=llh0, J=Jr, D=Dr, acc=np.float64(accr), **refvec.pack_paths("paths", R.paths()))

    r = refvec.reference_outputs("model_space_ref_%s" % sampler, reference)
    o = orc.Oracle(tree, model, fp, "A", seed=seed)
    o.reset()
    assert np.array_equal(o.tri_llh(), r["llh0"])
    Jo, Do, nacc, acc = o.run_mcmc(1, 2)
    assert 0 < nacc < 2 * 58
    assert np.array_equal(Jo, r["J"]) and np.array_equal(Do, r["D"]) and acc == float(r["acc"])
    assert orc.paths_equal(o.paths(), refvec.unpack_paths("paths", r))
