"""One GPU run of tests/test_direct_fused_gpu.py in a process of its own (a context reads its EPV_* knobs when it is
created, and the unrunnable row runs under a time limit): python direct_fused_gpu_child.py '<json spec>'.  Prints one
line "ok <json>" with what the parent compares.

A spec is direct_gpu_child.py's (kind, input, opts, expect, ...) with two more fields: "fused" -- the keyword of
set_direct_sampler, EPV_OPT_DIRECT_FUSED -- and, optionally, "cap", the capacity the paths are uploaded with (the
fused phase takes at most 31 slots).  The plan is asserted BEFORE the first launch of a colour phase: a row that
expects the fused direct body can never run a default-mode search by accident."""
import json
import os
import sys
import time

import numpy as np

_TESTS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_TESTS))
sys.path.insert(0, _TESTS)

from direct_gpu_child import _checked_run, _inputs, _replay, _sha      # noqa: E402
from epievo_amd import host                                             # noqa: E402
from epievo_amd.sampler import DeviceSampler                            # noqa: E402


def inputs(spec):
    model, tree, fp, cap = _inputs(spec)
    return model, tree, fp, int(spec.get("cap") or cap)


def set_options(d, spec):
    """the keywords of set_options, then the direct sampler with the row's `fused` through its own call"""
    d.set_options(**spec.get("opts", {}))
    d.set_direct_sampler(True, fused=bool(spec["fused"]))


def check_plan(plan, spec):
    bad = dict((k, (v, plan[k])) for k, v in spec["expect"].items() if plan[k] != v)
    assert not bad, "plan differs (expected, got): %r; plan %r" % (bad, plan)
    assert plan["direct"], plan
    if spec.get("must_fuse", spec["fused"]):
        assert plan["propose"] == "fused" and plan["jumps"] == "fused" and plan["accept"] == "fused", plan
    else:
        assert plan["propose"] != "fused", plan


def leaf_rows(tree):
    return [b - 1 for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1]


def extras(d, spec, tree, fp):
    """what makes the fused phase ineligible besides the options: unobserved leaf cells, leaf evidence"""
    B, n = tree.n_nodes - 1, fp.n_sites
    rng = np.random.RandomState(5)
    if spec.get("unobserved"):
        m = np.zeros((B, n), np.uint8)
        for r in leaf_rows(tree):
            m[r] = rng.rand(n) < 0.2
        d.set_unobserved(m)
    if spec.get("evidence"):
        e = np.full((B, n), np.nan, np.float32)
        for r in leaf_rows(tree):
            hit = rng.rand(n) < 0.2
            e[r, hit] = rng.uniform(0.1, 0.9, int(hit.sum())).astype(np.float32)
        d.set_leaf_evidence(e)


def context(spec, model, tree, fp, cap):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    extras(d, spec, tree, fp)
    set_options(d, spec)
    # an overflow leaves a valid chain and complete outputs; this only keeps run_mcmc from raising (the slots are
    # doubled BEHIND the call, and the wider slots take another plan: 2 C + 1 > 64 leaves the fused phase)
    d.auto_grow = bool(spec.get("overflows"))
    check_plan(d.phase_plan(), spec)          # before reset() and before any colour phase
    d.reset()
    plan = d.phase_plan()
    check_plan(plan, spec)
    # the planner without a GPU, given what this context holds, decides the same word for word (bit 23 and the
    # EPV_OPT_DIRECT_FUSED rule included)
    kbar = fp.counts().sum() / (fp.n_sites * (tree.n_nodes - 1))
    knobs = dict((k, v) for k, v in os.environ.items() if k.startswith("EPV_"))
    assert host.phase_plan(tree, fp.n_sites, d.capacity(), kbar, d.options(), d.unobserved_cells(),
                           d.leaf_evidence_cells(), knobs) == plan
    return d, plan


def run_family(spec):
    model, tree, fp, cap = inputs(spec)
    d, plan = context(spec, model, tree, fp, cap)
    if spec.get("unobserved") or spec.get("evidence"):
        # (leaf states are resampled: the checks of _checked_run that pin them do not apply)
        J, D, nacc = d.run_mcmc(2, 3, 19, sweep_base=4)
        p = d.paths()
        out = dict(paths=_sha(p.init, p.offsets, p.jumps), stats=_sha(J, D), nacc=int(nacc), tri=_sha(d.tri_llh()),
                   overflow=int(d.counters()["overflow"]))
    else:
        out = _checked_run(d, tree, fp, 19)
    assert spec.get("overflows") or d.phase_plan() == plan
    c = d.counters()
    out["giveups"] = int(d.direct_giveups())
    assert out["giveups"] == 0
    d.close()
    return dict(out, plan=plan, coop_tasks=int(c["coop_tasks"]), search_finished=int(c["search_finished"]))


def run_replay(spec):
    model, tree, fp, cap = inputs(spec)
    d, plan = context(spec, model, tree, fp, cap)
    compared = 0
    for colour in spec["colours"]:
        compared += _replay(d, spec, model, tree, cap, colour, 23, 5 + colour, spec["only_changed"])
    n_colour = sum(len([s for s in range(1, fp.n_sites - 1) if s % 3 == c]) for c in spec["colours"])
    if not spec["only_changed"]:
        assert compared == n_colour * (tree.n_nodes - 1), (compared, n_colour)      # no site left out
    assert d.direct_giveups() == 0
    d.close()
    return dict(plan=plan, compared=compared, cap=cap)


def run_unrunnable(spec):
    model, tree, fp, cap = inputs(spec)
    t0 = time.time()
    d, plan = context(spec, model, tree, fp, cap)
    out = _checked_run(d, tree, fp, 19)
    out["seconds"] = time.time() - t0
    # a phase from where the run ended replays from the restatement
    out["compared"] = _replay(d, spec, model, tree, cap, 1, 29, 40, True)
    assert d.direct_giveups() == 0
    d.close()
    return dict(out, plan=plan)


def run_two_contexts(spec):
    from epievo_amd.driver import CppSampler
    model, tree, fp, cap = inputs(spec)
    res = []
    for devices in ([0], [0, 0]):
        s = CppSampler(2, 3, devices=devices, capacity=cap)
        s.set_direct_sampler(True, fused=bool(spec["fused"]))     # before reset: the contexts do not exist yet
        s.reset(model, tree, fp)
        J, D, acc = s.run_mcmc(19, 0)
        p = s.paths()
        res.append(dict(paths=_sha(p.init, p.offsets, p.jumps), stats=_sha(J, D), acc=acc, mode=s.phase_mode()))
        s.close()
    return dict(one=res[0], two=res[1])


def run_group(spec):
    """a LocalGroup of three contexts against a single context, both with the row's switch"""
    from epievo_amd.parallel import LocalGroup
    model, tree, fp, cap = inputs(spec)
    d, plan = context(spec, model, tree, fp, cap)
    J, D, nacc = d.run_mcmc(2, 3, 19, sweep_base=4)
    p = d.paths()
    one = dict(paths=_sha(p.init, p.offsets, p.jumps), stats=_sha(J, D), nacc=int(nacc))
    d.close()
    g = LocalGroup(0, 3, sweeps_per_refresh=10)
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    g.set_direct_sampler(True, fused=bool(spec["fused"]))
    assert len(g.subs) == 3
    for s in g.subs:
        check_plan(s.phase_plan(), spec)
    g.reset()
    J, D, nacc = g.run_mcmc(2, 3, 19, sweep_base=4)
    p = g.paths()
    three = dict(paths=_sha(p.init, p.offsets, p.jumps), stats=_sha(J, D), nacc=int(nacc))
    assert sum(s.direct_giveups() for s in g.subs) == 0
    g.close()
    return dict(one=one, three=three, plan=plan)


if __name__ == "__main__":
    spec = json.loads(sys.argv[1])
    out = {"family": run_family, "replay": run_replay, "unrunnable": run_unrunnable, "two_contexts": run_two_contexts,
           "group": run_group}[spec["kind"]](spec)
    print("ok " + json.dumps(out))
