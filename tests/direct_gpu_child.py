"""One GPU run of tests/test_direct_sampler_gpu.py in a process of its own (a context reads its EPV_* knobs when it
is created, and the unrunnable row runs under a time limit): python direct_gpu_child.py '<json spec>'.  Prints one
line "ok <json>" with what the parent compares."""
import hashlib
import json
import os
import sys
import time

import numpy as np

_TESTS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_TESTS))
sys.path.insert(0, _TESTS)

from epievo_amd import host                         # noqa: E402
from epievo_amd.sampler import DeviceSampler       # noqa: E402


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _leaf_states(tree, fp):
    B, n = fp.n_nodes - 1, fp.n_sites
    end = (fp.init ^ (fp.counts() & 1).astype(np.uint8)).reshape(B, n)
    return end[np.asarray(tree.subtree_sizes)[1:] == 1]


def _inputs(spec):
    """model, tree, paths, capacity"""
    if spec["input"] == "dense":
        import dense_cases as dc
        mod, tree, fp = dc.workload(spec["workload"], spec.get("n"))
        return mod, tree, fp, int(max(16, 2 * fp.counts().max() + 8))
    if spec["input"] == "model_space":           # (data model, sampler model, tree, n) as model_cases.UNRUNNABLE names it
        import model_cases as mc
        dm, sm, t, n = spec["row"]
        tree = mc.scaled_tree(t, 1)
        fp = host.simulate(mc.model(dm), tree, n, mc.SIM_SEED)
        return mc.model(sm), tree, fp, int(max(16, 2 * fp.counts().max() + 8))
    if spec["input"] == "row":                   # a row of model_cases.ROWS by its id
        import model_cases as mc
        return mc.workload(spec["rid"])
    from common import ref_test_model
    from test_kernel_matrix import make_tree
    model, tree = ref_test_model(), make_tree(spec["tree"])
    fp = host.simulate(model, tree, spec["n"], 6)
    return model, tree, fp, int(max(16, 2 * fp.counts().max() + 8))


def _set_options(d, opts):
    """the keywords of set_options, and direct_sampler through its own call behind it"""
    opts = dict(opts)
    direct = opts.pop("direct_sampler", False)
    d.set_options(**opts)
    if direct:
        d.set_direct_sampler(True)


def _context(spec, model, tree, fp, cap):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    _set_options(d, spec["opts"])
    d.reset()
    plan = d.phase_plan()
    bad = dict((k, (v, plan[k])) for k, v in spec["expect"].items() if plan[k] != v)
    assert not bad, "plan differs (expected, got): %r; plan %r" % (bad, plan)
    return d, plan


def _replay(d, spec, model, tree, cap, colour, seed, sweep, only_changed):
    from direct_ref import replay_phase
    before = d.paths()
    d.sweep_phase(colour, seed, sweep)
    after = d.paths()
    compared, bad, longest = replay_phase(seed, sweep, colour, model.rates, tree.branches, before, after, cap, only_changed)
    assert not bad, "paths differ from the restatement at (site, branch) %r ... (%d of %d)" % (bad[:8], len(bad), compared)
    assert longest <= 20, longest
    return compared


def run_replay(spec):
    model, tree, fp, cap = _inputs(spec)
    d, plan = _context(spec, model, tree, fp, cap)
    compared = 0
    for colour in spec["colours"]:
        compared += _replay(d, spec, model, tree, cap, colour, 23, 5 + colour, spec["only_changed"])
    n_colour = sum(len([s for s in range(1, fp.n_sites - 1) if s % 3 == c]) for c in spec["colours"])
    if not spec["only_changed"]:
        assert compared == n_colour * (tree.n_nodes - 1), (compared, n_colour)      # no site left out
    assert d.direct_giveups() == 0
    d.close()
    return dict(plan=plan, compared=compared)


def _checked_run(d, tree, fp, seed):
    """run_mcmc(2, 3) and what every direct run must satisfy -> digest"""
    J, D, nacc = d.run_mcmc(2, 3, seed, sweep_base=4)
    after = d.paths()
    tri = d.tri_llh().copy()
    d.reset()
    assert np.array_equal(tri.view(np.uint64), d.tri_llh().view(np.uint64)), "tri_llh cache differs from a fresh reset()"
    B = tree.n_nodes - 1
    want = (fp.n_sites - 2) * np.asarray(tree.branches)[1:]
    got = np.asarray(D).reshape(B, 8).sum(axis=1)
    assert np.all(np.abs(got - want) <= 1e-9 * want), (got, want)                # time is conserved on every branch
    assert np.array_equal(_leaf_states(tree, fp), _leaf_states(tree, after)), "a leaf state changed"
    assert d.direct_giveups() == 0
    assert 0 < nacc
    return dict(paths=_sha(after.init, after.offsets, after.jumps), stats=_sha(J, D), nacc=int(nacc), tri=_sha(tri),
                overflow=int(d.counters()["overflow"]))


def run_family(spec):
    model, tree, fp, cap = _inputs(spec)
    d, plan = _context(spec, model, tree, fp, cap)
    out = _checked_run(d, tree, fp, 19)
    assert d.phase_plan() == plan
    d.close()
    return dict(out, plan=plan)


def run_unrunnable(spec):
    model, tree, fp, cap = _inputs(spec)
    t0 = time.time()
    d, plan = _context(spec, model, tree, fp, cap)
    out = _checked_run(d, tree, fp, 19)
    out["seconds"] = time.time() - t0
    # a phase from where the run ended replays from the restatement
    out["compared"] = _replay(d, spec, model, tree, cap, 1, 29, 40, True)
    assert d.direct_giveups() == 0
    d.close()
    return dict(out, plan=plan)


def run_two_contexts(spec):
    from epievo_amd.driver import CppSampler
    model, tree, fp, cap = _inputs(spec)
    res = []
    for devices in ([0], [0, 0]):
        s = CppSampler(2, 3, devices=devices, capacity=cap)
        _set_options(s, spec["opts"])                       # before reset: the contexts do not exist yet
        s.reset(model, tree, fp)
        J, D, acc = s.run_mcmc(19, 0)
        p = s.paths()
        res.append(dict(paths=_sha(p.init, p.offsets, p.jumps), stats=_sha(J, D), acc=acc, layout=s.layout()["text"]))
        s.close()
    return dict(one=res[0], two=res[1])


if __name__ == "__main__":
    spec = json.loads(sys.argv[1])
    out = {"replay": run_replay, "family": run_family, "unrunnable": run_unrunnable,
           "two_contexts": run_two_contexts}[spec["kind"]](spec)
    print("ok " + json.dumps(out))
