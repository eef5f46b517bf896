"""The model space: sampler models far from test.param, and above all models that did not generate the data they
sample (test_model_space.py on the CPU, test_model_space_gpu.py on the device).

Every other GPU row draws its histories from the model that then samples them, and from three rate sets in all.
The production loop does the opposite: EM moves the model every iteration, so the sampler always runs under a
model the paths were not drawn from.  The branches of the code that depend on the model:

  the no-jump shortcut goes silent at rate T >= 40           fast, skew, skewm
  exp(-rate T) underflows to 0, bracket trunc == 1.0         skew, and fast on the long branch of pair
  the Nielsen bracket 1 - exp(-rate T) cancels               slow, and test.param with every branch x 1e-6
  matrix table from pairs (r0, r1) many orders apart         ratio, skew, mixed
  logs of rates from 1e-10 to 1e5 in the acceptance          slow ... skew
  a capacity overflow caused by the model, not the input     fast, skewm

Models (the eight rates by context 4 l + 2 m + r):
  ref     test.param: 0.087 .. 10.2
  anti    stationary 0.05 0.05 / baseline -0.5 -0.5, scale=True: 0.21 .. 75.5
  mixed   stationary 0.99 0.6 / baseline 2.0 -6.0, scale=True: 1.7e-4 .. 125 (ratio 7e5)
  slow    test.param x 1e-9: 8.7e-11 .. 1.0e-8
  fast    test.param x 100: 8.7 .. 1020
  skew    stationary 0.999 0.999 / baseline -0.5 -3.0, scale=True: 0.019 .. 2.3e5.  On data of test.param a kept
          segment costs 604 trials on average (4.9e6 trials for 8097 segments at n = 300 on tree), far beyond the
          work bound: it samples only data it generated itself
  skewm   skew toned down to stationary 0.99 0.99: 0.09 .. 2283.  The mismatch rows of skew's shape that meet the work
          bound (at 0.995 star5 costs 92 trials per segment, at 0.99 at most 16.3)
  ratio   test.param x [1e4, 1, 1e-4, 1, 1, 1e4, 1, 1e-4]: 8.7e-6 .. 4.2e4.  Only on its own data, see below

The work bound.  A segment that keeps its state is sampled by forward rejection with no bound on the number of
trials; where leaving the state is fast and returning is slow the success probability is about exp(-rate T) and
the search effectively never ends (ratio sampling data of test.param: tree, n = 300, oracle seed 7, did not finish
in 40 s on the CPU).  The device's scan_trials shares the design, so such an input is a kernel that does not
return.  Therefore: a row goes to the device only if the oracle's run of exactly what the device will run has
trials / segments <= WORK_BOUND.  test_model_space.py asserts it for every (row, options) of gpu_cases(), the GPU
module takes its rows from gpu_cases() only, and each GPU child repeats the check on its own oracle run before it
creates a device context.  UNRUNNABLE names what is recorded and never run.

A row's input is host.simulate(data model, scaled tree, n, SIM_SEED); the capacity is the roomy one of the kernel
matrix, max(16, 2 max + 8).  Each row carries the figures of the CPU oracle run that justified it (rung B,
ORACLE_SEED, run_mcmc(2, 3, sweep_base=4), default options): acceptance, trials per segment, overflow count."""
import numpy as np

from common import _tmp, config, ref_test_model
from epievo_amd import host

MODEL_TEXT = {
    "anti": "stationary\t0.05\t0.05\nbaseline\t-0.5\t-0.5\n",
    "mixed": "stationary\t0.99\t0.6\nbaseline\t2.0\t-6.0\n",
    "skew": "stationary\t0.999\t0.999\nbaseline\t-0.5\t-3.0\n",
    "skewm": "stationary\t0.99\t0.99\nbaseline\t-0.5\t-3.0\n",
}
MODEL_FACTOR = {
    "slow": 1e-9,
    "fast": 100.0,
    "ratio": np.array([1e4, 1, 1e-4, 1, 1, 1e4, 1, 1e-4]),
}
MODELS = ("ref",) + tuple(MODEL_TEXT) + tuple(MODEL_FACTOR)
SIM_SEED, ORACLE_SEED = 5, 7
WORK_BOUND = 64.0
SHORTCUT_CUT, EXP_UNDERFLOW = 40.0, 745.2

# recorded, never run (not on the CPU either: it does not finish): (data model, sampler model, tree, n)
UNRUNNABLE = (("ref", "ratio", "tree", 300),)

_models, _inputs = {}, {}


def model(name):
    if name not in _models:
        ref = ref_test_model()
        if name == "ref":
            _models[name] = ref
        elif name in MODEL_TEXT:
            _models[name] = host.Model.read(_tmp("space_%s.param" % name, MODEL_TEXT[name]), scale=True)
        else:
            _models[name] = host.Model(ref.rates * MODEL_FACTOR[name], ref.T, ref.baseline)
    return _models[name]


def scaled_tree(name, factor):
    """the named tree of workloads.config with every branch multiplied by factor"""
    t = config(name)
    return host.Tree(t.subtree_sizes, t.parent_ids, t.branches * float(factor), t.node_names)


# (id, data model, sampler model, tree, branch factor, n, labels, (acceptance, trials / segment, overflows)).
# Labels are preconditions test_model_space.py computes from the sampler model, the tree and the oracle's run:
#   silent          some context has rate T_b >= 40 on some branch while the input has a mean below 1 jump per path
#   underflow       max rate x max branch > 745.2
#   tiny            max rate x max branch < 1e-6
#   ratio6          max / min rate >= 1e6
#   mismatch        the data model differs from the sampler model
#   model-overflow  the oracle counts overflows at the roomy capacity
#   accept-all      every proposal is accepted (else 0 < accepted < proposals is asserted)
#   fr              also runs with forward_rejection: its oracle run in that mode meets the work bound too
ROWS = [
    # data of test.param under the five other models, each on the trees of every kernel family
    ("anti-pair", "ref", "anti", "pair", 0.1, 300, ("mismatch",), (0.621, 23.30, 0)),
    ("anti-tree", "ref", "anti", "tree", 1, 300, ("mismatch", "fr"), (0.437, 15.60, 0)),             # fr: 19.13
    ("anti-star5", "ref", "anti", "star5", 1, 300, ("mismatch",), (0.162, 19.59, 0)),
    ("anti-cat6", "ref", "anti", "cat6", 1, 300, ("mismatch",), (0.169, 7.58, 0)),
    ("anti-bal16", "ref", "anti", "bal16", 1, 300, ("mismatch", "fr"), (0.177, 3.84, 0)),            # fr: 30.18
    ("anti-bal64", "ref", "anti", "bal64", 1, 130, ("mismatch",), (0.406, 3.72, 0)),
    ("mixed-pair", "ref", "mixed", "pair", 1, 300, ("mismatch", "fr"), (0.792, 1.32, 0)),            # fr: 16.12
    ("mixed-tree", "ref", "mixed", "tree", 1, 300, ("mismatch",), (0.985, 1.03, 0)),     # forward rejection: 216.5, not run
    ("mixed-star5", "ref", "mixed", "star5", 1, 300, ("mismatch",), (0.897, 1.17, 0)),   # forward rejection: 92.5, not run
    ("mixed-bal16", "ref", "mixed", "bal16", 1, 300, ("mismatch",), (0.826, 1.06, 0)),   # forward rejection: 93.7, not run
    ("mixed-bal64", "ref", "mixed", "bal64", 1, 130, ("mismatch",), (0.839, 1.04, 0)),
    ("slow-pair", "ref", "slow", "pair", 1, 300, ("tiny", "mismatch"), (0.897, 1.00, 0)),
    ("slow-tree", "ref", "slow", "tree", 1, 300, ("tiny", "mismatch"), (0.993, 1.00, 0)),
    ("slow-star5", "ref", "slow", "star5", 1, 300, ("tiny", "mismatch"), (0.940, 1.00, 0)),
    ("slow-bal16", "ref", "slow", "bal16", 1, 300, ("tiny", "mismatch"), (0.943, 1.00, 0)),
    ("slow-bal64", "ref", "slow", "bal64", 1, 130, ("tiny", "mismatch"), (0.953, 1.00, 0)),
    # (fast fills the 16 slots within a sweep: on the unscaled star5 and bal16 it accepts 14 and 13 of 894, so
    # their branches are shortened; pair's branch of 1.0 is kept once for the underflow, 2 accepted of 894)
    ("fast-pair", "ref", "fast", "pair", 0.1, 300, ("silent", "mismatch", "model-overflow", "fr"), (0.318, 1.18, 297)),   # fr: 1.60
    ("fast-pair-long", "ref", "fast", "pair", 1, 300, ("underflow", "mismatch", "model-overflow"), (0.002, 0.56, 1304)),
    ("fast-tree", "ref", "fast", "tree", 1, 300, ("silent", "mismatch", "model-overflow", "fr"), (0.201, 1.19, 340)),     # fr: 1.92
    ("fast-star5", "ref", "fast", "star5", 0.3, 300, ("silent", "mismatch", "model-overflow"), (0.153, 1.27, 366)),
    ("fast-bal16", "ref", "fast", "bal16", 0.4, 300, ("mismatch", "model-overflow"), (0.074, 1.34, 11)),
    ("fast-bal64", "ref", "fast", "bal64", 1, 130, ("mismatch", "model-overflow", "fr"), (0.062, 1.33, 16)),              # fr: 1.89
    ("skewm-pair", "ref", "skewm", "pair", 0.1, 300, ("silent", "mismatch"), (0.787, 16.34, 0)),
    ("skewm-pair-long", "ref", "skewm", "pair", 1, 300, ("underflow", "mismatch", "model-overflow"), (0.330, 1.69, 236)),
    ("skewm-tree", "ref", "skewm", "tree", 1, 300, ("silent", "mismatch"), (0.705, 6.36, 0)),
    ("skewm-star5", "ref", "skewm", "star5", 1, 300, ("silent", "mismatch", "model-overflow"), (0.445, 14.14, 17)),
    ("skewm-bal16", "ref", "skewm", "bal16", 1, 300, ("silent", "mismatch"), (0.387, 7.05, 0)),
    ("skewm-bal64", "ref", "skewm", "bal64", 1, 130, ("silent", "mismatch"), (0.401, 5.50, 0)),
    # the two models that sample only data they generated
    ("skew-pair", "skew", "skew", "pair", 1, 200, ("silent", "underflow", "ratio6"), (0.997, 1.00, 0)),
    ("skew-tree", "skew", "skew", "tree", 1, 200, ("silent", "underflow", "ratio6", "accept-all", "fr"), (1.000, 1.00, 0)),   # fr: 1.00
    ("skew-star5", "skew", "skew", "star5", 1, 200, ("silent", "underflow", "ratio6", "accept-all"), (1.000, 1.00, 0)),
    ("skew-bal16", "skew", "skew", "bal16", 1, 200, ("silent", "underflow", "ratio6"), (0.998, 1.00, 0)),
    ("skew-bal64", "skew", "skew", "bal64", 1, 130, ("silent", "underflow", "ratio6"), (0.982, 1.00, 0)),
    ("ratio-pair", "ratio", "ratio", "pair", 1, 200, ("silent", "underflow", "ratio6"), (0.657, 1.14, 0)),
    ("ratio-tree", "ratio", "ratio", "tree", 1, 200, ("silent", "underflow", "ratio6", "fr"), (0.599, 1.08, 0)),           # fr: 1.34
    ("ratio-star5", "ratio", "ratio", "star5", 1, 200, ("silent", "underflow", "ratio6"), (0.407, 1.12, 0)),
    ("ratio-bal16", "ratio", "ratio", "bal16", 1, 200, ("silent", "underflow", "ratio6"), (0.488, 1.02, 0)),
    ("ratio-bal64", "ratio", "ratio", "bal64", 1, 130, ("silent", "underflow", "ratio6"), (0.456, 1.01, 0)),
    # test.param with every branch x 1e-6 and x 100.  On its own data over the long branches test.param accepts
    # nothing (0 of 894; dense_cases.py found the same), so the x 100 row samples data of slow: no jumps at all
    ("ref-tree-x1e-6", "ref", "ref", "tree", 1e-6, 300, ("accept-all",), (1.000, 1.00, 0)),
    ("ref-bal16-x1e-6", "ref", "ref", "bal16", 1e-6, 300, ("tiny", "accept-all"), (1.000, 1.00, 0)),
    ("ref-tree-x100", "slow", "ref", "tree", 100, 300, ("silent", "mismatch", "model-overflow"), (0.220, 1.26, 264)),
    # the mismatch the other way
    ("antiref-tree", "anti", "ref", "tree", 1, 300, ("mismatch", "fr"), (0.980, 1.43, 0)),            # fr: 1.60
    ("antiref-cat6", "anti", "ref", "cat6", 1, 300, ("mismatch",), (0.776, 2.05, 0)),
]

LABELS = ("silent", "underflow", "tiny", "ratio6", "mismatch", "model-overflow", "accept-all", "fr")


def row(rid):
    for r in ROWS:
        if r[0] == rid:
            return r
    raise KeyError(rid)


def workload(rid):
    """-> (sampler model, tree, paths, roomy capacity): built once per process and shared, never modified"""
    if rid not in _inputs:
        _, dm, sm, t, factor, n, _, _ = row(rid)
        tree = scaled_tree(t, factor)
        fp = host.simulate(model(dm), tree, n, SIM_SEED)
        _inputs[rid] = (model(sm), tree, fp, int(max(16, 2 * fp.counts().max() + 8)))
    return _inputs[rid]


def oracle(rid, opts=None, cap=None, seed=ORACLE_SEED):
    """rung B on the row in the mode of the options (the keywords of DeviceSampler.set_options), reset"""
    import orc
    opts = opts or {}
    mod, tree, fp, roomy = workload(rid)
    o = orc.Oracle(tree, mod, fp, "B", cap=roomy if cap is None else cap, seed=seed)
    o.set_sampler(bool(opts.get("forward_rejection")))
    o.set_proposal_mode(bool(opts.get("reference_proposal_ratio")))
    o.reset()
    return o


def computed_labels(rid):
    """the labels that follow from the models and the tree alone, in numpy"""
    _, dm, sm, _, _, _, _, _ = row(rid)
    mod, tree, fp, _ = workload(rid)
    x = mod.rates[:, None] * tree.branches[None, 1:]
    out = set()
    if x.max() >= SHORTCUT_CUT and fp.counts().mean() < 1.0:
        out.add("silent")
    if mod.rates.max() * tree.branches.max() > EXP_UNDERFLOW:
        out.add("underflow")
    if mod.rates.max() * tree.branches.max() < 1e-6:
        out.add("tiny")
    if mod.rates.max() / mod.rates.min() >= 1e6:
        out.add("ratio6")
    if dm != sm:
        out.add("mismatch")
    return out


def work(counters):
    """trials per segment of an oracle's counters()"""
    return counters["trials"] / float(max(1, counters["segments"]))


# ---- which kernels a row runs on: the plan helpers and knobs of test_kernel_matrix.py
FR, REF = {"forward_rejection": True}, {"reference_proposal_ratio": True}


def families(tree):
    """(family, environment, expected plan fields) of every kernel family a row on this tree runs"""
    from test_kernel_matrix import _SEP, fused, v1, v2, v3
    return {
        "pair": [("fused2", {}, fused(2))],
        "tree": [("fused5", {}, fused(5)),
                 ("v2-jumps", dict(_SEP, EPV_SEG_JUMPS="0"), v2(False, "jumps_all")),
                 ("v2-seg", dict(_SEP, EPV_SEG_JUMPS="1"), v2(False, "segments")),
                 ("v1-global", dict(_SEP, EPV_PROPOSE_V1="1", EPV_FORCE_GLOBAL_POOL="1"),
                  v1(True, False, "jumps_all", "accept_cache"))],
        "star5": [("fused-generic", {}, fused(0))],
        "cat6": [("fused-generic", {"EPV_FUSED_PHASE": "1", "EPV_FORCE_LDS_POOL": "1"}, fused(0))],
        "bal16": [("v3-one-word", dict(_SEP, EPV_PROPOSE_V3="1"), v3(1, False, "jumps_all"))],
        "bal64": [("v3-two-words", dict(_SEP, EPV_PROPOSE_V3="1"), v3(2, False, "jumps_all"))],
    }[tree]


FAMILIES = ("fused2", "fused5", "fused-generic", "v2-jumps", "v2-seg", "v3-one-word", "v3-two-words", "v1-global")


def gpu_cases():
    """(case id, row id, environment, expected plan fields of the default options, the option sets the case runs).
    Every row runs the default options on every family of its tree; on the first of them it then runs once with
    reference_proposal_ratio and, if labelled fr, once with forward_rejection (new contexts, same knobs).
    ratio's own data has 0.28 (tree) and 0.60 (star5) jumps per path, and a context sizes its LDS record pool from
    that mean: without a knob those rows leave the fused phase and the segment lists for the large-tree kernel, so
    they set EPV_FORCE_LDS_POOL, as the fused cat6 row of test_kernel_matrix.py does for the same reason."""
    out = []
    for r in ROWS:
        for i, (fam, env, expect) in enumerate(families(r[3])):
            if r[2] == "ratio" and fam in ("fused2", "fused5", "fused-generic", "v2-seg"):
                env = dict(env, EPV_FORCE_LDS_POOL="1")
            modes = [{}]
            if i == 0:
                modes.append(REF)
                if "fr" in r[6]:
                    modes.append(FR)
            out.append(("%s-%s" % (r[0], fam), r[0], env, expect, modes))
    return out


def row_modes(rid):
    """every option set under which the row reaches the device"""
    modes = []
    for c in gpu_cases():
        if c[1] == rid:
            modes += [m for m in c[4] if m not in modes]
    return modes
