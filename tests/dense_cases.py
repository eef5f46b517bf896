"""Dense histories: inputs on which a (site, branch) path has tens of jumps, for the tests of the code that
only such paths reach (test_dense_histories.py on the CPU, test_dense_histories_gpu.py on the device).

The reference's test.param is no use here: on dense histories its acceptance rate is zero (measured: tree x 150,
star5 x 40, bal16 x 100, each 0 accepted of about 600), and a rejected proposal's jump times are never read back,
so a comparison would compare nothing.  Two models do work:

  weak   stationary 0.55 0.6 / baseline -0.1 -0.2, read with scale=True like the fuzz test's models: rates
         0.67 .. 1.33, acceptance 0.05 .. 0.75 on the workloads below
  flat   stationary 0.5 0.5 / baseline 0 0: all eight rates exactly 1, every interior proposal is accepted, so
         every proposed jump time lands in the compared paths

A workload is a named tree of epievo_amd.workloads.config with every branch multiplied by a factor, a model and a
genome length; its input is host.simulate(model, tree, n, SIM_SEED).  The module also holds a yardstick for the
sufficient statistics J and D that walks a FlatPaths in plain Python and shares no code with oracle/ or the
device's three-way merge."""
import math

import numpy as np

from common import _tmp, config
from epievo_amd import host

MODEL_TEXT = {
    "weak": "stationary\t0.55\t0.6\nbaseline\t-0.1\t-0.2\n",
    "flat": "stationary\t0.5\t0.5\nbaseline\t0\t0\n",
}
SIM_SEED, ORACLE_SEED = 77, 41


def model(name):
    return host.Model.read(_tmp("dense_%s.param" % name, MODEL_TEXT[name]), scale=True)


def scaled_tree(name, factor):
    """the named tree of workloads.config with every branch multiplied by factor"""
    t = config(name)
    return host.Tree(t.subtree_sizes, t.parent_ids, t.branches * float(factor), t.node_names)


# name -> (model, tree, factor, n, labels).  Labels are the preconditions test_dense_histories.py asserts on the
# generated input:
#   fused   run at C = 31 (the fused phase's largest capacity), mean >= 2 jumps per path
#   w2      at cap = max(16, 2 max + 8): 2 C + 1 > 64, two or more words of proposal states
#   over64  share of interior (branch, site) with K = nj[s-1] + nj[s+1] + 1 > 64 at least 0.03
#   both    over64, and the share with K <= 64 is at least 0.03 too: both list routes in one launch
WORKLOADS = {
    "weak-pair4": ("weak", "pair", 4, 600, ("fused",)),
    "weak-cherry12": ("weak", "cherry", 12, 600, ("fused",)),
    "weak-star3x15": ("weak", "star3", 15, 600, ("fused",)),
    "weak-tree40": ("weak", "tree", 40, 600, ("fused",)),
    "weak-star5x20": ("weak", "star5", 20, 600, ("fused",)),
    "weak-cat6x25": ("weak", "cat6", 25, 600, ("fused",)),
    "weak-tree150": ("weak", "tree", 150, 400, ("w2",)),
    "weak-pair25": ("weak", "pair", 25, 400, ("w2", "over64", "both")),
    "weak-pair40": ("weak", "pair", 40, 400, ("w2", "over64", "both")),
    "weak-tree300": ("weak", "tree", 300, 400, ("w2", "over64", "both")),
    "weak-cat6x150": ("weak", "cat6", 150, 300, ("w2", "over64", "both")),
    "weak-multi30": ("weak", "multi", 30, 300, ("w2",)),
    "weak-bal8x100": ("weak", "bal8", 100, 300, ("w2",)),
    "weak-bal16x60": ("weak", "bal16", 60, 300, ()),
    "flat-tree300": ("flat", "tree", 300, 400, ("w2", "over64", "both")),
    "flat-bal16x300": ("flat", "bal16", 300, 200, ("w2",)),
    "flat-bal32x400": ("flat", "bal32", 400, 130, ("w2",)),
    "flat-bal64x500": ("flat", "bal64", 500, 130, ("w2",)),
    # the longer chains of the statistical comparison and the inputs of the linked-reference goldens
    "weak-pair10": ("weak", "pair", 10, 4000, ()),
    "weak-tree100": ("weak", "tree", 100, 3000, ()),
}
# name -> (workload, first and last site of the window that stays dense).  Outside the window thin() leaves at
# most one jump per path, so the mean jump count -- from which a context sizes its LDS record pool when the
# paths are uploaded -- stays small enough for the second proposal kernel and the fused phase, which the
# homogeneous inputs above are too dense for; inside it the paths are as dense as ever, and after one sweep
# of proposals drawn over the long branches so is every site.
MIXED = {
    "mixed-pair40": ("weak-pair40", 100, 159),
    "mixed-pair25": ("weak-pair25", 100, 199),
    "mixed-tree300": ("weak-tree300", 100, 139),
    "mixed-star5x20": ("weak-star5x20", 200, 349),
    "mixed-tree150": ("weak-tree150", 100, 179),
    "mixed-tree40": ("weak-tree40", 200, 349),
}
# workloads that also run at a capacity equal to the input's own largest jump count: proposals overflow
OVERFLOW = ("weak-tree40", "weak-tree150", "weak-pair40", "mixed-tree150", "mixed-pair40")
FUSED_CAP = 31

_inputs = {}


def thin(fp, lo, hi):
    """the paths with, outside the sites lo .. hi, only the first (count mod 2) jumps of every path kept: the
    end states, and so the leaf data, are unchanged"""
    cnt = fp.counts()
    site = np.tile(np.arange(fp.n_sites), fp.n_nodes - 1)
    keep = np.where((site >= lo) & (site <= hi), cnt, cnt & 1)
    off = np.zeros(len(cnt) + 1, np.uint64)
    off[1:] = np.cumsum(keep)
    pieces = [fp.jumps[int(a):int(a) + int(k)] for a, k in zip(fp.offsets[:-1], keep) if k]
    return host.FlatPaths(fp.n_sites, fp.n_nodes, fp.init, off, np.concatenate(pieces))


def base(name):
    return MIXED[name][0] if name in MIXED else name


def workload(name, n=None):
    """-> (model, tree, paths): built once per process and shared, never modified"""
    key = (name, n)
    if name in MIXED:
        if key not in _inputs:
            mod, tree, fp = workload(MIXED[name][0], n)
            _inputs[key] = (mod, tree, thin(fp, *MIXED[name][1:]))
        return _inputs[key]
    if key not in _inputs:
        m, t, factor, n0, _ = WORKLOADS[name]
        mod, tree = model(m), scaled_tree(t, factor)
        _inputs[key] = (mod, tree, host.simulate(mod, tree, n0 if n is None else n, SIM_SEED))
    return _inputs[key]


def capacity(name, fp, kind="roomy"):
    """roomy: max(16, 2 max + 8), or 31 for a workload labelled fused; tight: the input's own maximum"""
    if kind == "tight":
        return int(fp.counts().max())
    if "fused" in WORKLOADS[base(name)][4]:
        return FUSED_CAP
    return int(max(16, 2 * fp.counts().max() + 8))


def words(cap):
    """64-bit words of proposal states per (site, branch): W = ceil((2 C + 1) / 64)"""
    return (2 * cap + 1 + 63) // 64


def density(fp):
    """mean and max jumps per (branch, site), and over the interior sites K = nj[s-1] + nj[s+1] + 1: its
    maximum and the shares of K > 64 and of K == 1"""
    B, n = fp.n_nodes - 1, fp.n_sites
    nj = fp.counts().reshape(B, n)
    K = nj[:, :-2] + nj[:, 2:] + 1
    return dict(mean=float(nj.mean()), max=int(nj.max()), kmax=int(K.max()), over64=float((K > 64).mean()),
                k1=float((K == 1).mean()))


def yardstick(fp, branches, first=1, last=None):
    """J and D of the interior sites first .. last by walking the paths.

    For every branch and site the jumps of the site and its two neighbours become one list of (time, whose)
    and are sorted; between two events the triple (left, middle, right) of states is a context 4 l + 2 m + r
    that the interval's length is spent in, and a jump of the middle site counts once in the context it
    leaves.  Events at exactly the same time are taken right, middle, left -- the reference's tie rule
    (Path.cpp:206-301); the interval between them is empty, so D does not depend on it.

    Every interval enters as the two terms +end and -start and a cell's terms are added with math.fsum, whose
    result is the correctly rounded exact sum: the yardstick's own error is half an ulp of the cell.

    -> (J int64 [B, 8], D float64 [B, 8], the number of intervals summed into each cell int64 [B, 8])"""
    B, n = fp.n_nodes - 1, fp.n_sites
    last = n - 2 if last is None else last
    off = [int(x) for x in fp.offsets]
    jumps = fp.jumps.tolist()
    init = [int(x) for x in fp.init]
    J = np.zeros((B, 8), np.int64)
    n_int = np.zeros((B, 8), np.int64)
    D = np.zeros((B, 8))
    for b in range(B):
        T = float(branches[b + 1])
        terms = [[] for _ in range(8)]
        for s in range(first, last + 1):
            events = []
            for rank, bit, site in ((0, 1, s + 1), (1, 2, s), (2, 4, s - 1)):
                e = b * n + site
                events.extend((t, rank, bit) for t in jumps[off[e]:off[e + 1]])
            events.sort()
            ctx = 4 * init[b * n + s - 1] + 2 * init[b * n + s] + init[b * n + s + 1]
            prev = 0.0
            for t, _, bit in events:
                terms[ctx].append(t)
                terms[ctx].append(-prev)
                n_int[b, ctx] += 1
                if bit == 2:
                    J[b, ctx] += 1
                ctx ^= bit
                prev = t
            terms[ctx].append(T)
            terms[ctx].append(-prev)
            n_int[b, ctx] += 1
        for c in range(8):
            D[b, c] = math.fsum(terms[c])
    return J, D, n_int


def dwell_bound(n_int, D, scales):
    """how far a fixed-point D cell may lie from the exact one.  The parallel rung and the device add, per
    interval, q = rint(fl(t - prev) * 2^k_b) as integers and convert the total once:
      * rint moves an interval by at most half a quantum 2^-k_b, so a cell of m intervals by m / 2 quanta;
      * fl(t - prev) is one fp64 subtraction, relative error 2^-53 of the interval, in total 2^-53 of the cell;
        the product with the power of two is exact;
      * int64 -> double rounds once (2^-53 relative), and so does the yardstick's fsum.
    The relative terms add up to 3 * 2^-53 < 1e-15; they are covered by the 1e-12 that test_exact_stats.py
    already allows between the integer and the fp64 sums.
    scales: 2^k_b per node as orc_stat_scales gives them (index 0 unused) -> float64 [B, 8]"""
    return n_int * (0.5 / np.asarray(scales)[1:, None]) + 1e-12 * np.abs(D)


def stat_scales(o):
    """2^k_b of every node from an Oracle (index 0 unused)"""
    import ctypes as C
    s = np.zeros(o.B + 1)
    o.L.orc_stat_scales(o.h, s.ctypes.data_as(C.POINTER(C.c_double)))
    return s


def oracle(name, cap, opts=None, seed=ORACLE_SEED, n=None):
    """rung B on the workload, in the mode of the options (the keywords of DeviceSampler.set_options), reset"""
    import orc
    opts = opts or {}
    mod, tree, fp = workload(name, n)
    o = orc.Oracle(tree, mod, fp, "B", cap=cap, seed=seed)
    o.set_sampler(bool(opts.get("forward_rejection")))
    o.set_proposal_mode(bool(opts.get("reference_proposal_ratio")))
    o.set_sample_root(bool(opts.get("sample_root")))
    o.reset()
    return o
