"""Every instantiation of the first proposal kernel's LEAF axis (epv_mh_propose_kernel<GPOOL, REFQ, LEAF>,
LEAF = EPV_LEAF_MASK or EPV_LEAF_EVIDENCE) against the oracle's rung B, bit for bit, in the style of
test_kernel_matrix.py.

The oracle takes the mask and the table itself (orc_set_unobserved, orc_set_leaf_evidence; its own law is
checked without a GPU in test_leaf_oracle.py), so a row checks what a SOFT leaf cell does, not an identity
of the new code with itself.  Each row asserts the plan after reset(), runs run_mcmc(2, 3, seed, sweep_base=4)
on both sides and compares J, D, the accept count, the paths, the cached triple likelihoods as uint64 and
the overflow counter.  Rows that need an EPV_* knob run in a fresh process with the knob in the environment.

Leaf content of a row (leaf_content): about 15 % of the leaf cells masked, about 15 % with evidence, a few
with both (the evidence wins), the rest data.  The evidence is a random float32 in (0, 1) and, on every leaf,
each of SPECIAL.  Masked and evidence cells sit at the local sites around the mask's word boundaries
(EDGE_SITES; n is no multiple of 32, so the last word of a bit row is partial) and at the genome's two end
sites, where they must have no effect.

Further tests: one genome cut by hand into two contexts with halos, the life cycle under a held table, and a
hard cell that contradicts the resident path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
from common import config, ref_test_model
from epievo_amd import host
from test_unobserved_leaves import leaf_ends

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))

NAN = np.float32(np.nan)
SUBNORMAL = np.float32(2.0 ** -149)            # the smallest float32 subnormal
# evidence values every leaf of a row carries; "data0" / "data1": r = 0 / 1 at a cell whose data agrees
SPECIAL = ["data0", "data1", np.float32(0.5), np.float32(-0.0), SUBNORMAL, np.float32(2.0 ** -24),
           np.float32(1.0 - 2.0 ** -24), np.float32(0.02), np.float32(0.8)]


def edge_sites(n):
    """around the first two word boundaries of a bit row, the last full boundary, the last interior site
    and the two end sites"""
    return [1, 31, 32, 33, 63, 64, 65, n - 34, n - 33, n - 2, 0, n - 1]


def make_tree(name):
    return host.Tree.single_branch(20.0) if name == "long" else config(name)


def leaf_nodes(tree):
    return [b for b in range(1, tree.n_nodes) if tree.subtree_sizes[b] == 1]


def leaf_content(tree, fp, kind, seed):
    """-> (mask [N-1, n] uint8 or None, r [N-1, n] float32 or None); kind: "mask", "ev" (evidence and mask)
    or "all" (evidence on every leaf cell: the tiny genomes)"""
    rng = np.random.default_rng(seed)
    n, B = fp.n_sites, tree.n_nodes - 1
    ends = leaf_ends(tree, fp)[1:]
    mask = np.zeros((B, n), np.uint8)
    r = np.full((B, n), NAN, np.float32)
    rand = lambda k: (2.0 ** -20 + (1.0 - 2.0 ** -19) * rng.random(k)).astype(np.float32)   # inside (0, 1)

    def special(b, s, v):
        if isinstance(v, str):
            return np.float32(ends[b, s])                   # 0 or 1, agreeing with the data
        if v == 0.0 and ends[b, s] != 0:                    # -0.0f is a hard 0: only where the data agree
            return np.float32(0.5)
        return v

    for o, node in enumerate(leaf_nodes(tree)):
        b = node - 1
        if kind == "all":
            order = [None, np.float32(0.5), np.float32(0.8)] + SPECIAL[3:] + SPECIAL[:2]
            for s in range(n):
                v = order[(s + 2 + 3 * o) % len(order)]
                r[b, s] = rand(1)[0] if v is None else special(b, s, v)
            continue
        m = rng.random(n) < 0.15
        e = (rng.random(n) < 0.15) & ~m
        edge = edge_sites(n)
        for i, s in enumerate(edge):                        # mask, evidence, both, in turn; shifted per leaf
            k = (i + o) % 3
            m[s], e[s] = k != 1, k != 0
        mask[b] = m
        r[b, e] = rand(int(e.sum()))
        free = np.flatnonzero(~m & ~e)
        free = free[(free > 0) & (free < n - 1)]
        rng.shuffle(free)
        zeros, ones = [s for s in free if ends[b, s] == 0], [s for s in free if ends[b, s] == 1]
        assert len(zeros) >= 2 and len(ones) >= 1, "leaf data too uniform for the special values"
        take = iter([s for s in free if s not in (zeros[0], zeros[1], ones[0])])
        for v in SPECIAL:
            if isinstance(v, str):
                s = zeros[0] if v == "data0" else ones[0]
            else:
                s = zeros[1] if v == 0.0 else next(take)
            r[b, s] = special(b, s, v)
    if kind == "mask":
        return mask, None
    if kind == "all":
        return None, r
    return mask, r


def soft_cells(tree, mask, r):
    """[N-1, n] bool: leaf cells whose end state the chain may change (interior sites only)"""
    B = tree.n_nodes - 1
    n = (mask if mask is not None else r).shape[1]
    rr = r if r is not None else np.full((B, n), NAN, np.float32)
    mm = mask if mask is not None else np.zeros((B, n), np.uint8)
    soft = np.where(np.isnan(rr), mm != 0, (rr > 0) & (rr < 1))
    soft[:, [0, -1]] = False
    return soft


def hard_cells(tree, mask, r):
    """[N-1, n] bool: leaf cells pinned to their state: data, and r exactly 0 (or -0) or 1"""
    B = tree.n_nodes - 1
    n = (mask if mask is not None else r).shape[1]
    rr = r if r is not None else np.full((B, n), NAN, np.float32)
    mm = mask if mask is not None else np.zeros((B, n), np.uint8)
    hard = np.where(np.isnan(rr), mm == 0, (rr == 0) | (rr == 1))
    rows = np.zeros(B, bool)
    rows[[b - 1 for b in leaf_nodes(tree)]] = True
    return hard & rows[:, None]


# ---- the rows
FR, REF, SR = {"forward_rejection": True}, {"reference_proposal_ratio": True}, {"sample_root": True}
FRREF = {"forward_rejection": True, "reference_proposal_ratio": True}


def _row(id, tree, n, content, opts, gpool, accept, env=None, mode="mcmc", seed=19):
    refq = bool(opts.get("reference_proposal_ratio") or opts.get("sample_root"))
    expect = dict(propose="V1", gpool=gpool, refq=refq, unobs=content != "all", evidence=content != "mask",
                  jumps="jumps" if opts.get("forward_rejection") else "jumps_all", accept=accept)
    return dict(id=id, tree=tree, n=n, content=content, opts=opts, env=env or {}, expect=expect, mode=mode, seed=seed)


CACHE, A3 = "accept_cache", "accept3"
ROWS = [
    # tree.nwk: the record pool in LDS
    _row("mask-lds", "tree", 1999, "mask", {}, False, CACHE),
    _row("ev-lds", "tree", 1999, "ev", {}, False, CACHE),
    _row("mask-lds-ref", "tree", 1999, "mask", REF, False, CACHE),
    _row("ev-lds-ref", "tree", 1999, "ev", REF, False, CACHE),
    _row("mask-lds-fr", "tree", 1999, "mask", FR, False, CACHE),
    _row("ev-lds-fr", "tree", 1999, "ev", FR, False, CACHE),
    _row("ev-lds-frref", "tree", 1999, "ev", FRREF, False, CACHE),
    _row("mask-lds-sr", "tree", 1999, "mask", SR, False, CACHE),
    _row("ev-lds-sr", "tree", 1999, "ev", SR, False, CACHE),
    _row("ev-lds-forced-global", "tree", 1999, "ev", {}, True, CACHE, env={"EPV_FORCE_GLOBAL_POOL": "1"}),
    # (without its meta cache the plan takes accept3 unless EPV_ACCEPT_V3=0 keeps the first accept kernel)
    _row("ev-no-cache", "tree", 1999, "ev", {}, False, "accept_no_cache",
         env={"EPV_ACCEPT_NO_CACHE": "1", "EPV_ACCEPT_V3": "0"}),
    # the 16-leaf tree: the pool in global memory, the accept stage over all sites
    _row("mask-g", "bal16", 599, "mask", {}, True, A3),
    _row("ev-g", "bal16", 599, "ev", {}, True, A3),
    _row("mask-g-ref", "bal16", 599, "mask", REF, True, A3),
    _row("ev-g-ref", "bal16", 599, "ev", REF, True, A3),
    _row("ev-g-fr", "bal16", 599, "ev", FR, True, A3),
    _row("ev-g-sr", "bal16", 599, "ev", SR, True, A3),
    # a node with three children; leaves at every depth
    _row("ev-multi", "multi", 1501, "ev", {}, True, CACHE),
    _row("ev-cat6", "cat6", 1501, "ev", {}, True, A3),
    # the leaf is the root's child; under SAMPLE_ROOT both ends of the branch are free
    _row("ev-pair", "pair", 1501, "ev", {}, False, CACHE),
    _row("ev-pair-sr", "pair", 1501, "ev", SR, False, CACHE),
    # one long branch (tens of jumps per path), the library's default capacity.  Few updates are accepted at
    # T = 20 (about 3 of 1194 in the five sweeps): the seed is one under which an accepted one flips a soft cell
    _row("ev-long", "long", 400, "ev", {}, True, CACHE, seed=35),
    # a capacity that overflows: two single sweeps (the seed: proposals overflow in both, 1 and 2 more)
    _row("ev-overflow", "tree", 1999, "ev", {}, False, CACHE, mode="overflow", seed=31),
    # the genome-end special cases: evidence on every leaf cell
    _row("ev-tiny-tree3", "tree", 3, "all", {}, False, CACHE),
    _row("ev-tiny-tree4", "tree", 4, "all", {}, False, CACHE),
    _row("ev-tiny-tree5", "tree", 5, "all", {}, False, CACHE),
    _row("ev-tiny-pair6", "pair", 6, "all", {}, False, CACHE),
]
ROW = {r["id"]: r for r in ROWS}
# (the seeds: the oracle leg of every row moves a soft cell under its seed, test_row_content_and_oracle_leg)
SEED = 19           # of the tests below the table


def make_case(row):
    model, tree = ref_test_model(), make_tree(row["tree"])
    fp = host.simulate(model, tree, row["n"], 6)
    mask, r = leaf_content(tree, fp, row["content"], 7)
    cap = int(fp.counts().max()) if row["mode"] == "overflow" else int(max(16, 2 * fp.counts().max() + 8))
    return model, tree, fp, mask, r, cap


def make_oracle(row, case, seed=None, cap=None):
    model, tree, fp, mask, r, cap0 = case
    o = orc.Oracle(tree, model, fp, "B", cap=cap or cap0, seed=row["seed"] if seed is None else seed)
    apply_options(o, row["opts"])
    o.set_unobserved(mask)
    o.set_leaf_evidence(r)
    o.reset()
    return o


def apply_options(o, opts):
    o.set_sampler(bool(opts.get("forward_rejection")))
    o.set_proposal_mode(bool(opts.get("reference_proposal_ratio")))
    o.set_sample_root(bool(opts.get("sample_root")))


def make_device(row, case, cap=None):
    from epievo_amd.sampler import DeviceSampler
    model, tree, fp, mask, r, cap0 = case
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap or cap0)
    d.set_options(**row["opts"])
    d.set_unobserved(mask)
    d.set_leaf_evidence(r)
    d.reset()
    return d


def oracle_leg(row, case):
    """the oracle's side of a row -> (J, D, accepts, paths, tri_llh, overflow count)"""
    o = make_oracle(row, case)
    if row["mode"] == "overflow":
        snaps = []
        for w in range(2):
            o.sweep(w)
            snaps.append(o.paths())
        return None, None, None, snaps, o.tri_llh(), o.counters()["overflow"]
    J, D, nacc, _ = o.run_mcmc(2, 3, sweep_base=4)
    return J, D, nacc, o.paths(), o.tri_llh(), o.counters()["overflow"]


def check_leaf_states(row, case, paths):
    """what holds on either side: pinned cells and the end sites keep their state -> soft cells that moved"""
    model, tree, fp, mask, r, cap = case
    before, after = leaf_ends(tree, fp)[1:], leaf_ends(tree, paths)[1:]
    hard = hard_cells(tree, mask, r)
    assert np.array_equal(after[hard], before[hard]), row["id"]
    assert np.array_equal(after[:, [0, -1]], before[:, [0, -1]]), row["id"]
    return int(((after != before) & soft_cells(tree, mask, r)).sum())


def run_row(row):
    """the GPU against the oracle (needs a GPU; called in-process, or in a child for the rows with knobs)"""
    case = make_case(row)
    d = make_device(row, case)
    plan = d.phase_plan()
    bad = dict((k, (v, plan[k])) for k, v in row["expect"].items() if plan[k] != v)
    assert not bad, "plan differs (expected, got): %r; plan %r" % (bad, plan)
    assert (plan["word"] >> 17 & 1, plan["word"] >> 18 & 1) == (row["expect"]["unobs"], row["expect"]["evidence"])
    assert d.phase_mode() == 0
    Jo, Do, no, po, to, ovo = oracle_leg(row, case)
    if row["mode"] == "overflow":
        for w in range(2):
            try:
                d.sweep(1, row["seed"], sweep_base=w)
            except Exception as e:
                assert "rejected" in str(e) or "capacity" in str(e).lower(), e
            assert orc.paths_equal(d.paths(), po[w]), "paths differ after overflow sweep %d" % w
        assert ovo > 0 and d.counters()["overflow"] == ovo
        assert check_leaf_states(row, case, po[-1]) >= 1
        check_leaf_states(row, case, d.paths())
        d.close()
        return plan
    Jd, Dd, nd = d.run_mcmc(2, 3, row["seed"], sweep_base=4)
    assert nd == no, (nd, no)
    assert np.array_equal(Jd, Jo) and np.array_equal(Dd, Do)
    pd = d.paths()
    assert orc.paths_equal(pd, po)
    # (SAMPLE_ROOT: the two end sites' cached likelihoods are never read and not kept current, test_sample_root.py)
    lo, hi = (1, -1) if row["opts"].get("sample_root") else (0, None)
    assert np.array_equal(d.tri_llh()[lo:hi].view(np.uint64), to[lo:hi].view(np.uint64))
    assert d.counters()["overflow"] == ovo
    assert d.phase_plan() == plan
    assert check_leaf_states(row, case, po) >= 1          # the oracle moved a soft cell: the row saw the leaf rule
    check_leaf_states(row, case, pd)
    d.close()
    return plan


_CODE = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import json
import test_leaf_matrix as m
print("ok", json.dumps(m.run_row(m.ROW[%(id)r])))
'''


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_leaf_kernel_matches_rung_b(row):
    if not row["env"]:
        run_row(row)
        return
    code = _CODE % dict(root=_ROOT, tests=_TESTS, id=row["id"])
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **row["env"]), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]


# ---- without a GPU
def test_rows_cover_the_leaf_matrix():
    """the table names all eight (gpool, refq, leaf mode) instantiations that take a mask or a table"""
    seen = set((r["expect"]["gpool"], r["expect"]["refq"], "evidence" if r["expect"]["evidence"] else "mask")
               for r in ROWS)
    for gpool in (False, True):
        for refq in (False, True):
            for leaf in ("mask", "evidence"):
                assert (gpool, refq, leaf) in seen, (gpool, refq, leaf)
    assert len(ROW) == len(ROWS)
    for r in ROWS:
        assert r["n"] % 32 != 0 and r["expect"]["propose"] == "V1"
        assert r["n"] <= (600 if r["tree"] == "bal16" else 2000)
    kids = lambda t: np.bincount(t.parent_ids[1:], minlength=t.n_nodes)
    assert max(kids(make_tree("multi"))[1:]) == 3
    depth = lambda t, v: 0 if v == 0 else 1 + depth(t, int(t.parent_ids[v]))
    cat = make_tree("cat6")
    assert sorted(set(depth(cat, v) for v in leaf_nodes(cat))) == list(range(1, max(depth(cat, v) for v in leaf_nodes(cat)) + 1))
    assert make_tree("pair").n_nodes == 2 and make_tree("long").n_nodes == 2


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_row_content_and_oracle_leg(row):
    """the content is what the module says, and the oracle's leg of the row moves a soft cell (so the GPU's
    comparison with it sees the leaf rule), keeps every pinned cell and overflows where it should"""
    case = make_case(row)
    model, tree, fp, mask, r, cap = case
    n = fp.n_sites
    leaves = [b - 1 for b in leaf_nodes(tree)]
    inner = [b for b in range(tree.n_nodes - 1) if b not in leaves]
    if mask is not None:
        assert not mask[inner].any()
    if r is not None:
        assert np.isnan(r[inner]).all()
        assert (((r >= 0) & (r <= 1)) | np.isnan(r)).all()
        ends = leaf_ends(tree, fp)[1:]
        pinned = (r == 0) | (r == 1)
        assert np.array_equal(r[pinned].astype(np.uint8), ends[pinned])          # a hard cell agrees with the data
    if row["content"] == "ev":
        for b in leaves:
            have = r[b][~np.isnan(r[b])]
            for v in SPECIAL[2:]:
                assert np.any(have.view(np.uint32) == np.float32(v).view(np.uint32)), (row["id"], b, v)
            assert np.any(have == 0) and np.any(have == 1)
            for s in edge_sites(n):
                assert mask[b, s] or not np.isnan(r[b, s])
        both = (mask != 0) & ~np.isnan(r)
        assert 0 < both.sum() <= 4 * len(leaves) + 1
        frac_m, frac_e = mask[leaves].mean(), (~np.isnan(r[leaves])).mean()
        assert 0.1 < frac_m < 0.2 and 0.1 < frac_e < 0.2, (frac_m, frac_e)
    if row["content"] == "all":
        assert not np.isnan(r[leaves]).any()
    J, D, nacc, paths, tri, overflow = oracle_leg(row, case)
    last = paths[-1] if row["mode"] == "overflow" else paths
    assert check_leaf_states(row, case, last) >= 1, row["id"]
    if row["mode"] == "overflow":
        assert overflow > 0
    else:
        assert overflow == 0 and np.isfinite(tri[1:-1]).all()


# ---- one genome, two contexts with halos
@pytest.mark.gpu
def test_two_contexts_with_halos_equal_one_context():
    """ev-lds cut by hand at a site that is no multiple of 32: each context gets the table's and the mask's
    columns of its local sites, halos included; the integer totals add up and the paths are the same"""
    from epievo_amd.parallel import concat_sites
    from epievo_amd.sampler import DeviceSampler
    row = ROW["ev-lds"]
    case = make_case(row)
    model, tree, fp, mask, r, cap = case
    n, cut, H = fp.n_sites, 1013, 34               # 5 sweeps = 15 colour phases need 30 halo columns
    one = make_device(row, case)
    counts, nacc = one.run_mcmc_counts(2, 3, SEED, sweep_base=4)
    parts = []
    for lo, hi, halo in ((0, cut + H, (0, H)), (cut - H, n, (H, 0))):
        d = DeviceSampler(0)
        d.set_tree(tree)
        d.set_model(model)
        d.upload_paths(fp.slice_sites(lo, hi), cap, lo, n)
        d.set_halo(*halo)
        d.set_options(**row["opts"])
        d.set_unobserved(mask[:, lo:hi])
        d.set_leaf_evidence(r[:, lo:hi])
        d.reset()
        assert d.phase_plan()["evidence"] and d.phase_plan()["unobs"] and d.halo_phases_left() >= 15
        parts.append(d)
    res = [d.run_mcmc_counts(2, 3, SEED, sweep_base=4) for d in parts]
    assert np.array_equal(res[0][0] + res[1][0], counts) and res[0][1] + res[1][1] == nacc
    got = concat_sites([parts[0].paths().slice_sites(0, cut), parts[1].paths().slice_sites(H, n - cut + H)])
    assert orc.paths_equal(got, one.paths())
    Jo, Do, no, po, to, _ = oracle_leg(row, case)
    J, D = one.counts_to_stats(res[0][0] + res[1][0], 3)
    assert np.array_equal(J, Jo) and np.array_equal(D, Do) and nacc == no and orc.paths_equal(got, po)
    for d in parts + [one]:
        d.close()


# ---- life cycle with content
@pytest.mark.gpu
def test_capacity_and_rescaling_keep_the_table_and_the_mask():
    """after set_capacity and after scale_jump_times under a held table the next run_mcmc is the oracle's,
    treated the same way"""
    row = ROW["ev-lds"]
    case = make_case(row)
    model, tree, fp, mask, r, cap = case
    d, o = make_device(row, case), make_oracle(row, case)

    def step(base):
        Jd, Dd, nd = d.run_mcmc(1, 2, SEED, sweep_base=base)
        Jo, Do, no, _ = o.run_mcmc(1, 2, sweep_base=base)
        assert nd == no and np.array_equal(Jd, Jo) and np.array_equal(Dd, Do)
        assert orc.paths_equal(d.paths(), o.paths())
        assert np.array_equal(d.tri_llh().view(np.uint64), o.tri_llh().view(np.uint64))

    step(0)
    cells = (d.unobserved_cells(), d.leaf_evidence_cells())
    d.set_capacity(2 * cap)
    o.set_rung("B", 2 * cap)
    apply_options(o, row["opts"])
    assert (d.unobserved_cells(), d.leaf_evidence_cells()) == cells
    step(3)
    nb = tree.branches * 1.03
    d.scale_jump_times(nb)
    o.scale_jump_times(nb)
    d.reset()
    o.reset()
    assert (d.unobserved_cells(), d.leaf_evidence_cells()) == cells and d.phase_plan()["evidence"]
    step(6)
    assert check_leaf_states(row, case, o.paths()) >= 1
    d.close()


# ---- a hard cell against the resident path
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["telescoped", "reference"])
def test_contradicting_hard_cell(mode):
    """r = 0 or 1 against the path's end state (the programs refuse such input; the ABI does not look).
    Default ratio: the cell takes the evidence's state at its site's first accepted update and keeps it.
    Reference ratio: the sums are not finite (epv_log(0), epv_exp of -inf or NaN); the GPU decides what the
    oracle's arithmetic decides, and nothing non-finite reaches tri_llh, J or D."""
    from epievo_amd.sampler import DeviceSampler
    from test_leaf_oracle import contradicting_case, check_repair
    model, tree, fp, r, cells = contradicting_case()
    cap = int(max(16, 2 * fp.counts().max() + 8))
    opts = {"reference_proposal_ratio": True} if mode == "reference" else {}
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    d.set_options(**opts)
    d.set_leaf_evidence(r)
    d.reset()
    assert d.phase_plan()["refq"] == (mode == "reference") and d.phase_plan()["evidence"]
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=29)
    apply_options(o, opts)
    o.set_leaf_evidence(r)
    o.reset()
    snaps = []
    for w in range(5):
        assert d.sweep(1, 29, sweep_base=w) == o.sweep(w)
        snaps.append(d.paths())
        assert orc.paths_equal(snaps[-1], o.paths()), w
        assert np.array_equal(d.tri_llh().view(np.uint64), o.tri_llh().view(np.uint64)), w
    Jd, Dd = d.suffstats()
    Jo, Do = o.suffstats()
    assert np.array_equal(Jd, Jo) and np.array_equal(Dd, Do)
    assert np.isfinite(Jd).all() and np.isfinite(Dd).all() and np.isfinite(d.tri_llh()).all()
    repaired = check_repair(tree, fp, snaps, cells)
    if mode == "telescoped":
        assert repaired == len(cells)
    d.close()
