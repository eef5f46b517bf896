"""The head of the fused colour phase -- the buffers of the five columns around a site, the matrix table and the
constants in one batch of loads, the meta words and the two outer columns (s_edge) in a second one -- against the
oracle's parallel rung B, bit for bit, at 16, 32 and 64 sites per wave.

What the head can get wrong shows where a wave's first or last valid lane is special: lane 0 fetches the column two
sites to its left, the last valid lane the one two sites to its right, one lane may be both, either column may lie
beyond the genome's end (zero words) or in a halo, and the lanes behind the last valid one load from clamped
addresses.  So the shapes are

  tiny     n = 3, 4, 5, 6: one to four interior sites, every colour's wave has one or two valid lanes, lane 0 is the
           last valid lane and has no left or no right outer column, or neither
  tails    n = 3 L + 2 + r, r = 0 .. 6, at each width L: the colours have L + (r + 2 - c') // 3 sites, so that every
           colour gets a last wave with exactly one valid lane (r = 1 .. 3) and with exactly two (r = 4 .. 6; r = 6
           for colour 0), and n = 6 L + 2: two full waves per colour
  trees    pair (NN = 2), tree (NN = 5), bal8 (generic body, 14 branches: the outer columns span four groups of the
           unrolled branch loop) and star5 (generic body, 5 branches: the acceptance reads the cached outer columns,
           which it does up to 8 branches only)
  cuts     two contexts cut by hand with a halo of 37 columns: the right one has g0 > 0, lane 0's left outer column
           in its halo, and an owned range that starts inside a wave in every phase of the run
  dense    weak-tree40 of dense_cases.py: columns with several jumps on both sides, so that the acceptance reads both
           outer columns with jumps in them

Every case runs 2 burn-in and 3 batch sweeps (run_mcmc_counts) and compares the paths, the integer J and D totals of
every batch sweep, their sum and the accept count.  Each (tree, width) row runs in a fresh process, because a context
reads EPV_FUSED_LANES when it is created, and asserts the plan: the fused phase, the expected body, the width.
Without a GPU the oracle's side of every case runs here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_cases as dc
import orc
from common import config, ref_test_model
from epievo_amd import host

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TESTS = os.path.dirname(os.path.abspath(__file__))

WIDTHS = (16, 32, 64)
BURN_IN, BATCH, SEED, BASE, SIM_SEED = 2, 3, 29, 4, 6
TINY = (3, 4, 5, 6)
TAIL_R = (0, 1, 2, 3, 4, 5, 6)
# (tree, node count of the small-tree body or 0 for the generic one)
TREES = (("pair", 2), ("tree", 5), ("bal8", 0), ("star5", 0))
# (n, cut, halo): context A holds [0, cut + halo) and owns [0, cut), B holds [cut - halo, n) and owns [cut, n);
# 15 colour phases use up 30 halo columns
CUTS = ((257, 129, 37), (700, 300, 37))
DENSE = "weak-tree40"
# (whether the record pool "typically" fits LDS, and with it the plan, turns on a sample's mean jump count -- the
# dense histories and some lengths of the larger trees go to other kernels -- so the pool is kept in LDS by the knob)
ROWS = [(t, nn, L, {"EPV_FUSED_PHASE": "1", "EPV_FUSED_LANES": str(L), "EPV_FORCE_LDS_POOL": "1"})
        for t, nn in TREES for L in WIDTHS]


def lengths(L):
    return list(TINY) + [3 * L + 2 + r for r in TAIL_R] + [6 * L + 2]


def colour_sites(n, colour, g0=0, first=1, last=None):
    """the local sites of one colour phase over [first, last] (the whole interior by default), ascending"""
    last = n - 2 if last is None else last
    return [s for s in range(first, last + 1) if (g0 + s) % 3 == colour]


def last_wave_lanes(count, L):
    """valid lanes of a colour's last wave"""
    return (count - 1) % L + 1 if count else 0


def make_input(tree_name, n):
    model, tree = ref_test_model(), config(tree_name)
    fp = host.simulate(model, tree, n, SIM_SEED)
    return model, tree, fp, int(max(16, 2 * fp.counts().max() + 8))


def dense_input():
    model, tree, fp = dc.workload(DENSE)
    return model, tree, fp, dc.capacity(DENSE, fp)


def oracle_run(tree, model, fp, cap, seed):
    """rung B, twice: run_mcmc(BURN_IN, BATCH) as one call -> (J, D, accepted, paths), and sweep by sweep -> the
    (J, D) of every batch sweep alone.  Both end on the same paths."""
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    o.reset()
    J, D, nacc, _ = o.run_mcmc(BURN_IN, BATCH, sweep_base=BASE)
    paths = o.paths()
    o.close()
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    o.reset()
    for w in range(BURN_IN):
        o.sweep(BASE + w)
    per_sweep = [o.run_mcmc(0, 1, sweep_base=BASE + BURN_IN + k)[:2] for k in range(BATCH)]
    assert orc.paths_equal(o.paths(), paths)
    o.close()
    return J, D, nacc, paths, per_sweep


_CHILD = r'''
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import orc
import dense_cases as dc
import test_fused_head_batch as hb
from epievo_amd.sampler import DeviceSampler
spec = json.loads(%(spec)r)
L = spec["width"]

def device(model, tree, fp, cap, offset=0, n_global=None, halo=None):
    d = DeviceSampler(0); d.set_tree(tree); d.set_model(model); d.upload_paths(fp, cap, offset, n_global)
    if halo:
        d.set_halo(*halo)
    d.reset()
    plan = d.phase_plan()
    assert plan["propose"] == "fused" and plan["small_nn"] == spec["small_nn"] and plan["fused_lanes"] == L, plan
    return d

def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)

def check(label, devs, owned, expect):
    """devs: the contexts of one genome; owned: per context (local first, local end, global first) of its sites"""
    J, D, nacc, paths, per_sweep = expect
    runs = [d.run_mcmc_counts(hb.BURN_IN, hb.BATCH, spec["seed"], sweep_base=hb.BASE) for d in devs]
    counts, got = sum(r[0] for r in runs), sum(r[1] for r in runs)
    print(label, "accepted", got, "oracle", nacc, flush=True)
    assert got == nacc, (label, got, nacc)
    for d, (lo, hi, g) in zip(devs, owned):
        assert orc.paths_equal(d.paths().slice_sites(lo, hi), paths.slice_sites(g, g + hi - lo)), (label, "paths")
    d = devs[0]
    for k, (Jk, Dk) in enumerate(per_sweep):
        Jd, Dd = d.counts_to_stats(counts[k:k + 1], 1)
        assert np.array_equal(Jd, Jk) and np.array_equal(bits(Dd), bits(Dk)), (label, "batch sweep", k)
    Jd, Dd = d.counts_to_stats(counts, hb.BATCH)
    assert np.array_equal(Jd, J) and np.array_equal(bits(Dd), bits(D)), (label, "totals")
    for d in devs:
        d.close()

for n in hb.lengths(L):
    model, tree, fp, cap = hb.make_input(spec["tree"], n)
    check("n=%%d" %% n, [device(model, tree, fp, cap)], [(0, n, 0)], hb.oracle_run(tree, model, fp, cap, spec["seed"]))
for n, cut, halo in hb.CUTS:
    model, tree, fp, cap = hb.make_input(spec["tree"], n)
    a = device(model, tree, fp.slice_sites(0, cut + halo), cap, 0, n, (0, halo))
    b = device(model, tree, fp.slice_sites(cut - halo, n), cap, cut - halo, n, (halo, 0))
    check("cut=%%d/%%d" %% (cut, n), [a, b], [(0, cut, 0), (halo, n - cut + halo, cut)],
          hb.oracle_run(tree, model, fp, cap, spec["seed"]))
if spec["dense"]:
    model, tree, fp, cap = hb.dense_input()
    check("dense", [device(model, tree, fp, cap)], [(0, fp.n_sites, 0)], hb.oracle_run(tree, model, fp, cap, spec["seed"]))
print("ok")
'''


@pytest.mark.gpu
@pytest.mark.parametrize("tree,small_nn,width,env", ROWS, ids=["%s-%d" % (r[0], r[2]) for r in ROWS])
def test_head_batches_match_rung_b(tree, small_nn, width, env):
    spec = dict(tree=tree, small_nn=small_nn, width=width, seed=SEED, dense=tree == "tree")
    src = _CHILD % dict(root=_ROOT, tests=_TESTS, spec=json.dumps(spec))
    clean = dict((k, v) for k, v in os.environ.items() if k not in ("EPV_FUSED_PHASE", "EPV_FUSED_LANES", "EPV_FORCE_LDS_POOL"))
    r = subprocess.run([sys.executable, "-c", src], env=dict(clean, **env), capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]


# ---- without a GPU
def test_lengths_put_one_and_two_sites_in_every_colours_last_wave():
    """plain arithmetic on the tables: tails, tiny genomes, full waves and the cuts"""
    for L in WIDTHS:
        seen = set()
        for r in TAIL_R:
            n = 3 * L + 2 + r
            for c in range(3):
                count = len(colour_sites(n, c))
                assert L <= count <= L + 3
                seen.add((c, last_wave_lanes(count, L) if count > L else 0))
        for c in range(3):
            assert (c, 1) in seen and (c, 2) in seen, (L, c, sorted(seen))
        assert all(len(colour_sites(6 * L + 2, c)) == 2 * L for c in range(3))
        assert lengths(L)[:4] == [3, 4, 5, 6] and len(set(lengths(L))) == len(lengths(L))
    # tiny genomes: a wave's only valid lanes are lane 0 (and 1); some site lacks the left outer column (site 1), some
    # the right one (site n - 2), one both (n = 3, 4: site 1 is also n - 2 or next to it)
    assert [sorted(len(colour_sites(n, c)) for c in range(3)) for n in TINY] == [[0, 0, 1], [0, 1, 1], [1, 1, 1], [1, 1, 2]]
    # cuts: B starts at g0 > 0 with its left halo; over the run's phases the range of a phase starts 2 (p + 1) columns
    # into the halo, so lane 0's left outer column is a halo column, and the first owned site is never a wave's lane 0
    phases = 3 * (BURN_IN + BATCH)
    for n, cut, halo in CUTS:
        assert halo % 2 and halo >= 2 * phases + 2 and 0 < cut - halo and cut + halo < n and cut % 64 and (cut - halo) % 64
        g0 = cut - halo
        for p in range(phases):
            first = 2 * (p + 1)
            assert first - 2 >= 0 and first < halo
            for c in range(3):
                sites = colour_sites(n - g0, c, g0, first, n - g0 - 2)
                lane_of_first_owned = min(i for i, s in enumerate(sites) if s >= halo)
                for L in WIDTHS:
                    assert lane_of_first_owned % L != 0, (n, p, c, L)
        # A: the owned range ends inside a wave as well (its right halo follows)
        for L in WIDTHS:
            assert all(len([s for s in colour_sites(cut + halo, c) if s < cut]) % L for c in range(3))
    names = dict(TREES)
    assert config("pair").n_nodes == 2 and config("tree").n_nodes == 5 and names["pair"] == 2 and names["tree"] == 5
    assert config("bal8").n_nodes - 1 == 14 and 5 < config("star5").n_nodes and config("star5").n_nodes - 1 <= 8
    assert dc.WORKLOADS[DENSE][1] == "tree" and dc.capacity(DENSE, dc.workload(DENSE)[2]) == dc.FUSED_CAP
    assert len(ROWS) == len(TREES) * len(WIDTHS) == len(set((r[0], r[2]) for r in ROWS))


def _oracle_side(tree, model, fp, cap):
    J, D, nacc, paths, per_sweep = oracle_run(tree, model, fp, cap, SEED)
    T = np.asarray(tree.branches)[1:]
    for Jk, Dk in per_sweep:
        assert np.all(Jk >= 0) and np.allclose(Dk.reshape(-1, 8).sum(axis=1), (fp.n_sites - 2) * T, rtol=1e-9, atol=0)
    # the batch average of the sweeps' totals is the one call's
    assert np.allclose(sum(j for j, _ in per_sweep) / BATCH, J, rtol=1e-12, atol=0)
    assert np.allclose(sum(d for _, d in per_sweep) / BATCH, D, rtol=1e-12, atol=0)
    return nacc, not orc.paths_equal(paths, fp)


@pytest.mark.parametrize("tree_name", [t for t, _ in TREES])
def test_oracle_side_of_the_cases(tree_name):
    """rung B on every length of every width and on the cuts' genomes: the sweeps' own totals add up to the call's,
    and no chain stands still -- every length from one wave on accepts a proposal and leaves the input, the tiny
    ones do so between them"""
    tiny_acc = 0
    for n in sorted(set(n for L in WIDTHS for n in lengths(L)) | set(c[0] for c in CUTS)):
        model, tree, fp, cap = make_input(tree_name, n)
        nacc, moved = _oracle_side(tree, model, fp, cap)
        if n in TINY:
            tiny_acc += nacc
        else:
            assert nacc >= 1 and moved, (tree_name, n, nacc, moved)
    assert tiny_acc >= 1, tree_name


def test_oracle_side_of_the_dense_case():
    model, tree, fp, cap = dense_input()
    nacc, moved = _oracle_side(tree, model, fp, cap)
    assert nacc >= 1 and moved
    assert dc.density(fp)["mean"] >= 2.0      # (jumps per path: the outer columns hold some)
