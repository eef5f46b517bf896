"""Spatial correlations, the parts that need no GPU: the numpy yardstick (tests/corr_ref.py) against a plain walk
over sites and pairs on the simulated configurations; the identities of parts through the C functions (merge of the
pieces = part of the whole, merging is associative, the bounds a closed part obeys) on random bit rows cut at
random points, a piece of exactly max_lag sites included; the refusal of a shorter piece; the file of
epievo_est_histories -C through its writer and reader; the summary helper on a periodic row whose correlation is
known in closed form; the option errors of the program; and the declared symbols.  The device side is in
test_spatial_correlation_gpu.py."""
import math
import os
import subprocess

import numpy as np
import pytest

import corr_ref as cr
from common import config, simulate
from epievo_amd import _build, host

EXE = os.path.join(_build.BIN_DIR, "epievo_est_histories")
CASES = [("tree", 600), ("pair", 600), ("multi", 500), ("star4", 421), ("bal16", 300)]
L_SIM = 70


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def sample(request):
    cfg, n = request.param
    model, tree, fp = simulate(cfg, n, seed=6)
    return cfg, tree, fp, cr.rows(fp, tree)


def test_yardstick_equals_a_walk_over_sites_and_pairs(sample):
    cfg, tree, fp, x = sample
    N, n = tree.n_nodes, fp.n_sites
    B = N - 1
    assert x.shape == (N + B, n) and x.dtype == np.uint8
    cnt, n11, edges = cr.part(x, L_SIM)
    assert cnt == n and edges.shape == (1, N + B, 2, 2)
    got = cr.close(cnt, n11, edges)
    want = cr.brute(fp.init.reshape(B, n).tolist(), fp.counts().reshape(B, n).tolist(), list(tree.parent_ids), L_SIM)
    for g, w in zip(got, want):
        assert g.dtype == np.uint64 and np.array_equal(g, w)
    # and through the C close
    for g, w in zip(host.corr_part_close(cnt, n11, edges), want):
        assert g.dtype == np.uint64 and np.array_equal(g, w)


def _random_rows(rng, R, n):
    """[R, n] rows of very different kinds: dense noise, long runs, constant, sparse, periodic"""
    out = np.zeros((R, n), np.uint8)
    for r in range(R):
        kind = rng.integers(0, 6)
        if kind == 0:
            out[r] = rng.integers(0, 2, n)
        elif kind == 1:
            out[r] = np.cumsum(rng.random(n) < 0.05) & 1
        elif kind == 2:
            out[r] = rng.integers(0, 2)
        elif kind == 3:
            out[r] = rng.random(n) < 0.02
        elif kind == 4:
            out[r] = (np.arange(n) % int(rng.integers(2, 70))) == 0
        else:
            out[r] = 1
    return out


def _cuts(rng, n, L, exact):
    """cut points of 1-5 pieces of [0, n), every piece of at least L sites; with `exact` one piece of exactly L"""
    k = int(rng.integers(2 if exact else 1, 6))
    k = max(min(k, n // L), 1)
    sizes = np.full(k, L)
    spare = n - k * L
    free = [i for i in range(k)]
    if exact and k > 1:
        free.remove(int(rng.integers(0, k)))
    for _ in range(3):
        if spare and free:
            i = free[int(rng.integers(0, len(free)))]
            add = int(rng.integers(0, spare + 1))
            sizes[i] += add
            spare -= add
    sizes[free[-1] if free else 0] += spare
    return [0] + [int(c) for c in np.cumsum(sizes)]


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _part_of(xs, a, b, L):
    p = cr.part(xs[0][:, a:b], L)
    for x in xs[1:]:
        p = cr.add_parts(p, cr.part(x[:, a:b], L))
    return p


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 130, 1024])
def test_merge_and_close_identities_through_the_c_functions(L):
    rng = np.random.default_rng(100 + L)
    exact_pieces = several = 0
    for trial in range(6 if L == 1024 else 40):
        R, ns = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        n = int(rng.integers(L, 5 * L + 200)) if trial else 3 * L + 7
        xs = [_random_rows(rng, R, n) for _ in range(ns)]
        cuts = _cuts(rng, n, L, exact=trial % 2 == 0)
        spans = list(zip(cuts[:-1], cuts[1:]))
        assert all(b - a >= L for a, b in spans) and cuts[-1] == n
        exact_pieces += int(len(spans) > 1 and any(b - a == L for a, b in spans))
        several += int(len(spans) > 2)
        parts = [_part_of(xs, a, b, L) for a, b in spans]
        full = _part_of(xs, 0, n, L)
        # 1. merge(parts of the pieces) = part(concatenation), by the yardstick and by the C function
        assert _same(cr.merge(parts), full)
        got = host.corr_parts_merge(parts)
        assert got[1].dtype == np.uint64 and got[2].dtype == np.uint64 and _same(got, full)
        # 2. associative: any split into two groups merged first
        if len(parts) >= 2:
            j = int(rng.integers(1, len(parts)))
            left, right = host.corr_parts_merge(parts[:j]), host.corr_parts_merge(parts[j:])
            assert _same(host.corr_parts_merge([left, right]), full)
        # 3. closing: the C function equals the yardstick, and the bounds of a 2 x 2 table hold
        n11, left1, right1 = host.corr_part_close(*got)
        want = cr.close(*full)
        assert np.array_equal(n11, want[0]) and np.array_equal(left1, want[1]) and np.array_equal(right1, want[2])
        assert (n11 <= np.minimum(left1, right1)).all()
        assert (left1 + right1 - n11 <= cr.pairs(ns, n, L)[None]).all()
        assert np.array_equal(n11[:, 0], left1[:, 0]) and np.array_equal(n11[:, 0], right1[:, 0])
        assert np.array_equal(n11[:, 0], sum(x.sum(axis=1, dtype=np.uint64) for x in xs))
        # the spare bits of the last edge word are zero
        if L % 64:
            assert not (got[2][..., -1] >> np.uint64(L % 64)).any()
        assert _same(got, full)                                              # close works on copies
    assert exact_pieces >= 3 and several >= 3                                # the cases were met


def test_a_piece_shorter_than_max_lag_is_refused():
    rng = np.random.default_rng(3)
    L = 65
    x = _random_rows(rng, 2, 300)
    a, b = cr.part(x[:, :200], L), cr.part(x[:, 200:], L)
    short = (L - 1, b[1], b[2])                                              # claims fewer sites than max_lag
    with pytest.raises(RuntimeError, match="64 sites, fewer than max_lag = 65"):
        host.corr_parts_merge([a, short])
    with pytest.raises(RuntimeError, match="fewer than max_lag"):
        host.corr_parts_merge([short, a])
    with pytest.raises(RuntimeError, match="fewer than max_lag"):
        host.corr_part_close(L - 1, a[1], a[2])
    with pytest.raises(ValueError):
        host.corr_parts_merge([])
    with pytest.raises(ValueError):
        host.corr_parts_merge([a, (200, a[1][:, :-1], a[2])])
    with pytest.raises(ValueError):
        host.corr_part_close(200, np.zeros((2, 1026), np.uint64), np.zeros((1, 2, 2, 17), np.uint64))
    exact = cr.part(x[:, 200:200 + L], L)                                    # exactly max_lag sites is taken
    assert _same(host.corr_parts_merge([a, exact]), cr.part(x[:, :200 + L], L))


def test_file_round_trip(sample, tmp_path):
    cfg, tree, fp, x = sample
    N, n = tree.n_nodes, fp.n_sites
    n11, left1, right1 = cr.close(*cr.part(x, L_SIM))
    n11[1, 3] += np.uint64(2 ** 40)                                          # a count beyond 32 bits
    names = list(tree.node_names)
    path = str(tmp_path / "corr.txt")
    host.write_spatial_correlation(path, names, 7, n, n11, left1, right1)
    got = host.read_spatial_correlation(path)
    assert got["samples"] == 7 and got["sites"] == n and got["max_lag"] == L_SIM
    assert got["row_names"] == ["NODE:" + s for s in names] + ["BRANCH:" + s for s in names[1:]]
    for k, w in (("n11", n11), ("left1", left1), ("right1", right1)):
        assert got[k].dtype == np.uint64 and np.array_equal(got[k], w)
    lines = open(path).read().split("\n")
    assert lines[0] == "#samples\t7\tsites\t%d\tmax_lag\t%d" % (n, L_SIM) and lines[1] == "NODE:" + names[0]
    assert lines[2] == "ones\t%d" % n11[0, 0]
    assert lines[3] == "1\t%d\t%d\t%d" % (n11[0, 1], left1[0, 1], right1[0, 1])
    assert lines[2 + L_SIM] == "%d\t%d\t%d\t%d" % (L_SIM, n11[0, L_SIM], left1[0, L_SIM], right1[0, L_SIM])
    assert lines[N * (L_SIM + 2) + 1] == "BRANCH:" + names[1] and len(lines) == (2 * N - 1) * (L_SIM + 2) + 2
    assert all(c in "0123456789\t" for l in lines if l and l[0].isdigit() for c in l)   # integers only
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("#samples\t7\tsites\t9\tmax_lag\t2\nNODE:A\nones\t3\n1\t1\t2\t2\n")
    with pytest.raises(RuntimeError, match="lacks a lag"):
        host.read_spatial_correlation(bad)
    open(bad, "w").write("#samples\t7\tsites\t9\tmax_lag\t2\nNODE:A\nones\t3\n2\t1\t2\t2\n")
    with pytest.raises(RuntimeError, match="bad lag line"):
        host.read_spatial_correlation(bad)
    open(bad, "w").write("#samples\t7\tsites\t9\tmax_lag\t2000\n")
    with pytest.raises(RuntimeError, match="max_lag"):
        host.read_spatial_correlation(bad)
    with pytest.raises(ValueError):
        host.write_spatial_correlation(path, names + ["x"], 1, n, n11, left1, right1)


def test_summary_helper_on_a_periodic_row():
    """node 1 of a pair: X[p] = 1 iff p % 4 == 0 over n = 4000 sites.  On a ring the correlation at lag d is 1 where
    4 | d and -1/3 elsewhere (margins 1/4: (0 - 1/16) / (3/16)); on the open stretch the counts are exact integers:
    n11[d] = (n - d) / 4 at 4 | d, and the margins differ from 1/4 only by the sites the ends cut off"""
    tree = config("pair")
    n, L, S = 4000, 24, 3
    x = np.zeros((3, n), np.uint8)
    x[1] = (np.arange(n) % 4) == 0                                           # node 1; node 0 constant 0, no change
    x[2] = x[1]                                                              # the branch's changes: the same row
    p = cr.part(x, L)
    for _ in range(S - 1):
        p = cr.add_parts(p, cr.part(x, L))
    n11, left1, right1 = host.corr_part_close(*p)
    s = host.spatial_correlation_summary(S, n, n11, left1, right1, tree)
    assert s["corr"].shape == (3, L + 1) and np.isnan(s["corr"][0]).all() and s["decay"][0] is None
    for d in range(L + 1):
        want11 = (n - d) // 4 if d % 4 == 0 else 0
        assert n11[1, d] == S * want11
        pl, pr = -(-(n - d) // 4) / (n - d), ((n - 1) // 4 - (d - 1) // 4) / (n - d) if d else 0.25
        p11 = want11 / (n - d)
        want = (p11 - pl * pr) / math.sqrt(pl * (1 - pl) * pr * (1 - pr))
        assert s["corr"][1, d] == pytest.approx(want, abs=1e-12)
        assert s["corr"][1, d] == pytest.approx(1.0 if d % 4 == 0 else -1.0 / 3.0, abs=2e-3)   # the ring's value
        tab = [s[k][1, d] for k in ("p11", "p10", "p01", "p00")]
        assert sum(tab) == pytest.approx(1.0, abs=1e-12) and min(tab) >= -1e-15
        assert s["p11"][1, d] == pytest.approx(p11, abs=1e-15)
    assert s["decay"][1] == 1 and s["decay"][2] == 1 and np.array_equal(s["corr"][1], s["corr"][2])
    # a row that stays correlated: one long block of ones
    y = np.zeros((3, n), np.uint8)
    y[1, 1000:3000] = 1
    n11, left1, right1 = host.corr_part_close(*cr.part(y, L))
    s = host.spatial_correlation_summary(1, n, n11, left1, right1, tree)
    assert s["decay"][1] is None and (s["corr"][1] > 0.9).all() and s["corr"][1, 0] == pytest.approx(1.0)
    with pytest.raises(ValueError):
        host.spatial_correlation_summary(1, n, n11[:-1], left1, right1, tree)


def _run(*args):
    return subprocess.run([EXE] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_option_errors_come_before_any_device(tmp_path):
    """refused on the options alone (the input files do not even exist): -M without -C, -M 0, -M 1025, and a batch
    beyond the 2^21 samples the edge records take"""
    files = [tmp_path / "p.param", tmp_path / "t.nwk", tmp_path / "in.local_paths"]
    r = _run("-o", tmp_path / "o.paths", "-M", 5, *files)
    assert r.returncode != 0 and "-M/--maxlag belongs to -C/--correlation" in r.stderr, r.stderr
    for bad in (0, 1025):
        r = _run("-o", tmp_path / "o.paths", "-C", tmp_path / "c.txt", "-M", bad, *files)
        assert r.returncode != 0 and "-M: a largest lag of 1 to 1024 sites" in r.stderr, r.stderr
    r = _run("-o", tmp_path / "o.paths", "-C", tmp_path / "c.txt", "-B", 2 ** 21 + 1, *files)
    assert r.returncode != 0 and "-C/--correlation" in r.stderr and "2^21" in r.stderr, r.stderr
    for ok in (1, 1024):                                                     # the options themselves are taken
        r = _run("-o", tmp_path / "o.paths", "-C", tmp_path / "c.txt", "-M", ok, *files)
        assert r.returncode != 0 and "-M" not in r.stderr and "p.param" in r.stderr, r.stderr
    assert not (tmp_path / "c.txt").exists()
    usage = _run().stderr
    assert "-C, -correlation" in usage and "-M, -maxlag" in usage            # the usage lists them


def test_correlation_symbols_declared():
    from epievo_amd.driver import DRIVER_SYMBOLS
    from epievo_amd.sampler import ABI_SYMBOLS
    for s in ("epv_set_spatial_correlation", "epv_reset_spatial_correlation", "epv_accumulate_spatial_correlation",
              "epv_spatial_correlation_samples", "epv_spatial_correlation_layout", "epv_get_spatial_correlation"):
        assert s in ABI_SYMBOLS
    for s in ("epvd_set_corr", "epvd_reset_corr", "epvd_accumulate_corr", "epvd_corr_part_sizes",
              "epvd_download_corr_part", "epvd_download_corr"):
        assert s in DRIVER_SYMBOLS
    header = open(os.path.join(_build.INCLUDE, "epievo_mi355x.h")).read()
    for s in ABI_SYMBOLS:
        if "spatial_correlation" in s:
            assert "int %s(" % s in header
    L = host.lib()
    for s in ("epvh_corr_parts_merge", "epvh_corr_part_close", "epvh_write_spatial_correlation",
              "epvh_read_spatial_correlation"):
        assert hasattr(L, s)
