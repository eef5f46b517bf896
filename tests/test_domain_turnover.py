"""Domain turnover, the parts that need no GPU: the numpy yardstick (tests/turnover_ref.py) against a plain
per-site walk on every simulated configuration, where no turned-over class may be vacuous; the three identities of
parts through the C functions (merge of the pieces = part of the whole, merging is associative, a closed part holds
every site of every row once), with runs whose only kept site lies in another piece; the file of
epievo_est_histories -R through its writer and reader; the summary helper; the option errors of the program; and
the declared symbols.  The device side is in test_domain_turnover_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import domains_ref as dr
import turnover_ref as tr
from common import simulate
from epievo_amd import _build, host

EXE = os.path.join(_build.BIN_DIR, "epievo_est_histories")
CASES = ["tree", "pair", "cat6", "multi", "star4", "bal16"]


@pytest.fixture(scope="module", params=CASES)
def sample(request):
    model, tree, fp = simulate(request.param, 3000, seed=6)
    return request.param, tree, fp, tr.rows(fp)


def test_yardstick_equals_a_per_site_walk(sample):
    cfg, tree, fp, x = sample
    B, n = tree.n_nodes - 1, fp.n_sites
    assert x.shape == (2 * B, n) and x.dtype == np.uint8
    hist, len_sum = tr.close(*tr.part(x))
    init = fp.init.reshape(B, n).tolist()
    counts = fp.counts().reshape(B, n).tolist()
    wh, wl = tr.brute(init, counts)
    assert np.array_equal(hist, wh) and np.array_equal(len_sum, wl)
    assert (len_sum.sum(axis=(1, 2)) == n).all() and not hist[:, :, :, 0].any()
    # summed over kept, a row's runs are the runs of the domain size spectra's yardstick on that row
    dh, dl = dr.walk(x)
    assert np.array_equal(hist.sum(axis=2), dh) and np.array_equal(len_sum.sum(axis=2), dl)


def test_no_turned_over_class_is_vacuous_on_the_simulated_inputs(sample):
    cfg, tree, fp, x = sample
    hist, _ = tr.close(*tr.part(x))
    born, died, filled, opened = tr.turned_over_counts(hist)
    assert born > 0 and died > 0 and filled > 0 and opened > 0, (cfg, born, died, filled, opened)
    runs = hist.sum(axis=3)
    assert (runs[:, :, 1].sum(axis=1) > 0).all()                             # every row keeps something


def _random_pair(rng, n):
    """a start row and an end row [2, n]: the start row of very different run lengths, the end row the start row
    changed at no site, at every site, at single sites or over stretches"""
    kind = rng.integers(0, 4)
    if kind == 0:
        a = rng.integers(0, 2, n)
    elif kind == 1:
        a = np.cumsum(rng.random(n) < 0.05) & 1
    elif kind == 2:
        a = np.full(n, rng.integers(0, 2))
    else:
        a = (np.cumsum(rng.random(n) < 0.3) + rng.integers(0, 2)) & 1
    kind = rng.integers(0, 5)
    if kind == 0:
        c = np.zeros(n, np.int64)
    elif kind == 1:
        c = np.ones(n, np.int64)
    elif kind == 2:
        c = (rng.random(n) < 0.9).astype(np.int64)                           # few kept sites: most runs turned over
    elif kind == 3:
        c = np.cumsum(rng.random(n) < 0.1) & 1
    else:
        c = np.ones(n, np.int64)
        c[rng.integers(0, n)] = 0                                            # a single kept site
    return np.stack([a, a ^ c]).astype(np.uint8)


def _pieces(rng, n):
    """cut points of 1-6 stretches of [0, n), empty, one-site and whole stretches included"""
    k = int(rng.integers(1, 7))
    cuts = np.sort(rng.integers(0, n + 1, k - 1)) if k > 1 else np.zeros(0, np.int64)
    if k > 2 and rng.random() < 0.3:
        cuts[1] = cuts[0]                                                    # an empty stretch
    if k > 2 and rng.random() < 0.3 and cuts[0] + 1 <= n:
        cuts[1] = cuts[0] + 1                                                # a one-site stretch
        cuts = np.sort(cuts)
    return [0] + [int(c) for c in cuts] + [n]


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _part_of(xs, a, b):
    p = tr.part(xs[0][:, a:b])
    for x in xs[1:]:
        p = tr.add_parts(p, tr.part(x[:, a:b]))
    return p


def test_merge_and_close_identities_through_the_c_functions():
    rng = np.random.default_rng(5)
    whole_parts = empty_parts = kept_elsewhere = 0
    for trial in range(300):
        Bp, n, ns = int(rng.integers(1, 3)), int(rng.integers(1, 201)), int(rng.integers(1, 4))
        xs = [np.concatenate([_random_pair(rng, n) for _ in range(Bp)]) for _ in range(ns)]
        cuts = _pieces(rng, n)
        parts = [_part_of(xs, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
        for (a, b), p in zip(zip(cuts[:-1], cuts[1:]), parts):
            whole_parts += int(b > a and (p[2][:, :, 0] & np.uint64(tr.WHOLE)).any())
            empty_parts += int(b == a)
        full = _part_of(xs, 0, n)
        # 1. merge(parts of the pieces) = part(concatenation), by the yardstick and by the C function
        assert _same(tr.merge(parts), full)
        got = host.turnover_parts_merge(parts)
        assert all(g.dtype == np.uint64 for g in got) and _same(got, full)
        # 2. associative: any split into two groups merged first
        if len(parts) >= 2:
            j = int(rng.integers(1, len(parts)))
            left, right = host.turnover_parts_merge(parts[:j]), host.turnover_parts_merge(parts[j:])
            assert _same(host.turnover_parts_merge([left, right]), full)
        # 3. closing: every site of every row once; the C function equals the yardstick
        hist, len_sum = host.turnover_part_close(*got)
        assert _same((hist, len_sum), tr.close(*full))
        assert (len_sum.sum(axis=(1, 2)) == ns * n).all()
        assert _same(got, full)                                              # close works on copies
        # a run that the union keeps although the piece that holds its first site shows it turned over
        ff, pf = full[2][:, :, 0], parts[[b > a for a, b in zip(cuts[:-1], cuts[1:])].index(True)][2][:, :, 0]
        kept_elsewhere += int(((ff & np.uint64(tr.KEPT)) > (pf & np.uint64(tr.KEPT))).any())
    assert whole_parts > 50 and empty_parts > 20 and kept_elsewhere > 20     # the cases were met


def test_single_records():
    """a run whose only kept site lies in another piece; a whole part between two others"""
    x = np.array([[0, 1, 1, 1, 1, 1, 0, 0], [0, 0, 0, 0, 1, 0, 1, 1]], np.uint8)   # the run of 1s keeps site 4 only
    a, b, c = tr.part(x[:, :3]), tr.part(x[:, 3:4]), tr.part(x[:, 4:])
    assert int(a[2][0, 0, 1]) == tr.record(2, 1, False) and int(b[2][0, 0, 0]) == tr.record(1, 1, False, True)
    assert int(c[2][0, 0, 0]) == tr.record(2, 1, True)
    hist, len_sum, edges = host.turnover_parts_merge([a, b, c])
    assert hist[0, 1, 1, 5] == 1 and hist[0].sum() == 1 and len_sum[0].tolist() == [[0, 0], [0, 5]]
    assert [int(e) for e in edges[0, 0]] == [tr.record(1, 0, True), tr.record(2, 0, False)]
    assert _same((hist, len_sum, edges), tr.part(x))
    # without the piece that holds the kept site the joined run stays turned over
    hist, len_sum, edges = host.turnover_parts_merge([a, b])
    assert int(edges[0, 0, 1]) == tr.record(3, 1, False) and not hist.any()
    one_site = tr.part(np.array([[1], [0]], np.uint8))
    assert int(one_site[2][0, 0, 0]) == tr.record(1, 1, False, True) == int(one_site[2][0, 0, 1])
    assert int(one_site[2][0, 1, 0]) == tr.record(1, 0, False, True)
    with pytest.raises(ValueError):
        host.turnover_parts_merge([])
    with pytest.raises(ValueError):
        host.turnover_parts_merge([a, (a[0], a[1], np.zeros((2, 2, 2), np.uint64))])


def test_file_round_trip(sample, tmp_path):
    cfg, tree, fp, x = sample
    B = tree.n_nodes - 1
    hist, len_sum = tr.close(*tr.part(x))
    hist[1, 1, 0, 127] += np.uint64(2 ** 40)                                 # the last bin, a count beyond 32 bits
    names = list(tree.node_names)[1:]
    path = str(tmp_path / "turnover.txt")
    host.write_domain_turnover(path, names, 7, hist, len_sum)
    got = host.read_domain_turnover(path)
    assert got["samples"] == 7 and got["branch_names"] == names
    assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], hist) and np.array_equal(got["len_sum"], len_sum)
    lines = open(path).read().split("\n")
    assert lines[0] == "#samples\t7\tbins\t128" and lines[1] == "BRANCH:" + names[0]
    assert lines[2] == "start\tstate\t0\tkept\t0\truns\t%d\tsites\t%d" % (hist[0, 0, 0].sum(), len_sum[0, 0, 0])
    first = int(np.nonzero(hist[0, 0, 0])[0][0])
    lo, hi = dr.bin_range(first)
    assert lines[3] == "%d\t%d\t%d" % (lo, hi, hist[0, 0, 0, first])
    heads = [l for l in lines if l.startswith(("start", "end"))]
    assert len(heads) == 8 * B and heads[4].startswith("end\tstate\t0\tkept\t0\t") and heads[7].startswith("end\tstate\t1\tkept\t1\t")
    assert all(c in "0123456789\t" for l in lines if l and l[0].isdigit() for c in l)   # integers only
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("#samples\t7\tbins\t128\nBRANCH:A\nstart\tstate\t0\tkept\t0\truns\t1\tsites\t3\n3\t4\t1\n")
    with pytest.raises(RuntimeError, match="range of a bin"):
        host.read_domain_turnover(bad)
    open(bad, "w").write("#samples\t7\tbins\t128\nBRANCH:A\nstart\tstate\t0\tkept\t0\truns\t0\tsites\t0\n")
    with pytest.raises(RuntimeError, match="lacks a class"):
        host.read_domain_turnover(bad)
    with pytest.raises(ValueError):
        host.write_domain_turnover(path, ["a"] * (B + 1), 1, hist, len_sum)


def test_summary_helper(sample):
    cfg, tree, fp, x = sample
    B, n = tree.n_nodes - 1, fp.n_sites
    hist, len_sum = tr.close(*tr.part(x))
    s = host.domain_turnover_summary(3, hist * np.uint64(3), len_sum * np.uint64(3), tree)   # three equal samples
    born, died, filled, opened = tr.turned_over_counts(hist)
    assert s["born"].shape == (B,) and s["born"].sum() == born and s["died"].sum() == died
    assert s["merged"].sum() == filled and s["split"].sum() == opened
    for b in range(B):
        a, e = x[2 * b].astype(np.int64), x[2 * b + 1].astype(np.int64)
        assert s["parent_domains"][b] == int((np.diff(a) == 1).sum()) + int(a[0])     # the runs of 1s, counted directly
        assert s["child_domains"][b] == int((np.diff(e) == 1).sum()) + int(e[0])
        if s["born"][b]:
            assert s["born_size"][b] == len_sum[2 * b + 1, 1, 0] / hist[2 * b + 1, 1, 0].sum()
        else:
            assert np.isnan(s["born_size"][b])
    with pytest.raises(ValueError):
        host.domain_turnover_summary(3, hist[:-1], len_sum, tree)


def _run(*args):
    return subprocess.run([EXE] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_option_errors_come_before_any_device(tmp_path):
    """refused on the options alone (the input files do not even exist): a batch beyond the 2^21 samples the edge
    records take, and -w, which the turnover has no use for"""
    files = [tmp_path / "p.param", tmp_path / "t.nwk", tmp_path / "in.local_paths"]
    r = _run("-o", tmp_path / "o.paths", "-R", tmp_path / "r.txt", "-B", 2 ** 21 + 1, *files)
    assert r.returncode != 0 and "-R/--turnover" in r.stderr and "2^21" in r.stderr, r.stderr
    r = _run("-o", tmp_path / "o.paths", "-R", tmp_path / "r.txt", "-w", 5, *files)
    assert r.returncode != 0 and "-w/--window belongs to" in r.stderr, r.stderr
    r = _run("-o", tmp_path / "o.paths", "-R", tmp_path / "r.txt", "-B", 2 ** 21, *files)   # the option itself is taken
    assert r.returncode != 0 and "-R/--turnover" not in r.stderr and "p.param" in r.stderr, r.stderr
    assert not (tmp_path / "r.txt").exists()
    assert "-R, -turnover" in _run().stderr                                  # the usage lists it


def test_turnover_symbols_declared():
    from epievo_amd.driver import DRIVER_SYMBOLS
    from epievo_amd.sampler import ABI_SYMBOLS
    for s in ("epv_set_domain_turnover", "epv_reset_domain_turnover", "epv_accumulate_domain_turnover",
              "epv_domain_turnover_samples", "epv_domain_turnover_layout", "epv_get_domain_turnover"):
        assert s in ABI_SYMBOLS
    for s in ("epvd_set_turnover", "epvd_reset_turnover", "epvd_accumulate_turnover", "epvd_turnover_part_sizes",
              "epvd_download_turnover_part", "epvd_download_turnover"):
        assert s in DRIVER_SYMBOLS
    header = open(os.path.join(_build.INCLUDE, "epievo_mi355x.h")).read()
    for s in ABI_SYMBOLS:
        if "turnover" in s:
            assert "int %s(" % s in header
    L = host.lib()
    for s in ("epvh_turnover_parts_merge", "epvh_turnover_part_close", "epvh_write_domain_turnover",
              "epvh_read_domain_turnover"):
        assert hasattr(L, s)
