"""Change tracts, the parts that need no GPU: the numpy yardstick (tests/tracts_ref.py) against a plain per-site walk
on every simulated configuration, where no pure class may be vacuous; the identities of parts through the C
functions (merge of the pieces = part of the whole with its records, merging is associative, a closed part holds
every changed site once, close of the whole = the walk), with tracts cut in three, tracts that end at a cut and cuts
between a tract and its flank; single records; the file of epievo_est_histories -X through its writer and reader;
the summary helper; the option errors of the program; the declared symbols and the table entries.  The device side
is in test_change_tracts_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import domains_ref as dr
import tracts_ref as xr
from common import simulate
from epievo_amd import _build, host

EXE = os.path.join(_build.BIN_DIR, "epievo_est_histories")
CASES = ["tree", "pair", "cat6", "multi", "star4", "bal16"]


@pytest.fixture(scope="module", params=CASES)
def sample(request):
    model, tree, fp = simulate(request.param, 3000, seed=6)
    return request.param, tree, fp, xr.rows(fp)


def _walk(x):
    """brute on rows [2 B, n]: the start rows as init states, the changes as jump counts"""
    return xr.brute(x[0::2].tolist(), (x[0::2] ^ x[1::2]).tolist())


def test_yardstick_equals_a_per_site_walk(sample):
    cfg, tree, fp, x = sample
    B, n = tree.n_nodes - 1, fp.n_sites
    hist, len_sum = xr.close(*xr.part(x))
    wh, wl = xr.brute(fp.init.reshape(B, n).tolist(), fp.counts().reshape(B, n).tolist())
    assert hist.shape == (B, 27, 128) and np.array_equal(hist, wh) and np.array_equal(len_sum, wl)
    changed = (fp.counts().reshape(B, n) & 1).sum(axis=1)
    assert np.array_equal(len_sum.sum(axis=1), changed) and not hist[:, :, 0].any()
    got = host.tract_part_close(*xr.part(x))               # close(part(whole genome)) = the walk, by the C function
    assert np.array_equal(got[0], wh) and np.array_equal(got[1], wl)


def test_no_pure_class_is_vacuous_on_the_simulated_inputs(sample):
    cfg, tree, fp, x = sample
    hist, _ = xr.close(*xr.part(x))
    counts = xr.pure_counts(hist)
    for d in (0, 1):
        for l in (0, 1):
            for r in (0, 1):
                assert counts[d, l, r] > 0, (cfg, d, l, r)
    if cfg != "tree":
        assert all(counts[2, l, r] > 0 for l in (0, 1) for r in (0, 1)), (cfg, counts)


def _random_pair(rng, n):
    """a start row and an end row [2, n]: changes at no site, at every site, in long tracts, in short ones, at all
    sites but one"""
    kind = rng.integers(0, 3)
    if kind == 0:
        a = rng.integers(0, 2, n)
    elif kind == 1:
        a = np.cumsum(rng.random(n) < 0.05) & 1
    else:
        a = np.full(n, rng.integers(0, 2))
    kind = rng.integers(0, 6)
    if kind == 0:
        c = np.zeros(n, np.int64)
    elif kind == 1:
        c = np.ones(n, np.int64)
    elif kind == 2:
        c = (rng.random(n) < 0.9).astype(np.int64)
    elif kind == 3:
        c = np.cumsum(rng.random(n) < 0.1) & 1                                # long tracts
    elif kind == 4:
        c = (rng.random(n) < 0.3).astype(np.int64)
    else:
        c = np.ones(n, np.int64)
        c[rng.integers(0, n)] = 0                                            # a single unchanged site
    return np.stack([a, a ^ c]).astype(np.uint8)


def _pieces(rng, n, x):
    """cut points of 1-7 stretches of [0, n): empty and one-site stretches, and cuts at the first site of a tract,
    behind its last site and between a tract and its flank"""
    k = int(rng.integers(1, 8))
    cuts = [int(c) for c in rng.integers(0, n + 1, k - 1)]
    c = (x[0] ^ x[1]).astype(np.int64)
    step = np.diff(np.concatenate([[0], c, [0]]))
    starts, ends = np.nonzero(step == 1)[0], np.nonzero(step == -1)[0]        # first site, and the site behind the last
    if len(starts) and cuts:
        i = int(rng.integers(0, len(starts)))
        cuts[0] = int(rng.choice([starts[i], ends[i], max(starts[i] - 1, 0), min(ends[i] + 1, n)]))
    if len(cuts) >= 2 and rng.random() < 0.3:
        cuts[1] = cuts[0]                                                    # an empty stretch
    if len(cuts) >= 2 and rng.random() < 0.3:
        cuts[1] = min(cuts[0] + 1, n)                                        # a one-site stretch
    return [0] + sorted(cuts) + [n]


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _part_of(xs, a, b):
    p = xr.part(xs[0][:, a:b])
    for x in xs[1:]:
        p = xr.add_parts(p, xr.part(x[:, a:b]))
    return p


def test_merge_and_close_identities_through_the_c_functions():
    rng = np.random.default_rng(5)
    whole_parts = empty_parts = in_three = 0
    for trial in range(300):
        Bp, n, ns = int(rng.integers(1, 3)), int(rng.integers(1, 201)), int(rng.integers(1, 4))
        xs = [np.concatenate([_random_pair(rng, n) for _ in range(Bp)]) for _ in range(ns)]
        cuts = _pieces(rng, n, xs[0])
        spans = list(zip(cuts[:-1], cuts[1:]))
        parts = [_part_of(xs, a, b) for a, b in spans]
        for (a, b), p in zip(spans, parts):
            whole_parts += int(b > a and (p[2][:, :, 0] & np.uint64(xr.WHOLE)).any())
            empty_parts += int(b == a)
        c = xs[0][0] ^ xs[0][1]
        in_three += int(any(d > a >= 1 and d < n and c[a - 1:d + 1].all() for a, d in spans[1:-1]))   # a tract in three pieces
        full = _part_of(xs, 0, n)
        # 1. merge(parts of the pieces) = part(concatenation), by the yardstick and by the C function
        assert _same(xr.merge(parts), full), (trial, cuts)
        got = host.tract_parts_merge(parts)
        assert all(g.dtype == np.uint64 for g in got) and _same(got, full), (trial, cuts)
        # 2. associative: any split into two groups merged first
        if len(parts) >= 2:
            j = int(rng.integers(1, len(parts)))
            left, right = host.tract_parts_merge(parts[:j]), host.tract_parts_merge(parts[j:])
            assert _same(host.tract_parts_merge([left, right]), full)
        # 3. closing: every changed site of every branch once; the C function equals the yardstick and the walk
        hist, len_sum = host.tract_part_close(*got)
        assert _same((hist, len_sum), xr.close(*full))
        walked = [_walk(x) for x in xs]
        assert np.array_equal(hist, sum(w[0] for w in walked)) and np.array_equal(len_sum, sum(w[1] for w in walked))
        changed = sum((x[0::2] ^ x[1::2]).sum(axis=1, dtype=np.uint64) for x in xs)
        assert np.array_equal(len_sum.sum(axis=1), changed)
        assert _same(got, full)                                              # close works on copies
    assert whole_parts > 50 and empty_parts > 20 and in_three > 20           # the cases were met


def test_single_records():
    """a tract cut in three; a tract that ends exactly at a cut; a cut between a tract and its flank; empty,
    one-site and whole stretches"""
    #                 0  1  2  3  4  5  6  7  8  9
    a = np.array([0, 0, 0, 1, 0, 1, 1, 1, 0, 0], np.uint8)
    c = np.array([0, 1, 1, 1, 1, 1, 0, 1, 1, 0], np.uint8)                   # tracts 1-5 (mixed, 0 | 1) and 7-8 (mixed, 1 | 0)
    x = np.stack([a, a ^ c])
    full = xr.part(x)
    assert full[0][0, xr.cls_of(2, 0, 1), 5] == 1 and full[0][0, xr.cls_of(2, 1, 0), 2] == 1 and full[0].sum() == 2
    assert [int(e) for e in full[2][0, 0]] == [xr.record(0, 0), xr.record(0, 0)]
    # the tract 1-5 cut in three: sites 0-2, 3, 4-9
    p, q, r = xr.part(x[:, :3]), xr.part(x[:, 3:4]), xr.part(x[:, 4:])
    assert int(p[2][0, 0, 1]) == xr.record(2, 1, gain=1, flank=0)             # sites 1, 2 gained, behind site 0 (y = 0)
    assert int(q[2][0, 0, 0]) == xr.record(1, 0, loss=1, whole=True) == int(q[2][0, 0, 1])
    assert int(r[2][0, 0, 0]) == xr.record(2, 1, gain=1, loss=1, flank=1)     # site 4 gained, 5 lost, before site 6 (y = 1)
    assert not p[0].any() and not q[0].any() and r[0].sum() == 1
    for merge in (xr.merge, host.tract_parts_merge):
        assert _same(merge([p, q, r]), full)
        hist, len_sum, edges = merge([p, q])                                  # without the last piece the tract stays open
        assert not hist.any() and int(edges[0, 0, 1]) == xr.record(3, 0, gain=1, loss=1, flank=0)
        # the tract ends exactly at the cut 6: its right flank is the neighbour's first site
        left, right = xr.part(x[:, :6]), xr.part(x[:, 6:])
        assert int(left[2][0, 0, 1]) == xr.record(5, 0, gain=1, loss=1, flank=0) and int(right[2][0, 0, 0]) == xr.record(0, 1)
        assert _same(merge([left, right]), full)
        # a cut between the tract and its flank on either side (1: before site 1; 7: between the flank 6 and tract 7-8)
        assert _same(merge([xr.part(x[:, :1]), xr.part(x[:, 1:7]), xr.part(x[:, 7:])]), full)
        # empty stretches anywhere change nothing
        e = xr.part(x[:, 4:4])
        assert not e[2].any() and _same(merge([e, p, e, e, q, r, e]), full)
        assert not merge([e, e])[2].any()
    # all sites changed: one whole record, closed with both flanks none
    w = xr.part(np.stack([a, a ^ 1]))
    assert int(w[2][0, 0, 0]) == xr.record(10, 1, gain=1, loss=1, whole=True)
    assert int(w[2][0, 0, 1]) == xr.record(10, 1, gain=1, loss=1, whole=True)
    hist, len_sum = host.tract_part_close(*w)
    assert hist[0, xr.cls_of(2, 2, 2), 10] == 1 and hist.sum() == 1 and len_sum[0, 26] == 10
    # tracts at the genome's ends take flank none
    ends = np.array([[0, 0, 1, 1, 1], [1, 0, 1, 0, 0]], np.uint8)             # site 0 gained; sites 3-4 lost
    hist, len_sum = host.tract_part_close(*xr.part(ends))
    assert hist[0, xr.cls_of(0, 2, 0), 1] == 1 and hist[0, xr.cls_of(1, 1, 2), 2] == 1 and hist.sum() == 2
    with pytest.raises(ValueError):
        host.tract_parts_merge([])
    with pytest.raises(ValueError):
        host.tract_parts_merge([p, (p[0], p[1], np.zeros((2, 2, 2), np.uint64))])


def test_file_round_trip(sample, tmp_path):
    cfg, tree, fp, x = sample
    B = tree.n_nodes - 1
    hist, len_sum = xr.close(*xr.part(x))
    hist[0, 26, 127] += np.uint64(2 ** 40)                                   # the last bin, a count beyond 32 bits
    len_sum[0, 26] += np.uint64(2 ** 50)
    names = list(tree.node_names)[1:]
    path = str(tmp_path / "tracts.txt")
    host.write_change_tracts(path, names, 7, hist, len_sum)
    got = host.read_change_tracts(path)
    assert got["samples"] == 7 and got["branch_names"] == names
    assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], hist) and np.array_equal(got["len_sum"], len_sum)
    lines = open(path).read().split("\n")
    assert lines[0] == "#samples\t7\tbins\t128" and lines[1] == "BRANCH:" + names[0]
    first = int(np.nonzero(hist[0].sum(axis=1))[0][0])                        # the first class of branch 0 with a tract
    flank = "01-"
    assert lines[2] == "%s\tleft\t%s\tright\t%s\ttracts\t%d\tsites\t%d" % (
        ("gain", "loss", "mixed")[first // 9], flank[first // 3 % 3], flank[first % 3], hist[0, first].sum(), len_sum[0, first])
    b0 = int(np.nonzero(hist[0, first])[0][0])
    assert lines[3] == "%d\t%d\t%d" % (dr.bin_range(b0) + (hist[0, first, b0],))
    heads = [l for l in lines if l.startswith(("gain", "loss", "mixed"))]
    assert len(heads) == int((hist.sum(axis=2) > 0).sum())                   # a class without a tract has no line
    assert any(l.startswith("mixed\tleft\t-\tright\t-\t") for l in heads)
    assert all(c in "0123456789\t" for l in lines if l and l[0].isdigit() for c in l)   # integers only
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("#samples\t7\tbins\t128\nBRANCH:A\ngain\tleft\t0\tright\t0\ttracts\t1\tsites\t3\n3\t4\t1\n")
    with pytest.raises(RuntimeError, match="range of a bin"):
        host.read_change_tracts(bad)
    open(bad, "w").write("#samples\t7\tbins\t128\nBRANCH:A\ngain\tleft\t0\tright\t0\ttracts\t2\tsites\t3\n3\t3\t1\n")
    with pytest.raises(RuntimeError, match="do not add up"):
        host.read_change_tracts(bad)
    with pytest.raises(ValueError):
        host.write_change_tracts(path, ["a"] * (B + 1), 1, hist, len_sum)


class _Tree:
    n_nodes = 3


def test_summary_helper_on_a_hand_made_example():
    hist, len_sum = np.zeros((2, 27, 128), np.uint64), np.zeros((2, 27), np.uint64)

    def put(b, d, l, r, lengths):
        for ln in lengths:
            hist[b, xr.cls_of(d, l, r), dr.bin_of(ln)] += np.uint64(1)
            len_sum[b, xr.cls_of(d, l, r)] += np.uint64(ln)

    put(0, 0, 0, 0, [3, 5])            # two domains born, 8 sites
    put(0, 0, 1, 1, [2])               # a gap of 2 filled
    put(0, 0, 0, 1, [4, 4, 4, 4])      # grew at the left edge, 16 sites
    put(0, 0, 1, 0, [6])               # grew at the right edge
    put(0, 1, 0, 0, [7])               # died
    put(0, 1, 1, 1, [1, 1])            # split
    put(0, 1, 0, 1, [10])              # shrank at the left edge
    put(0, 1, 1, 0, [2, 2])            # shrank at the right edge
    put(0, 2, 0, 1, [9])               # mixed
    put(0, 2, 1, 1, [3])
    put(0, 0, 2, 0, [5])               # open
    put(0, 2, 2, 2, [40])
    s = host.change_tract_summary(2, hist, len_sum, _Tree())
    want = dict(born=1.0, filled=0.5, grew_left=2.0, grew_right=0.5, died=0.5, split=1.0, shrank_left=0.5,
                shrank_right=1.0, mixed=1.0, open=1.0)
    sizes = dict(born=4.0, filled=2.0, grew_left=4.0, grew_right=6.0, died=7.0, split=1.0, shrank_left=10.0,
                 shrank_right=2.0, mixed=6.0, open=22.5)
    for k, v in want.items():
        assert s[k].shape == (2,) and s[k].dtype == np.float64 and s[k][0] == v and s[k][1] == 0.0, k
        assert s[k + "_size"][0] == sizes[k] and np.isnan(s[k + "_size"][1]), k
    assert s["net_edge_sites"].tolist() == [(16 + 6 - 10 - 4) / 2.0, 0.0]
    with pytest.raises(ValueError):
        host.change_tract_summary(2, hist[:1], len_sum, _Tree())


def _run(*args):
    return subprocess.run([EXE] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_option_errors_come_before_any_device(tmp_path):
    """refused on the options alone (the input files do not even exist): a batch beyond the 2^21 samples the edge
    records take, and -w, which the change tracts have no use for"""
    files = [tmp_path / "p.param", tmp_path / "t.nwk", tmp_path / "in.local_paths"]
    r = _run("-o", tmp_path / "o.paths", "-X", tmp_path / "x.txt", "-B", 2 ** 21 + 1, *files)
    assert r.returncode != 0 and "-X/--tracts" in r.stderr and "2^21" in r.stderr, r.stderr
    r = _run("-o", tmp_path / "o.paths", "-X", tmp_path / "x.txt", "-w", 5, *files)
    assert r.returncode != 0 and "-w/--window belongs to" in r.stderr, r.stderr
    r = _run("-o", tmp_path / "o.paths", "--tracts", tmp_path / "x.txt", "-B", 2 ** 21, *files)   # the option itself is taken
    assert r.returncode != 0 and "-X/--tracts" not in r.stderr and "p.param" in r.stderr, r.stderr
    assert not (tmp_path / "x.txt").exists()


def test_change_tract_symbols_declared():
    from epievo_amd.driver import DRIVER_SYMBOLS
    from epievo_amd.sampler import ABI_SYMBOLS
    for s in ("epv_set_change_tracts", "epv_reset_change_tracts", "epv_accumulate_change_tracts",
              "epv_change_tracts_samples", "epv_change_tracts_layout", "epv_get_change_tracts"):
        assert s in ABI_SYMBOLS
    for s in ("epvd_set_tracts", "epvd_reset_tracts", "epvd_accumulate_tracts", "epvd_tracts_part_sizes",
              "epvd_download_tracts_part", "epvd_download_tracts"):
        assert s in DRIVER_SYMBOLS
    header = open(os.path.join(_build.INCLUDE, "epievo_mi355x.h")).read()
    for s in ABI_SYMBOLS:
        if "change_tracts" in s:
            assert "int %s(" % s in header
    driver = open(os.path.join(_build.INCLUDE, "epievo_mi355x_driver.h")).read()
    for s in DRIVER_SYMBOLS:
        if "tracts" in s:
            assert "int %s(" % s in driver
    L = host.lib()
    for s in ("epvh_tract_parts_merge", "epvh_tract_part_close", "epvh_write_change_tracts", "epvh_read_change_tracts"):
        assert hasattr(L, s)


def test_layer_tables_hold_the_change_tracts_last():
    """the row stands in a fourth table: the three earlier tables and their sum LAYERS stay as recorded"""
    from epievo_amd import summaries
    from epievo_amd.parallel import LocalGroup, ShardedSampler
    from epievo_amd.sampler import DeviceSampler, SingleSiteSampler
    assert summaries.TRACT_SUMMARIES == (summaries.Summary("change_tracts", "a", "change-tract"),)
    assert summaries.CHAIN == summaries.LAYERS + summaries.TRACT_SUMMARIES and len(summaries.CHAIN) == 12
    assert summaries.LAYERS == summaries.SUMMARIES + summaries.DIAGNOSTICS + summaries.LATER_SUMMARIES
    assert summaries.NOUN["change_tracts"] == "change-tract"
    assert summaries.LIFECYCLE[-4:] == ["enable_change_tracts", "reset_change_tracts", "accumulate_change_tracts",
                                        "change_tracts_samples"]
    assert len(summaries.LIFECYCLE) == 4 * 12
    for cls in (DeviceSampler, SingleSiteSampler, ShardedSampler, LocalGroup):
        for name in summaries.LIFECYCLE[-4:] + ["change_tracts_layout", "change_tracts_part", "change_tracts"]:
            assert callable(getattr(cls, name, None)), (cls.__name__, name)
