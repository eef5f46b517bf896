"""Domain size spectra, the parts that need no GPU: the bins of libepv_host.so against the plain Python
definition, the numpy yardstick (tests/domains_ref.py) against a per-site walk, the three identities of parts
through the C functions (merge of the pieces = part of the whole, merging is associative, a closed part holds
every site once), the invariants of a result, and the file of epievo_est_histories -d through its writer and
reader.  The device side is in test_domain_stats_gpu.py."""
import numpy as np
import pytest

import domains_ref as dr
import orc
from common import simulate
from epievo_amd import host


def test_bins_equal_the_python_definition():
    L = host.lib()
    assert host.DOMAIN_BINS == dr.BINS == 128
    got = np.fromiter((L.epvh_domain_bin(l) for l in range(2 ** 20 + 1)), np.int64, 2 ** 20 + 1)
    want = np.fromiter((dr.bin_of(l) for l in range(2 ** 20 + 1)), np.int64, 2 ** 20 + 1)
    assert np.array_equal(got, want)
    assert np.array_equal(dr.bins_of(np.arange(2 ** 20 + 1)), want)          # the yardstick's vector form
    edge = set()
    for k in range(1, 32):
        edge.update((2 ** k - 1, 2 ** k, 2 ** k + 1))
        for q in range(1, 4):                                                # the quarter-octave edges
            e = 2 ** k + q * 2 ** k // 4
            edge.update((e - 1, e, e + 1))
    edge.update((2 ** 32 - 2, 2 ** 32 - 1))
    for l in sorted(edge):
        assert host.domain_bin(l) == dr.bin_of(l), l
    assert dr.bin_of(15) == 15 and dr.bin_of(16) == 16 and dr.bin_of(19) == 16 and dr.bin_of(20) == 17
    assert dr.bin_of(2 ** 32 - 1) == 127 and host.domain_bin(2 ** 32 - 1) == 127


def test_bin_ranges_tile_the_lengths():
    edges = host.domain_bin_edges()
    assert edges.dtype == np.uint64 and edges.shape == (128, 2) and edges[0].tolist() == [0, 0]
    at = 1
    for b in range(1, 128):
        lo, hi = host.domain_bin_range(b)
        assert (lo, hi) == dr.bin_range(b) == tuple(int(x) for x in edges[b])
        assert lo == at and hi >= lo                                         # no gap, no overlap
        assert host.domain_bin(lo) == b and host.domain_bin(hi) == b
        at = hi + 1
    assert at == 2 ** 32


@pytest.fixture(scope="module", params=[("tree", 257), ("bal16", 300)], ids=["tree257", "bal16x300"])
def one(request):
    cfg, n = request.param
    model, tree, fp = simulate(cfg, n, seed=6)
    return model, tree, fp, dr.node_states(fp, tree)


def test_yardstick_equals_a_per_site_walk(one):
    model, tree, fp, x = one
    N, n = tree.n_nodes, fp.n_sites
    assert x.shape == (N, n)
    # the node states by hand: flip the init state once per jump
    off = fp.offsets.astype(np.int64)
    for v in range(1, N):
        for s in range(n):
            st = int(fp.init[(v - 1) * n + s])
            for _ in range(int(off[(v - 1) * n + s + 1] - off[(v - 1) * n + s])):
                st ^= 1
            assert x[v, s] == st
    child0 = list(tree.parent_ids[1:]).index(0) + 1
    assert np.array_equal(x[0], fp.init.reshape(N - 1, n)[child0 - 1])
    hist, len_sum = dr.close(*dr.part(x))
    wh, wl = dr.walk(x)
    assert np.array_equal(hist, wh) and np.array_equal(len_sum, wl)
    assert (len_sum.sum(axis=1) == n).all() and not hist[:, :, 0].any()
    assert hist.sum() > 4 * N                                                # not vacuous: many runs per node


def _random_rows(rng, N, n):
    """rows of very different run lengths: coin flips, long runs, constant rows"""
    x = np.zeros((N, n), np.uint8)
    for v in range(N):
        kind = rng.integers(0, 4)
        if kind == 0:
            x[v] = rng.integers(0, 2, n)
        elif kind == 1:
            x[v] = np.cumsum(rng.random(n) < 0.05) & 1
        elif kind == 2:
            x[v] = rng.integers(0, 2)
        else:
            x[v] = (np.cumsum(rng.random(n) < 0.3) + rng.integers(0, 2)) & 1
    return x


def _pieces(rng, n):
    """cut points of 1-6 stretches of [0, n), empty and one-site stretches included"""
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


def test_merge_and_close_identities_through_the_c_functions():
    rng = np.random.default_rng(5)
    whole_parts = empty_parts = 0
    for trial in range(300):
        N, n, ns = int(rng.integers(1, 4)), int(rng.integers(1, 201)), int(rng.integers(1, 4))
        xs = [_random_rows(rng, N, n) for _ in range(ns)]
        cuts = _pieces(rng, n)
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            p = dr.part(xs[0][:, a:b])
            for x in xs[1:]:
                p = dr.add_parts(p, dr.part(x[:, a:b]))
            parts.append(p)
            whole_parts += int(b > a and (p[2][:, :, 0] & np.uint64(dr.WHOLE)).any())
            empty_parts += int(b == a)
        full = dr.part(xs[0])
        for x in xs[1:]:
            full = dr.add_parts(full, dr.part(x))
        # 1. merge(parts of the pieces) = part(concatenation), by the yardstick and by the C function
        assert _same(dr.merge(parts), full)
        got = host.domain_parts_merge(parts)
        assert all(g.dtype == np.uint64 for g in got) and _same(got, full)
        # 2. associative: any split into two groups merged first
        if len(parts) >= 2:
            j = int(rng.integers(1, len(parts)))
            left, right = host.domain_parts_merge(parts[:j]), host.domain_parts_merge(parts[j:])
            assert _same(host.domain_parts_merge([left, right]), full)
        # 3. closing: every site once; the C function equals the yardstick and the walk
        hist, len_sum = host.domain_part_close(*got)
        assert _same((hist, len_sum), dr.close(*full))
        assert (len_sum.sum(axis=1) == ns * n).all()
        wh = sum(dr.walk(x)[0] for x in xs)
        assert np.array_equal(hist, wh)
        assert _same(got, full)                                              # close works on copies
    assert whole_parts > 50 and empty_parts > 20                             # the cases were met


def test_single_records():
    """a part of one site, a whole part between two others of its state, and of the other state"""
    one_site = dr.part(np.array([[1]], np.uint8))
    assert int(one_site[2][0, 0, 0]) == dr.record(1, 1, True) == int(one_site[2][0, 0, 1])
    a, b, c = (dr.part(np.array([r], np.uint8)) for r in ([0, 1, 1], [1, 1], [1, 0, 0, 1]))
    hist, len_sum, edges = host.domain_parts_merge([a, b, c])
    assert [int(e) for e in edges[0, 0]] == [dr.record(1, 0), dr.record(1, 1)]
    assert hist[0, 1, 5] == 1 and hist[0, 0, 2] == 1 and hist.sum() == 2 and len_sum.tolist() == [[2, 5]]
    b0 = dr.part(np.array([[0, 0]], np.uint8))
    hist, len_sum, edges = host.domain_parts_merge([a, b0, c])
    assert hist[0, 1, 2] == 1 and hist[0, 0, 2] == 2 and hist[0, 1, 1] == 1 and hist.sum() == 4
    with pytest.raises(ValueError):
        host.domain_parts_merge([])
    with pytest.raises(ValueError):
        host.domain_parts_merge([a, (a[0], a[1], np.zeros((2, 1, 2), np.uint64))])


def test_invariants_over_sampled_histories(one):
    """over the oracle's sweeps: the lengths add up to samples x sites, the bins to the runs, and an observed
    leaf's spectrum is samples x the spectrum of its data"""
    model, tree, fp, x0 = one
    N, n, ns = tree.n_nodes, fp.n_sites, 3
    o = orc.Oracle(tree, model, fp, "B", cap=int(max(16, 2 * fp.counts().max() + 8)), seed=77)
    o.reset()
    total, runs, per_sample = None, 0, []
    for w in range(ns):
        o.sweep(5 + w)
        x = dr.node_states(o.paths(), tree)
        p = dr.part(x)
        per_sample.append(dr.close(*p)[0])
        total = p if total is None else dr.add_parts(total, p)
        runs += int((x[:, :-1] != x[:, 1:]).sum()) + N
    hist, len_sum = host.domain_part_close(*total)
    assert (len_sum.sum(axis=1) == ns * n).all()
    assert int(hist.sum()) == runs
    data_hist, data_len = dr.walk(x0)
    leaves = [v for v in range(1, N) if tree.subtree_sizes[v] == 1]
    for v in leaves:
        assert np.array_equal(hist[v], data_hist[v] * np.uint64(ns)) and np.array_equal(len_sum[v], data_len[v] * np.uint64(ns))
    internal = [v for v in range(1, N) if v not in leaves]
    assert any(not np.array_equal(per_sample[0][v], per_sample[1][v]) for v in internal)   # the ancestors move
    assert all(np.array_equal(per_sample[0][0], h[0]) for h in per_sample)                 # the root is not resampled
    per_run, mean_len = host.domain_summary(ns, hist, len_sum)
    assert np.array_equal(per_run, hist.sum(axis=2) / float(ns))
    assert np.allclose((per_run * mean_len).sum(axis=1), n)


def test_file_round_trip(one, tmp_path):
    model, tree, fp, x = one
    hist, len_sum = dr.close(*dr.part(x))
    hist[1, 1, 127] += np.uint64(2 ** 40)                                    # the last bin, a count beyond 32 bits
    path = str(tmp_path / "domains.txt")
    host.write_domain_stats(path, list(tree.node_names), 7, hist, len_sum)
    got = host.read_domain_stats(path)
    assert got["samples"] == 7 and got["node_names"] == list(tree.node_names)
    assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], hist) and np.array_equal(got["len_sum"], len_sum)
    lines = open(path).read().split("\n")
    assert lines[0] == "#samples\t7\tbins\t128" and lines[1] == "NODE:" + tree.node_names[0]
    assert lines[2] == "state\t0\truns\t%d\tsites\t%d" % (hist[0, 0].sum(), len_sum[0, 0])
    lo, hi = dr.bin_range(int(np.nonzero(hist[0, 0])[0][0]))
    assert lines[3] == "%d\t%d\t%d" % (lo, hi, hist[0, 0][np.nonzero(hist[0, 0])[0][0]])
    assert all(c in "0123456789\t" for l in lines if l and l[0].isdigit() for c in l)   # integers only
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("#samples\t7\tbins\t128\nNODE:R\nstate\t0\truns\t1\tsites\t3\n3\t4\t1\n")
    with pytest.raises(RuntimeError, match="range of a bin"):
        host.read_domain_stats(bad)
    with pytest.raises(ValueError):
        host.write_domain_stats(path, ["a"], 1, hist, len_sum)
