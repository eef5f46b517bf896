"""Domain maps without a GPU (include/epievo_mi355x.h, epv_set_domain_maps): the numpy yardstick against a plain
per-site walk; the opening of a bit string in libepv_host.so (epvh_domain_map_members) for every size 1 .. 70 and
around 128 and 1024, on runs of L - 1, L and L + 1 sites at bit 0, across the bits 63/64 and at the end of the string;
the two identities of the merge -- merge(parts of the pieces) = part(concatenation), for counts and records alike,
and associativity -- through the C functions (epvh_domain_maps_part, the CPU twin of the kernel, and
epvh_domain_maps_merge) on random rows cut at random points, stretches of exactly E sites, constant and 0101.. rows
and L_K = 1; the refusals; domain_calls and domain_map_windows on hand-made maps; the file round trip; LocalGroup
and ShardedSampler over stand-ins; the table row and the ABI."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import domain_maps_ref as mr
from epievo_amd import host
from test_domain_stats_layers import _Buf, _FakeComm

SIZES = [(1,), (2,), (1, 5, 20), (3, 64, 65), (5, 20, 100, 1000), (1024,), (1, 2)]


def _random_rows(rng, N, n, p_flip=0.1):
    """rows with runs of geometric lengths (mean 1 / p_flip), so that runs on either side of every size occur"""
    flips = rng.random((N, n)) < p_flip
    return (np.cumsum(flips, axis=1) + rng.integers(0, 2, (N, 1))).astype(np.uint8) & 1


# ---- the yardstick itself
def test_yardstick_equals_a_walk_over_the_sites():
    rng = np.random.default_rng(1)
    for sizes in [(1, 2, 3, 7), (2, 5), (4,)]:
        x = _random_rows(rng, 3, 200, 0.25)
        x[0, :9] = 1
        x[1, -7:] = 1
        cnt, counts, edges = mr.part(x, sizes)
        assert cnt == 200 and np.array_equal(counts, mr.walk(x.tolist(), sizes))
        for v in range(3):                         # ... and the host library's opening says the same of every row
            for k, L in enumerate(sizes):
                assert np.array_equal(host.domain_map_members(x[v], L), counts[v, k])
        assert (counts[:, 1:] <= counts[:, :-1]).all()
        if sizes[0] == 1:
            assert np.array_equal(counts[:, 0], x)
    assert np.array_equal(mr.run_lengths([1, 1, 0, 1, 1, 1, 0, 0]), [2, 2, 1, 3, 3, 3, 2, 2])


# ---- the opening in the host library
@pytest.mark.parametrize("L", list(range(1, 71)) + [127, 128, 129, 1023, 1024])
def test_opening_keeps_runs_of_at_least_L(L):
    """runs of L - 1, L and L + 1 ones (a zero on either side where the string allows): at bit 0, across the bits
    63/64, and ending on the last bit of a string whose length is no multiple of 64"""
    for r in (L - 1, L, L + 1):
        if r == 0:
            continue
        n = 64 * ((2 * r + 200) // 64) + 37
        starts = [0, n - r] + ([64 - (r + 1) // 2] if r >= 2 and 64 - (r + 1) // 2 >= 1 else [])
        if r > 64:
            starts.append(1)                        # (a run longer than a word that starts inside the first)
        for st in starts:
            x = np.zeros(n, np.uint8)
            x[st:st + r] = 1
            if 2 <= r and st not in (0, n - r):
                assert st <= 63 < 64 <= st + r - 1 or r > 64        # the run holds bits 63 and 64
            got = host.domain_map_members(x, L)
            want = x if r >= L else np.zeros(n, np.uint8)
            assert np.array_equal(got, want), (L, r, st)
            assert np.array_equal(got, mr.members(x, L))
    # two runs a single zero apart do not help each other; all ones; the empty string; a string shorter than L
    x = np.ones(3 * L + 1, np.uint8)
    assert np.array_equal(host.domain_map_members(x, L), x)
    if L >= 2:
        x[L - 1] = 0
        want = x.copy()
        want[:L - 1] = 0
        assert np.array_equal(host.domain_map_members(x, L), want)
        assert not host.domain_map_members(np.ones(L - 1, np.uint8), L).any()
    assert host.domain_map_members(np.zeros(0, np.uint8), L).shape == (0,)


def test_opening_on_random_strings():
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 700):
        for p in (0.02, 0.3):
            x = _random_rows(rng, 1, n, p)[0]
            for L in (1, 2, 3, 9, 64, 65, 200):
                assert np.array_equal(host.domain_map_members(x, L), mr.members(x, L)), (n, p, L)
    with pytest.raises(RuntimeError, match="at least 1"):
        host.domain_map_members(np.ones(4, np.uint8), 0)


# ---- the CPU twin of the kernel, and the merge
def _assert_part(got, want):
    assert got[0] == want[0]
    assert got[1].dtype == np.uint32 and got[2].dtype == np.uint64
    assert got[1].shape == want[1].shape and got[2].shape == want[2].shape
    assert np.array_equal(got[2], want[2])          # every word of every record
    assert np.array_equal(got[1], want[1])


@pytest.mark.parametrize("sizes", SIZES, ids=str)
def test_twin_equals_the_yardstick(sizes):
    rng = np.random.default_rng(sum(sizes))
    E = mr.edge_bits(sizes)
    for n in (max(E, 1), E + 1, E + 64, 2 * E + 333):
        x = _random_rows(rng, 3, n, 1.5 / (sizes[-1] + 1.0))
        x[1] = 1
        x[2] = np.arange(n) & 1
        got = host.domain_maps_part(x, sizes)
        _assert_part(got, mr.part(x, sizes))
        if E % 64:
            assert not (got[2][..., -1] >> np.uint64(E % 64)).any()         # the spare bits of the last word
        assert got[2].shape == (1, 3, 2, (E + 63) // 64)
        assert (got[1][1] == (1 if n >= sizes[-1] else 0)).all() or n < sizes[-1]
        assert not got[1][2, np.array(sizes) > 1].any()                      # 0101..: no run of two


def _sum_parts(xs, a, b, sizes, f):
    p = f(xs[0][:, a:b], sizes)
    for x in xs[1:]:
        p = mr.add_parts(p, f(x[:, a:b], sizes))
    return p


@pytest.mark.parametrize("sizes", SIZES, ids=str)
def test_merge_of_the_pieces_is_the_part_of_the_whole_and_merging_is_associative(sizes):
    rng = np.random.default_rng(100 + sum(sizes))
    E = mr.edge_bits(sizes)
    n = 6 * max(E, 8) + 77
    xs = [_random_rows(rng, 4, n, 1.5 / (sizes[-1] + 1.0)) for _ in range(2)]      # two samples
    xs[0][2], xs[1][2] = 1, 0                                                      # constant rows
    xs[0][3] = xs[1][3] = np.arange(n) & 1                                         # 0101..
    whole = _sum_parts(xs, 0, n, sizes, host.domain_maps_part)
    _assert_part(whole, _sum_parts(xs, 0, n, sizes, mr.part))
    cut_sets = [[E], [n - E], [E, 2 * E], [E, 2 * E, 3 * E]]                       # stretches of exactly E sites
    for _ in range(4):                                                             # random cuts, each piece >= E
        k = int(rng.integers(1, 4))
        while True:
            cuts = sorted(int(c) for c in rng.integers(E, n - E + 1, k))
            if all(b - a >= max(E, 1) for a, b in zip([0] + cuts, cuts + [n])):
                break
        cut_sets.append(cuts)
    for cuts in cut_sets:
        if any(b - a < 1 for a, b in zip([0] + cuts, cuts + [n])):
            continue
        bounds = [0] + cuts + [n]
        pieces = [_sum_parts(xs, a, b, sizes, host.domain_maps_part) for a, b in zip(bounds[:-1], bounds[1:])]
        merged = host.domain_maps_merge(sizes, pieces)
        _assert_part(merged, whole)
        _assert_part(mr.merge(sizes, pieces), whole)                               # the yardstick's own merge
        if len(pieces) >= 3:
            left = host.domain_maps_merge(sizes, [host.domain_maps_merge(sizes, pieces[:2])] + pieces[2:])
            right = host.domain_maps_merge(sizes, pieces[:1] + [host.domain_maps_merge(sizes, pieces[1:])])
            _assert_part(left, whole)
            _assert_part(right, whole)
    # what the merge adds is real: a run across a cut that neither piece could see
    if sizes[-1] >= 2:
        L = sizes[-1]
        x = np.zeros((1, 2 * max(E, 2) + 10), np.uint8)
        c = x.shape[1] // 2
        x[0, c - (L // 2):c - (L // 2) + L] = 1
        a, b = host.domain_maps_part(x[:, :c], sizes), host.domain_maps_part(x[:, c:], sizes)
        assert not a[1][0, -1].any() and not b[1][0, -1].any()
        assert int(host.domain_maps_merge(sizes, [a, b])[1][0, -1].sum()) == L


def test_refusals():
    for bad in [(5, 5), (5, 3), (0,), (0, 4), (1025,), (1, 2, 3, 4, 5), ()]:
        with pytest.raises(ValueError):
            host.domain_map_sizes(bad)
        with pytest.raises(ValueError):
            host.domain_maps_part(np.zeros((1, 4000), np.uint8), bad)
    L = host.lib()
    import ctypes as C
    one32, one64 = np.zeros(4096, np.uint32), np.zeros(64, np.uint64)
    for bad in [(5, 5), (5, 3), (0,), (1025,), (1, 2, 3, 4, 5)]:
        z = np.array(bad, np.uint32)
        assert L.epvh_domain_maps_part(1, len(z), host._p(z, C.c_uint32), 4000, host._p(one64, C.c_uint64),
                                       host._p(one32, C.c_uint32), host._p(one64, C.c_uint64)) != 0
        assert L.epvh_last_error()
    with pytest.raises(RuntimeError, match="fewer than the 38"):
        host.domain_maps_part(np.zeros((1, 37), np.uint8), (20,))
    a = host.domain_maps_part(np.zeros((1, 38), np.uint8), (20,))
    short = (37, a[1][:, :, :37], a[2])
    with pytest.raises(RuntimeError, match="part 1 holds 37 sites"):
        host.domain_maps_merge((20,), [a, short])
    with pytest.raises(ValueError):
        host.domain_maps_merge((20,), [a, (38, a[1], a[2][:, :, :, :0])])
    with pytest.raises(ValueError):
        host.domain_maps_merge((20,), [])


# ---- what a user reads off the maps
def test_windows_on_a_hand_made_map():
    maps = np.arange(2 * 2 * 7, dtype=np.uint32).reshape(2, 2, 7)
    w = host.domain_map_windows(maps, 3)
    assert w.dtype == np.uint64 and w.shape == (2, 2, 3)
    assert w[0, 0].tolist() == [0 + 1 + 2, 3 + 4 + 5, 6] and w[1, 1].tolist() == [21 + 22 + 23, 24 + 25 + 26, 27]
    assert np.array_equal(host.domain_map_windows(maps, 1), maps) and host.domain_map_windows(maps, 100).shape == (2, 2, 1)
    assert int(host.domain_map_windows(np.full((1, 1, 5), 2 ** 32 - 1, np.uint32), 5)[0, 0, 0]) == 5 * (2 ** 32 - 1)
    with pytest.raises(ValueError):
        host.domain_map_windows(maps, 0)
    with pytest.raises(ValueError):
        host.domain_map_windows(maps.astype(np.float64), 2)


def test_calls_on_a_hand_made_map():
    samples = 10
    maps = np.zeros((2, 2, 12), np.uint32)
    maps[0, 1] = [0, 5, 9, 10, 4, 5, 5, 0, 10, 10, 10, 10]
    maps[1, 1, :] = 10
    calls = host.domain_calls(samples, maps, 1, support=0.5, min_sites=1)
    assert calls[0] == [(1, 3, 24.0 / 30.0), (5, 6, 0.5), (8, 11, 1.0)] and calls[1] == [(0, 11, 1.0)]
    assert host.domain_calls(samples, maps, 1, support=0.5, min_sites=3)[0] == [(1, 3, 0.8), (8, 11, 1.0)]
    assert host.domain_calls(samples, maps, 1, support=0.9)[0] == [(2, 3, 0.95), (8, 11, 1.0)]
    assert host.domain_calls(samples, maps, 0) == [[], []]
    # thresholding the marginal and taking runs is not this: a site near one half in the middle splits nothing here
    with pytest.raises(ValueError):
        host.domain_calls(0, maps, 1)
    with pytest.raises(ValueError):
        host.domain_calls(samples, maps, 1, support=0.0)


def test_file_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    names = ["R", "U", "A", "B"]
    sizes, n, W = (5, 20), 1003, 100
    sums = rng.integers(0, 2 ** 40, (4, 2, 11), dtype=np.uint64)
    path = str(tmp_path / "maps.txt")
    host.write_domain_maps(path, names, 50, 0, sizes, n, W, sums)
    text = open(path).read().split("\n")
    assert text[0] == "#samples\t50\tstate\t0\tsizes\t5\t20" and text[1] == "#window\t100\tsites\t1003"
    assert text[2] == "NODE:R" and text[3] == "%d\t%d" % (sums[0, 0, 0], sums[0, 1, 0]) and text[14] == "NODE:U"
    body = [l for l in text[2:] if l and not l.startswith("NODE:")]
    assert len(body) == 44 and all(f.isdigit() for l in body for f in l.split("\t"))       # integers only
    back = host.read_domain_maps(path)
    assert (back["samples"], back["sites"], back["window"], back["state"]) == (50, n, W, 0)
    assert back["sizes"].tolist() == [5, 20] and back["node_names"] == names and np.array_equal(back["sums"], sums)
    with pytest.raises(ValueError):
        host.write_domain_maps(path, names, 50, 0, sizes, n, W, sums[:, :, :10])
    for cut in (1, 20, len(text) - 3):
        open(path, "w").write("\n".join(text[:cut]) + "\n")
        with pytest.raises(RuntimeError):
            host.read_domain_maps(path)
    with pytest.raises(RuntimeError):
        host.read_domain_maps(str(tmp_path / "missing.txt"))


# ---- the layers above the device, over stand-ins
class _Shard:
    """a shard (or a rank's device) that holds a part"""

    def __init__(self, sizes, state, ns, part, first=0):
        self.sizes, self.state, self.ns, self.part, self.first, self.calls = tuple(sizes), state, ns, part, first, []

    def domain_maps_layout(self):
        return (self.part[1].shape[0], self.sizes, self.state, self.first, self.part[0], 16384)

    def domain_maps_part(self):
        return (self.ns,) + tuple(self.part)

    def domain_maps_samples(self):
        return self.ns

    def enable_domain_maps(self, *args):
        self.calls.append(("enable_domain_maps",) + args)

    def reset_domain_maps(self):
        self.calls.append(("reset_domain_maps",))

    def accumulate_domain_maps(self):
        self.calls.append(("accumulate_domain_maps",))

    def alloc(self, nbytes):
        return _Buf(nbytes)

    def write(self, buf, offset, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf.data[offset:offset + raw.size] = raw

    def read(self, buf, offset, count, dtype=np.float64):
        return buf.data[offset:offset + count * np.dtype(dtype).itemsize].view(dtype).copy()


@pytest.fixture(scope="module")
def three():
    """three samples of random rows over 700 sites, cut 38 / 400 / 262 with sizes (1, 5, 20): the first stretch holds
    exactly E = 38 sites"""
    rng = np.random.default_rng(11)
    sizes, n, cuts = (1, 5, 20), 700, [0, 38, 438, 700]
    xs = [_random_rows(rng, 3, n, 0.08) for _ in range(3)]
    xs[1][1, 20:600] = 1                                   # a run that spans a whole stretch
    parts = [_sum_parts(xs, a, b, sizes, mr.part) for a, b in zip(cuts[:-1], cuts[1:])]
    return sizes, n, cuts, parts, _sum_parts(xs, 0, n, sizes, mr.part)


def test_local_group_merges_its_shards(three):
    from epievo_amd.parallel import LocalGroup
    sizes, n, cuts, parts, whole = three
    g = object.__new__(LocalGroup)
    g.subs = [_Shard(sizes, 1, 3, p, first=(0 if i == 0 else 256)) for i, p in enumerate(parts)]
    g.pool, g.halo_mode, g._closed = ThreadPoolExecutor(max_workers=3), False, True
    try:
        assert g.domain_maps_layout() == (3, sizes, 1, 0, n, 16384)
        got = g.domain_maps_part()
        assert got[0] == 3
        _assert_part(got[1:], whole)
        ns, maps = g.domain_maps(counts=True)
        assert ns == 3 and maps.dtype == np.uint32 and np.array_equal(maps, whole[1])
        ns, maps = g.domain_maps()
        assert maps.dtype == np.float64 and np.array_equal(maps, whole[1] / 3.0)
        assert sum(int(p[1].sum()) for p in parts) < int(whole[1].sum())           # the merge adds what the cuts hid
        assert g.domain_maps_samples() == 3
        g.enable_domain_maps(sizes, 0, 7)
        g.reset_domain_maps()
        assert all(s.calls == [("enable_domain_maps", sizes, 0, 7), ("reset_domain_maps",)] for s in g.subs)
        assert g._dmaps_on
        with pytest.raises(RuntimeError, match="reset\\(\\) the group before taking a domain-map sample"):
            g.accumulate_domain_maps()
        g.halo_mode = True
        g.accumulate_domain_maps()
        assert all(s.calls[-1] == ("accumulate_domain_maps",) for s in g.subs)
        g.subs[1].ns = 2
        with pytest.raises(RuntimeError, match="different numbers of domain-map samples"):
            g.domain_maps_part()
    finally:
        g.pool.shutdown(wait=True)


def test_sharded_sampler_merges_the_ranks(three):
    from epievo_amd.parallel import ShardedSampler
    sizes, n, cuts, parts, whole = three
    pieces, ranks = {}, []
    for r in range(3):
        s = object.__new__(ShardedSampler)
        s.comm, s.cuts, s.dev = _FakeComm(3, r, pieces), cuts, _Shard(sizes, 1, 3, parts[r])
        ranks.append(s)
    for _ in range(2):                     # (the ranks run one after the other here: two rounds fill both collectives)
        for s in ranks:
            try:
                s.domain_maps_part()
            except (RuntimeError, ValueError):
                pass
    for s in ranks:
        got = s.domain_maps_part()
        assert got[0] == 3
        _assert_part(got[1:], whole)
        assert np.array_equal(s.domain_maps(counts=True)[1], whole[1])
    ranks[2].dev.ns = 2
    ranks[2].dev.part = (parts[2][0], parts[2][1], parts[2][2][:2])
    with pytest.raises(RuntimeError, match="different numbers of domain-map samples"):
        ranks[2].domain_maps_part()
    one = object.__new__(ShardedSampler)
    one.comm, one.cuts, one.dev = _FakeComm(1, 0, {}), [0, n], _Shard(sizes, 1, 3, whole)
    _assert_part(one.domain_maps_part()[1:], whole)
    assert not one.comm.pieces


def test_table_row_abi_and_surface():
    from epievo_amd import sampler, summaries
    from epievo_amd.parallel import LocalGroup, ShardedSampler
    assert [(s.stem, s.article, s.noun) for s in summaries.LATER_SUMMARIES] == [("domain_maps", "a", "domain-map")]
    assert summaries.LAYERS == summaries.SUMMARIES + summaries.DIAGNOSTICS + summaries.LATER_SUMMARIES
    assert summaries.NOUN["domain_maps"] == "domain-map"
    names = ["enable_domain_maps", "reset_domain_maps", "accumulate_domain_maps", "domain_maps_samples"]
    assert all(m in summaries.LIFECYCLE for m in names)
    for cls in (sampler.DeviceSampler, sampler.SingleSiteSampler, ShardedSampler, LocalGroup):
        for m in names + ["domain_maps_layout", "domain_maps_part", "domain_maps"]:
            assert callable(getattr(cls, m, None)), (cls.__name__, m)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "epievo_mi355x.h")).read()
    for s in ("epv_set_domain_maps", "epv_reset_domain_maps", "epv_accumulate_domain_maps", "epv_domain_maps_samples",
              "epv_domain_maps_layout", "epv_get_domain_maps"):
        assert s in sampler.ABI_SYMBOLS and ("int %s(" % s) in header
    L = host.lib()
    for s in ("epvh_domain_map_members", "epvh_domain_maps_part", "epvh_domain_maps_merge", "epvh_write_domain_maps",
              "epvh_read_domain_maps"):
        assert hasattr(L, s)
