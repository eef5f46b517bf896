"""Change tracts, the layers above the device that need no GPU: LocalGroup over stand-ins for its shards -- the
lifecycle reaches every shard, the shards' parts are merged in genome order and closed -- and ShardedSampler's
read-out over stand-ins for the device and the collective -- the ranks' parts all-gathered, the sample counts
compared, every rank merging and closing; and that every engine has every method the layers call."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import tracts_ref as xr
from common import simulate
from epievo_amd import host

STEM = "change_tracts"
ASKED = ["enable_" + STEM, "reset_" + STEM, "accumulate_" + STEM, STEM + "_samples", STEM + "_layout", STEM + "_part", STEM]


class _Buf:
    def __init__(self, nbytes):
        self.data = np.zeros(nbytes, np.uint8)

    def free(self):
        pass


class _FakeDev:
    """what ShardedSampler and LocalGroup ask of a device: its part, its layout, the lifecycle, host-side buffers"""

    def __init__(self, ns, part, first=0, count=0):
        self.ns, self.part, self.first, self.count, self.calls = ns, part, first, count, []

    def change_tracts_part(self):
        return (self.ns,) + tuple(self.part)

    def change_tracts_samples(self):
        return self.ns

    def change_tracts_layout(self):
        return (self.part[0].shape[0], 27, 128, self.first, self.count, 65536)

    def enable_change_tracts(self, max_samples):
        self.calls.append(("enable", max_samples))

    def reset_change_tracts(self):
        self.calls.append(("reset",))

    def accumulate_change_tracts(self):
        self.calls.append(("accumulate",))

    def alloc(self, nbytes):
        return _Buf(nbytes)

    def write(self, buf, offset, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf.data[offset:offset + raw.size] = raw

    def read(self, buf, offset, count, dtype=np.float64):
        return buf.data[offset:offset + count * np.dtype(dtype).itemsize].view(dtype).copy()


class _FakeComm:
    """an all-gather among ranks that run one after the other: pieces are remembered by rank"""

    def __init__(self, world, rank, pieces):
        self.world, self.rank, self.pieces = world, rank, pieces

    def all_gather(self, dev, piece, gathered):
        k = piece.data.size
        self.pieces[(self.rank, k)] = piece.data.copy()        # (a read-out is two collectives of different sizes)
        for (r, size), p in self.pieces.items():
            if size == k:
                gathered.data[r * k:(r + 1) * k] = p


def test_every_layer_has_the_methods():
    from epievo_amd.driver import CppSampler
    from epievo_amd.parallel import LocalGroup, ShardedSampler
    from epievo_amd.sampler import DeviceSampler, SingleSiteSampler
    assert sorted(m for m in vars(ShardedSampler) if STEM in m) == sorted(ASKED)
    for engine in (DeviceSampler, LocalGroup, SingleSiteSampler, ShardedSampler):
        missing = [m for m in ASKED if not callable(getattr(engine, m, None))]
        assert not missing, (engine.__name__, missing)
    for m in ("enable_" + STEM, "reset_" + STEM, "accumulate_" + STEM, STEM + "_part", STEM):
        assert callable(getattr(CppSampler, m, None)), m


N, NS, CUTS = 3000, 3, [0, 1024, 2304, 3000]


@pytest.fixture(scope="module")
def rows():
    xs = [xr.rows(simulate("tree", N, seed=9 + i)[2]) for i in range(NS)]
    xs[1][2, 1000:2400] = 0                        # branch 1: a gained tract that spans a whole stretch, but for the one
    xs[1][3, 1000:2400] = 1                        # lost site 2350, between an unchanged 0 at 999 and an unchanged 1 at 2400
    xs[1][2, 2350] = 1
    xs[1][3, 2350] = 0
    xs[1][2:4, 999] = 0
    xs[1][2:4, 2400] = 1
    return xs


def _part_of(xs, a, b):
    p = xr.part(xs[0][:, a:b])
    for x in xs[1:]:
        p = xr.add_parts(p, xr.part(x[:, a:b]))
    return p


@pytest.fixture()
def ranks(rows):
    from epievo_amd.parallel import ShardedSampler
    pieces, out = {}, []
    for r in range(3):
        s = object.__new__(ShardedSampler)
        s.comm, s.cuts = _FakeComm(3, r, pieces), CUTS
        s.dev = _FakeDev(NS, _part_of(rows, CUTS[r], CUTS[r + 1]))
        out.append(s)
    return out, _part_of(rows, 0, N)


def _fill(shards):
    """every rank leaves its pieces of both collectives (the ranks run one after the other here, so it takes two
    rounds)"""
    for _ in range(2):
        for s in shards:
            try:
                s.change_tracts_part()
            except RuntimeError:
                pass


def _check_long_tract(closed):
    k = xr.cls_of(2, 0, 1)                          # mixed, flanks 0 | 1, 1400 sites: no stretch could close it
    assert closed[0][1, k, xr.bin_of(1400)] >= 1 and closed[1][1, k] >= 1400


def test_sharded_read_out_merges_in_genome_order(ranks, rows):
    shards, full = ranks
    mid = shards[1].dev.part[2][1, 1]
    assert (mid & np.uint64(xr.WHOLE)).all() and ((mid >> np.uint64(xr.LOSS_SHIFT)) & np.uint64(1) == 0).all()   # whole, gains only
    _fill(shards)
    closed = xr.close(*full)
    changed = sum((x[0::2] ^ x[1::2]).sum(axis=1, dtype=np.uint64) for x in rows)
    for s in shards:
        got = s.change_tracts_part()
        assert got[0] == NS and all(g.dtype == np.uint64 for g in got[1:])
        assert all(np.array_equal(g, w) for g, w in zip(got[1:], full))
        got = s.change_tracts()
        assert got[0] == NS and np.array_equal(got[1], closed[0]) and np.array_equal(got[2], closed[1])
        assert np.array_equal(got[2].sum(axis=1), changed)
    _check_long_tract(closed)
    assert not np.array_equal(shards[0].dev.part[0], full[0])   # a rank alone is not the genome


def test_sharded_sample_counts_must_agree(ranks):
    shards, full = ranks
    _fill(shards)
    shards[1].dev.ns = NS - 1
    keep = shards[1].dev.part
    shards[1].dev.part = (keep[0], keep[1], keep[2][:NS - 1])
    for s in (shards[1], shards[0]):
        with pytest.raises(RuntimeError) as e:
            s.change_tracts()
        assert str(e.value) == "the ranks hold different numbers of change-tract samples"
    shards[1].dev.ns, shards[1].dev.part = NS, keep
    _fill(shards)
    assert np.array_equal(shards[0].change_tracts_part()[1], full[0])


def test_one_rank_needs_no_collective(rows):
    from epievo_amd.parallel import ShardedSampler
    p = xr.part(rows[0][:, :500])
    s = object.__new__(ShardedSampler)
    s.comm, s.cuts, s.dev = _FakeComm(1, 0, {}), [0, 500], _FakeDev(1, p)
    got = s.change_tracts()
    want = xr.close(*p)
    assert got[0] == 1 and np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1])
    assert not s.comm.pieces


@pytest.fixture()
def group(rows):
    from epievo_amd.parallel import LocalGroup
    g = object.__new__(LocalGroup)
    g.subs = [_FakeDev(NS, _part_of(rows, a, b), first=1 if a else 0, count=b - a) for a, b in zip(CUTS[:-1], CUTS[1:])]
    g.pool, g.halo_mode, g._closed = ThreadPoolExecutor(max_workers=3), False, True
    yield g
    g.pool.shutdown(wait=True)


def test_group_lifecycle_and_read_out(group, rows):
    assert group.enable_change_tracts(5) is None and group.reset_change_tracts() is None
    assert all(s.calls == [("enable", 5), ("reset",)] for s in group.subs)
    with pytest.raises(RuntimeError) as e:           # before the first reset() of the group the shards' ranges overlap
        group.accumulate_change_tracts()
    assert str(e.value) == "reset() the group before taking a change-tract sample"
    group.halo_mode = True
    assert group.accumulate_change_tracts() is None and all(s.calls[-1] == ("accumulate",) for s in group.subs)
    assert group.change_tracts_samples() == NS
    assert group.change_tracts_layout() == (4, 27, 128, 0, N, 65536)
    full = _part_of(rows, 0, N)
    got = group.change_tracts_part()
    assert got[0] == NS and all(np.array_equal(g, w) and g.dtype == np.uint64 for g, w in zip(got[1:], full))
    assert all(np.array_equal(g, w) for g, w in zip(got[1:], host.tract_parts_merge([s.part for s in group.subs])))
    closed = xr.close(*full)
    got = group.change_tracts()
    assert got[0] == NS and np.array_equal(got[1], closed[0]) and np.array_equal(got[2], closed[1])
    _check_long_tract(closed)
    group.subs[1].ns = NS + 1
    with pytest.raises(RuntimeError) as e:
        group.change_tracts()
    assert str(e.value) == "the shards of the group hold different numbers of change-tract samples"
