"""Spatial correlations, the layers above the device that need no GPU: ShardedSampler's read-out over stand-ins for
the device and the collective -- the ranks' parts all-gathered, the sample counts compared, every rank merging in
genome order and closing -- and that every engine has every method the layers call."""
import numpy as np
import pytest

import corr_ref as cr
from common import config, simulate

L = 130


class _Buf:
    def __init__(self, nbytes):
        self.data = np.zeros(nbytes, np.uint8)

    def free(self):
        pass


class _FakeDev:
    """what ShardedSampler asks of its device: this rank's part, and host-side buffers"""

    def __init__(self, ns, part):
        self.ns, self.part = ns, part

    def spatial_correlation_part(self):
        return (self.ns,) + tuple(self.part)

    def spatial_correlation_samples(self):
        return self.ns

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
    asked = ["enable_spatial_correlation", "reset_spatial_correlation", "accumulate_spatial_correlation",
             "spatial_correlation_samples", "spatial_correlation_layout", "spatial_correlation_part",
             "spatial_correlation"]
    assert sorted(m for m in vars(ShardedSampler) if "spatial_correlation" in m) == sorted(asked)
    for engine in (DeviceSampler, LocalGroup, SingleSiteSampler, ShardedSampler):
        missing = [m for m in asked if not callable(getattr(engine, m, None))]
        assert not missing, (engine.__name__, missing)
    for m in ("enable_spatial_correlation", "reset_spatial_correlation", "accumulate_spatial_correlation",
              "spatial_correlation_part", "spatial_correlation"):
        assert callable(getattr(CppSampler, m, None)), m


@pytest.fixture(scope="module")
def ranks():
    from epievo_amd.parallel import ShardedSampler
    n, ns = 1500, 3
    tree = config("tree")
    xs = [cr.rows(simulate("tree", n, seed=9 + i)[2], tree) for i in range(ns)]
    xs[1][2, 600:1100] = 1                         # pairs of ones across both boundaries of the middle rank
    cuts = [0, 700, 700 + L, n]                    # the middle rank holds exactly max_lag sites

    def part_of(a, b):
        p = cr.part(xs[0][:, a:b], L)
        for x in xs[1:]:
            p = cr.add_parts(p, cr.part(x[:, a:b], L))
        return p

    pieces, out = {}, []
    for r in range(3):
        s = object.__new__(ShardedSampler)
        s.comm, s.cuts = _FakeComm(3, r, pieces), cuts
        s.dev = _FakeDev(ns, part_of(cuts[r], cuts[r + 1]))
        out.append(s)
    return out, part_of(0, n), ns, n


def _fill(shards):
    """every rank leaves its pieces of both collectives (the ranks run one after the other here, so it takes two
    rounds)"""
    for _ in range(2):
        for s in shards:
            try:
                s.spatial_correlation_part()
            except RuntimeError:
                pass


def test_sharded_read_out_merges_in_genome_order(ranks):
    shards, full, ns, n = ranks
    _fill(shards)
    closed = cr.close(*full)
    for s in shards:
        got = s.spatial_correlation_part()
        assert got[0] == ns and got[1] == n and got[2].dtype == np.uint64 and got[3].dtype == np.uint64
        assert np.array_equal(got[2], full[1]) and np.array_equal(got[3], full[2])
        got = s.spatial_correlation()
        assert got[0] == ns and all(np.array_equal(g, w) for g, w in zip(got[1:], closed))
    # the ranks alone miss the pairs that cross their boundaries
    alone = sum(s.dev.part[1] for s in shards)
    assert (alone[:, 1:] <= full[1][:, 1:]).all() and (alone[2, 1:] < full[1][2, 1:]).all()
    assert np.array_equal(alone[:, 0], full[1][:, 0])


def test_sharded_sample_counts_must_agree(ranks):
    shards, full, ns, n = ranks
    _fill(shards)
    shards[1].dev.ns = ns - 1
    keep = shards[1].dev.part
    shards[1].dev.part = (keep[0], keep[1], keep[2][:ns - 1])
    try:
        for s in (shards[1], shards[0]):
            with pytest.raises(RuntimeError, match="different numbers"):
                s.spatial_correlation()
    finally:
        shards[1].dev.ns, shards[1].dev.part = ns, keep
    _fill(shards)
    assert np.array_equal(shards[0].spatial_correlation_part()[2], full[1])


def test_one_rank_needs_no_collective():
    from epievo_amd.parallel import ShardedSampler
    tree = config("tree")
    x = cr.rows(simulate("tree", 500, seed=3)[2], tree)
    p = cr.part(x, L)
    s = object.__new__(ShardedSampler)
    s.comm, s.cuts, s.dev = _FakeComm(1, 0, {}), [0, 500], _FakeDev(1, p)
    got = s.spatial_correlation()
    assert got[0] == 1 and all(np.array_equal(g, w) for g, w in zip(got[1:], cr.close(*p)))
    assert not s.comm.pieces
