"""Domain turnover, the layers above the device that need no GPU: ShardedSampler's read-out over stand-ins for the
device and the collective -- the ranks' parts all-gathered, the sample counts compared, every rank merging in
genome order and closing -- and that every engine has every method the layers call."""
import numpy as np
import pytest

import turnover_ref as tr
from common import simulate


class _Buf:
    def __init__(self, nbytes):
        self.data = np.zeros(nbytes, np.uint8)

    def free(self):
        pass


class _FakeDev:
    """what ShardedSampler asks of its device: this rank's part, and host-side buffers"""

    def __init__(self, ns, part):
        self.ns, self.part = ns, part

    def domain_turnover_part(self):
        return (self.ns,) + tuple(self.part)

    def domain_turnover_samples(self):
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
    asked = ["enable_domain_turnover", "reset_domain_turnover", "accumulate_domain_turnover", "domain_turnover_samples",
             "domain_turnover_layout", "domain_turnover_part", "domain_turnover"]
    assert sorted(m for m in vars(ShardedSampler) if "domain_turnover" in m) == sorted(asked)
    for engine in (DeviceSampler, LocalGroup, SingleSiteSampler, ShardedSampler):
        missing = [m for m in asked if not callable(getattr(engine, m, None))]
        assert not missing, (engine.__name__, missing)
    for m in ("enable_domain_turnover", "reset_domain_turnover", "accumulate_domain_turnover", "domain_turnover_part",
              "domain_turnover"):
        assert callable(getattr(CppSampler, m, None)), m


@pytest.fixture(scope="module")
def ranks():
    from epievo_amd.parallel import ShardedSampler
    n, ns = 3000, 3
    xs = [tr.rows(simulate("tree", n, seed=9 + i)[2]) for i in range(ns)]
    xs[1][2, 1000:2400] = 1                        # a run that spans a whole rank, kept only by a site of rank 2
    xs[1][3, 1000:2400] = 0
    xs[1][3, 2350] = 1
    cuts = [0, 1024, 2304, n]

    def part_of(a, b):
        p = tr.part(xs[0][:, a:b])
        for x in xs[1:]:
            p = tr.add_parts(p, tr.part(x[:, a:b]))
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
                s.domain_turnover_part()
            except RuntimeError:
                pass


def test_sharded_read_out_merges_in_genome_order(ranks):
    shards, full, ns, n = ranks
    mid = shards[1].dev.part[2][1, 2]
    assert (mid & np.uint64(tr.WHOLE)).all() and not (mid & np.uint64(tr.KEPT)).any()   # whole and turned over there
    _fill(shards)
    closed = tr.close(*full)
    for s in shards:
        got = s.domain_turnover_part()
        assert got[0] == ns and all(g.dtype == np.uint64 for g in got[1:])
        assert all(np.array_equal(g, w) for g, w in zip(got[1:], full))
        got = s.domain_turnover()
        assert got[0] == ns and np.array_equal(got[1], closed[0]) and np.array_equal(got[2], closed[1])
        assert (got[2].sum(axis=(1, 2)) == ns * n).all()
    assert closed[0][2, 1, 1, tr.bin_of(1400):].sum() >= 1        # the long run is kept in the merged result
    # a rank alone is not the genome
    assert not np.array_equal(shards[0].dev.part[0], full[0])


def test_sharded_sample_counts_must_agree(ranks):
    shards, full, ns, n = ranks
    _fill(shards)
    shards[1].dev.ns = ns - 1
    keep = shards[1].dev.part
    shards[1].dev.part = (keep[0], keep[1], keep[2][:ns - 1])
    try:
        for s in (shards[1], shards[0]):
            with pytest.raises(RuntimeError, match="different numbers"):
                s.domain_turnover()
    finally:
        shards[1].dev.ns, shards[1].dev.part = ns, keep
    _fill(shards)
    assert np.array_equal(shards[0].domain_turnover_part()[1], full[0])


def test_one_rank_needs_no_collective():
    from epievo_amd.parallel import ShardedSampler
    x = tr.rows(simulate("tree", 500, seed=3)[2])
    p = tr.part(x)
    s = object.__new__(ShardedSampler)
    s.comm, s.cuts, s.dev = _FakeComm(1, 0, {}), [0, 500], _FakeDev(1, p)
    got = s.domain_turnover()
    want = tr.close(*p)
    assert got[0] == 1 and np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1])
    assert not s.comm.pieces
