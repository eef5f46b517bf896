"""Lineage origin maps, the layers above the device that need no GPU: ShardedSampler's read-out over stand-ins
for the device and the collective -- the ranks' cells gathered and concatenated along sites (64-bit ages
included), the sample counts and the scale compared, window sums added across ranks as integers -- and that
DeviceSampler and LocalGroup have every method the sharded layer calls."""
import numpy as np
import pytest

import origin_ref
from common import simulate


class _Buf:
    def __init__(self, nbytes):
        self.data = np.zeros(nbytes, np.uint8)

    def free(self):
        pass


class _FakeDev:
    """what ShardedSampler asks of its device: this rank's cells and window contributions, and host-side buffers"""

    def __init__(self, ns, k, rows, origin, age, first_site, n_global):
        self.ns, self.k, self.rows, self.origin, self.age = ns, k, rows, origin, age
        self.first_site, self.n_global = first_site, n_global

    def lineage_origins(self, counts=False):
        assert counts
        return self.ns, self.rows, self.origin, self.age

    def lineage_origins_scale_exp(self):
        return self.k

    def lineage_origin_rows(self):
        return self.rows

    def lineage_origins_samples(self):
        return self.ns

    def lineage_origin_windows(self, W):
        return (self.ns, origin_ref.windows(self.origin, W, self.first_site, self.n_global),
                origin_ref.windows(self.age, W, self.first_site, self.n_global))

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
        self.pieces[self.rank] = piece.data.copy()
        k = piece.data.size
        for r, p in self.pieces.items():
            if p.size == k:
                gathered.data[r * k:(r + 1) * k] = p


def test_engines_have_what_the_sharded_layer_asks_for():
    from epievo_amd.parallel import LocalGroup, ShardedSampler
    from epievo_amd.sampler import DeviceSampler, SingleSiteSampler
    asked = [m for m in vars(_FakeDev) if not m.startswith("_")]
    asked += [m for m in vars(ShardedSampler) if "lineage_origin" in m]
    for m in ("enable_lineage_origins", "reset_lineage_origins", "accumulate_lineage_origins", "lineage_origins_samples",
              "lineage_origin_rows", "lineage_origins", "lineage_origin_windows"):
        assert m in asked
    for engine in (DeviceSampler, LocalGroup):
        missing = [m for m in asked + ["lineage_origins_layout"] if not callable(getattr(engine, m, None))]
        assert not missing, (engine.__name__, missing)
    # the same methods on every layer
    import inspect
    from epievo_amd.driver import CppSampler
    same = ("enable_lineage_origins", "reset_lineage_origins", "accumulate_lineage_origins", "lineage_origin_rows",
            "lineage_origins_scale_exp", "lineage_origins", "lineage_origin_windows")
    for layer in (DeviceSampler, SingleSiteSampler, LocalGroup, ShardedSampler, CppSampler):
        missing = [m for m in same if not callable(getattr(layer, m, None))]
        assert not missing, (layer.__name__, missing)
    for layer in (DeviceSampler, SingleSiteSampler, LocalGroup, ShardedSampler):
        for m in ("lineage_origins_samples", "lineage_origins_layout"):
            assert callable(getattr(layer, m, None)), (layer.__name__, m)
    for layer in (DeviceSampler, SingleSiteSampler, LocalGroup):      # a piece of the windows can be asked for
        assert list(inspect.signature(layer.lineage_origin_windows).parameters)[1:] == ["W", "first_window", "n_windows"]


@pytest.fixture(scope="module")
def ranks():
    from epievo_amd.parallel import ShardedSampler
    n, ns = 3000, 5
    model, tree, fp = simulate("tree", n, seed=9)
    tab = origin_ref.tables(tree)
    origin, age = origin_ref.sample(fp, tree, tab)
    origin, age = origin * np.uint32(ns), age * np.uint64(ns)
    age[0, 7] += np.uint64(3 << 40)                # a cell whose high word is not zero goes through the gather
    cuts = [0, 1024, 2304, n]                      # unequal pieces, cut inside windows of 100 sites
    pieces, out = {}, []
    for r in range(3):
        s = object.__new__(ShardedSampler)
        s.comm, s.cuts = _FakeComm(3, r, pieces), cuts
        a, b = cuts[r], cuts[r + 1]
        s.dev = _FakeDev(ns, tab["k"], tab["rows"], origin[:, a:b].copy(), age[:, a:b].copy(), a, n)
        out.append(s)
    return out, tab, origin, age, ns, n


def test_sharded_read_out_concatenates_along_sites(ranks):
    shards, tab, origin, age, ns, n = ranks
    for s in shards:                               # round 0 only fills the pieces: the others' are still missing
        if s is shards[-1]:
            s.lineage_origins(counts=True)
        else:
            with pytest.raises(RuntimeError, match="different numbers"):
                s.lineage_origins(counts=True)
    for s in shards:
        got_ns, rows, o, a = s.lineage_origins(counts=True)
        assert got_ns == ns and np.array_equal(rows, tab["rows"])
        assert o.dtype == np.uint32 and o.shape == origin.shape and np.array_equal(o, origin)
        assert a.dtype == np.uint64 and a.shape == age.shape and np.array_equal(a, age)
        got_ns, rows, p, mean_age = s.lineage_origins()
        assert np.array_equal(p, origin / float(ns))
        assert np.array_equal(mean_age, np.ldexp(age.astype(np.float64), -tab["k"]) / ns)
    # posterior over the origin branch: a leaf's rows sum to one
    for li in range(len(tab["leaves"])):
        assert np.array_equal(p[tab["first"][li]:tab["first"][li + 1]].sum(axis=0), np.ones(n))


@pytest.mark.parametrize("W", [1, 100, 1000, 10 ** 6])
def test_sharded_window_sums_add_as_integers(ranks, W):
    shards, tab, origin, age, ns, n = ranks
    for s in shards:
        try:
            s.lineage_origin_windows(W)            # (fills the pieces of this size)
        except RuntimeError:
            pass
    want_o, want_a = origin_ref.windows(origin, W), origin_ref.windows(age, W)
    for s in shards:
        got_ns, ow, aw = s.lineage_origin_windows(W)
        assert got_ns == ns and ow.dtype == np.uint64 and aw.dtype == np.uint64
        assert np.array_equal(ow, want_o) and np.array_equal(aw, want_a)
    if W == 100:                                   # window 10 = sites 1000 .. 1099 straddles the first cut
        p0, p1 = (s.dev.lineage_origin_windows(W)[1] for s in shards[:2])
        assert p0[:, 10].any() and p1[:, 10].any()


def _fill(shards):
    """every rank leaves its current piece (a rank that meets a stale piece of another raises: that is the check)"""
    for s in shards:
        try:
            s.lineage_origins(counts=True)
        except RuntimeError:
            pass


def test_sharded_sample_counts_and_scales_must_agree(ranks):
    shards, tab, origin, age, ns, n = ranks
    _fill(shards)
    shards[1].dev.ns = ns - 1
    try:
        for s in (shards[1], shards[0]):
            with pytest.raises(RuntimeError, match="different numbers"):
                s.lineage_origins(counts=True)
        with pytest.raises(RuntimeError, match="different numbers"):
            shards[1].lineage_origin_windows(100)
    finally:
        shards[1].dev.ns = ns
    _fill(shards)
    assert np.array_equal(shards[0].lineage_origins(counts=True)[2], origin)
    shards[2].dev.k = tab["k"] + 1
    try:
        for s in (shards[2], shards[0]):           # (the first call leaves rank 2's piece, with its own k)
            with pytest.raises(RuntimeError, match="different scales"):
                s.lineage_origins(counts=True)
    finally:
        shards[2].dev.k = tab["k"]
    _fill(shards)
    assert np.array_equal(shards[0].lineage_origins(counts=True)[3], age)


def test_sums_over_contexts_refuse_to_wrap(ranks):
    """a single context refuses an age sum of a window beyond 64 bits; so do the sums over shards and ranks"""
    from epievo_amd.parallel import LocalGroup, add_uint64
    a = np.array([[1, 2 ** 63], [5, 7]], np.uint64)
    b = np.array([[2, 2 ** 63 - 1], [1, 1]], np.uint64)
    got = add_uint64([a, b])
    assert got.dtype == np.uint64 and got.tolist() == [[3, 2 ** 64 - 1], [6, 8]]
    assert np.array_equal(add_uint64([a]), a) and add_uint64([a]) is not a
    with pytest.raises(OverflowError, match="64 bits"):
        add_uint64([a, b, np.array([[0, 1], [0, 0]], np.uint64)])
    # ranks: one rank's age sum near 2^64 (the layer adds what the engines give, whatever the sample count)
    shards, tab, origin, age, ns, n = ranks
    W = 10 ** 6
    big = shards[0].dev.age.copy()
    keep = shards[0].dev.age
    big[1, 0] = np.uint64(2 ** 64 - 1) - big[1, 1:].sum(dtype=np.uint64)       # rank 0's window sum: 2^64 - 1
    shards[0].dev.age = big
    try:
        for s in shards:
            try:
                s.lineage_origin_windows(W)
            except (RuntimeError, OverflowError):
                pass
        for s in shards:
            with pytest.raises(OverflowError, match="64 bits"):
                s.lineage_origin_windows(W)
    finally:
        shards[0].dev.age = keep
    # shards of a group
    g = object.__new__(LocalGroup)
    g.subs = [s.dev for s in shards]
    g._each = lambda fn: [fn(j, s) for j, s in enumerate(g.subs)]
    for s in g.subs:
        s.lineage_origin_windows = (lambda dev: lambda W, first_window=0, n_windows=None:
                                    type(dev).lineage_origin_windows(dev, W))(s)
    ns3, ow, aw = g.lineage_origin_windows(100)
    assert ns3 == ns and np.array_equal(ow, origin_ref.windows(origin, 100))
    assert np.array_equal(aw, origin_ref.windows(age, 100))
    shards[0].dev.age = big
    try:
        with pytest.raises(OverflowError, match="64 bits"):
            g.lineage_origin_windows(W)
    finally:
        shards[0].dev.age = keep
        for s in g.subs:
            del s.lineage_origin_windows
