"""The chain mixing diagnostics without a GPU: the numpy yardstick (tests/mixing_ref.py) on hand-made histories
and its run rules, host.mixing_summary and host.mixing_window_summary on chains whose answer is known, LocalGroup's
read-outs over stand-ins for its shards, ShardedSampler's over stand-ins for the device and the collective, the file
round trip and the surface of the samplers."""
import inspect
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mixing_ref
from epievo_amd import host
from epievo_amd.host import FlatPaths

K = 3


def _fp(cells):
    """cells[b][s] = (init, [jump times]) -> FlatPaths of len(cells) branches"""
    B, n = len(cells), len(cells[0])
    flat = [cells[b][s] for b in range(B) for s in range(n)]
    off = np.concatenate([[0], np.cumsum([len(t) for _, t in flat])])
    jumps = np.array([v for _, t in flat for v in t], np.float64)
    return FlatPaths(n, B + 1, [a for a, _ in flat], off, jumps)


# two branches, four sites
BASE = [[(0, []), (1, [0.25]), (0, [0.1, 0.7]), (1, [])],
        [(0, [0.5]), (0, []), (1, [0.3]), (1, [])]]


def _with(cells, b, s, cell):
    out = [list(row) for row in cells]
    out[b][s] = cell
    return out


def test_what_counts_as_a_move():
    a = _fp(BASE)
    same = _fp([list(row) for row in BASE])
    assert not mixing_ref.differs(a, same).any()                                     # an identical history: no move
    time_only = _fp(_with(BASE, 0, 1, (1, [0.26])))                                  # a jump time alone changes
    assert mixing_ref.differs(a, time_only).tolist() == [False, True, False, False]
    assert np.array_equal(mixing_ref.jump_counts(a), mixing_ref.jump_counts(time_only))
    swapped = _fp(_with(_with(BASE, 0, 2, (0, [0.3, 0.7])), 1, 2, (1, [0.1])))        # 0.1 and 0.3 change branches
    assert mixing_ref.differs(a, swapped).tolist() == [False, False, True, False]
    init_only = _fp(_with(BASE, 1, 3, (0, [])))
    assert mixing_ref.differs(a, init_only).tolist() == [False, False, False, True]
    moved_jump = _fp(_with(_with(BASE, 0, 0, (0, [0.5])), 1, 0, (0, [])))             # the same x, on the other branch
    assert mixing_ref.differs(a, moved_jump).tolist() == [True, False, False, False]
    signed_zero = _fp(_with(BASE, 0, 1, (1, [-0.0])))                                 # bit patterns, not values
    assert mixing_ref.differs(_fp(_with(BASE, 0, 1, (1, [0.0]))), signed_zero)[1]
    # the vectorised comparison against the walk over every history
    for q in (same, time_only, swapped, init_only, moved_jump):
        walk = [mixing_ref.history(a, s) != mixing_ref.history(q, s) for s in range(4)]
        assert mixing_ref.differs(a, q).tolist() == walk


def test_run_rules():
    a, b = _fp(BASE), _fp(_with(BASE, 0, 1, (1, [0.26])))
    xa = mixing_ref.jump_counts(a).astype(np.uint64)        # [1, 1, 3, 0]
    assert xa.tolist() == [1, 1, 3, 0]
    # one run_mcmc call of four samples: the opening state is no sample, every sample is linked
    m = mixing_ref.Mixing(4, K)
    m.run_mcmc(a, [a, b, b, a])
    assert (m.samples, m.moved_pairs) == (4, 4) and m.pairs.tolist() == [0, 3, 2, 1]
    assert m.moved.tolist() == [0, 2, 0, 0]                 # a -> a no move, a -> b, b -> b no move, b -> a
    assert np.array_equal(m.S1, 4 * xa) and np.array_equal(m.S2, 4 * xa * xa)
    assert np.array_equal(m.C, np.outer([3, 2, 1], xa * xa).astype(np.uint64))
    # a second call links nothing to the first: the pairs add up per call
    m.run_mcmc(b, [a])
    assert (m.samples, m.moved_pairs) == (5, 5) and m.pairs.tolist() == [0, 3, 2, 1] and m.moved.tolist() == [0, 3, 0, 0]
    # explicit samples: the first opens a run and is linked to nothing; an unlinked one opens the next run
    e = mixing_ref.Mixing(4, K)
    e.sample(a, linked=True)                                # (no run is open: linked to nothing)
    e.sample(b)
    e.sample(a)
    assert (e.samples, e.moved_pairs) == (3, 2) and e.pairs.tolist() == [0, 2, 1, 0] and e.moved.tolist() == [0, 2, 0, 0]
    e.sample(b, linked=False)
    assert (e.samples, e.moved_pairs) == (4, 2) and e.pairs.tolist() == [0, 2, 1, 0] and e.moved.tolist() == [0, 2, 0, 0]
    e.sample(a)
    assert (e.samples, e.moved_pairs) == (5, 3) and e.pairs.tolist() == [0, 3, 1, 0] and e.moved.tolist() == [0, 3, 0, 0]
    # batch beyond the lag: the ring of the last K values
    r = mixing_ref.Mixing(4, 2)
    r.run_mcmc(a, [a] * 5)
    assert r.pairs.tolist() == [0, 4, 3] and np.array_equal(r.C, np.outer([4, 3], xa * xa).astype(np.uint64))
    # one run through the class equals the closed form over the chain of x
    ns, mp, pairs, S1, S2, C = mixing_ref.counts_of_chain(np.stack([xa] * 5), 2)
    assert (ns, mp) == (5, 4) and np.array_equal(pairs, r.pairs) and np.array_equal(C, r.C)
    assert np.array_equal(S1, r.S1) and np.array_equal(S2, r.S2)


def _summary_of_chain(xs, max_lag, moved=None):
    ns, mp, pairs, S1, S2, C = mixing_ref.counts_of_chain(xs, max_lag)
    moved = np.zeros(np.asarray(xs).shape[1], np.uint32) if moved is None else moved
    return host.mixing_summary(ns, mp, pairs, moved, S1, S2, C), (ns, mp, pairs, moved, S1, S2, C)


def test_summary_of_an_alternating_and_a_constant_chain():
    T = 40
    alt = np.where(np.arange(T) % 2 == 0, 2, 5)
    xs = np.stack([alt, np.full(T, 3)], axis=1)
    s, _ = _summary_of_chain(xs, 4, moved=np.array([T - 1, 0], np.uint32))
    assert s["samples"] == T and s["moved_pairs"] == T - 1 and s["move_rate"].tolist() == [1.0, 0.0]
    assert s["mean"].tolist() == [3.5, 3.0] and s["var"].tolist() == [2.25, 0.0]
    assert s["rho"][:, 0].tolist() == [1.0, -1.0, 1.0, -1.0, 1.0]
    assert np.isnan(s["rho"][:, 1]).all() and np.isnan(s["tau"][1]) and np.isnan(s["ess"][1])     # constant: nan
    assert s["ess"][0] == T                                                                       # clipped to samples
    with pytest.raises(ValueError):
        host.mixing_summary(0, 0, np.zeros(2, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint64),
                            np.zeros(1, np.uint64), np.zeros((1, 1), np.uint64))


def test_summary_recovers_tau_of_an_integer_ar1_chain():
    """binomial thinning, x_t = Bin(x_{t-1}, a) + Poisson(lam (1 - a)): an integer chain with rho_k = a^k exactly,
    so tau = (1 + a) / (1 - a).  Tolerance: the windowed estimator of tau over lags up to M has variance about
    2 (2 M + 1) tau^2 / T (Sokal); Geyer's sequence cuts at most at M = max_lag, so four standard deviations at
    M = max_lag bound the error from above.  What the lags beyond max_lag hold, 2 a^(M + 1) / (1 - a), is added."""
    a, lam, T, M, sites = 0.5, 20.0, 200000, 16, 3
    rng = np.random.default_rng(5)
    xs = np.zeros((T, sites), np.int64)
    x = rng.poisson(lam, sites)
    for t in range(T):
        x = rng.binomial(x, a) + rng.poisson(lam * (1.0 - a), sites)
        xs[t] = x
    s, _ = _summary_of_chain(xs, M)
    tau = (1.0 + a) / (1.0 - a)
    tol = 4.0 * tau * np.sqrt(2.0 * (2 * M + 1) / T) + 2.0 * a ** (M + 1) / (1.0 - a)
    assert tol < 0.25
    assert (np.abs(s["tau"] - tau) < tol).all(), (s["tau"], tol)
    assert np.allclose(s["ess"], T / s["tau"])
    assert (np.abs(s["rho"][1] - a) < 4.0 * 2.0 / np.sqrt(T)).all()      # (Bartlett: sd of rho_1 below 2 / sqrt(T))
    assert (np.abs(s["mean"] - lam) < 4.0 * np.sqrt(lam * tau / T)).all()


def test_window_summary_equals_direct_evaluation():
    rng = np.random.default_rng(11)
    T, n, W, first = 50, 23, 5, 7                          # global sites 7 .. 29: windows 1 .. 5, the first one cut
    xs = rng.integers(0, 6, (T, n))
    moved = rng.integers(0, T, n).astype(np.uint32)
    _, c = _summary_of_chain(xs, K, moved)
    w = host.mixing_window_summary(W, *c, first_site=first)
    assert w["first_window"] == 1 and w["sites"].tolist() == [3, 5, 5, 5, 5]
    x = xs.astype(np.float64)
    mean = x.mean(axis=0)
    var = (x * x).mean(axis=0) - mean * mean
    edges = [0, 3, 8, 13, 18, 23]
    for i, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        assert w["moved"][i] == moved[lo:hi].sum()
        assert w["move_rate"][i] == moved[lo:hi].sum() / float((T - 1) * (hi - lo))
        for k in range(1, K + 1):
            cov = (x[k:] * x[:-k]).sum(axis=0) / float(T - k) - mean * mean
            want = cov[lo:hi].sum() / var[lo:hi].sum() if var[lo:hi].sum() > 0 else np.nan
            assert np.isclose(w["rho"][k, i], want, rtol=1e-12, atol=1e-12, equal_nan=True)
    assert not np.isnan(w["rho"][:, :2]).any()
    # a window none of whose sites varies
    xs2 = xs.copy()
    xs2[:, 8:13] = 4
    w2 = host.mixing_window_summary(W, *_summary_of_chain(xs2, K, moved)[1], first_site=first)
    assert np.isnan(w2["rho"][:, 2]).all() and np.isnan(w2["tau"][2]) and not np.isnan(w2["rho"][:, 1]).any()
    with pytest.raises(ValueError):
        host.mixing_window_summary(0, *c)


def test_file_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    xs = rng.integers(0, 9, (30, 17))
    xs[:, 5:10] = 2                                        # global sites 10 .. 14: a window of nan
    moved = rng.integers(0, 29, 17).astype(np.uint32)
    _, c = _summary_of_chain(xs, K, moved)
    w = host.mixing_window_summary(5, *c, first_site=5)
    path = str(tmp_path / "mixing.txt")
    host.write_mixing(path, c[0], c[1], c[2], w)
    r = host.read_mixing(path)
    assert (r["samples"], r["moved_pairs"], r["max_lag"], r["window"], r["first_window"]) == (30, 29, K, 5, 1)
    assert np.array_equal(r["pairs"], c[2]) and np.array_equal(r["sites"], w["sites"])
    assert r["moved"].dtype == np.uint64 and np.array_equal(r["moved"], w["moved"])
    for key in ("move_rate", "rho", "tau"):                # bit for bit, nan where it was nan
        assert np.array_equal(r[key], w[key], equal_nan=True), key
    assert np.isnan(r["rho"][:, 1]).all() and not np.isnan(r["rho"][:, 0]).any()
    bad = tmp_path / "bad.txt"
    bad.write_text("samples 3\n")
    with pytest.raises(RuntimeError):
        host.read_mixing(str(bad))


# ---- LocalGroup over stand-ins for its shards
N_SITES, CUT = 40, 24


class _Shard:
    """a shard that answers mixing() and mixing_windows() with what it was given and notes every call"""
    n_global = N_SITES

    def __init__(self, counts):
        self.c, self.calls = counts, []

    def mixing(self, counts=False):
        self.calls.append(("mixing", counts))
        return self.c

    def mixing_windows(self, W, first_window, n_windows):
        self.calls.append(("mixing_windows", W, first_window, n_windows))
        return self.c[0], self.c[1], mixing_ref.windows(self.c[3], W, self.first, N_SITES)[first_window:first_window + n_windows]

    def mixing_layout(self):
        return self.first, len(self.c[3]), K

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            return self.c[0] if name.endswith("_samples") else None
        return call


@pytest.fixture()
def group():
    from epievo_amd.parallel import LocalGroup
    rng = np.random.default_rng(7)
    xs = rng.integers(0, 7, (9, N_SITES))
    moved = rng.integers(0, 8, N_SITES).astype(np.uint32)
    ns, mp, pairs, S1, S2, C = mixing_ref.counts_of_chain(xs, K)
    whole = (ns, mp, pairs, moved, S1, S2, C)
    g = object.__new__(LocalGroup)
    g.subs = []
    for a, b in ((0, CUT), (CUT, N_SITES)):
        s = _Shard((ns, mp, pairs.copy(), moved[a:b], S1[a:b], S2[a:b], C[:, a:b]))
        s.first = a
        g.subs.append(s)
    g.pool, g.halo_mode, g._closed = ThreadPoolExecutor(max_workers=2), False, True
    yield g, whole
    g.pool.shutdown(wait=True)


def test_group_concatenates_by_site(group):
    g, whole = group
    got = g.mixing(counts=True)
    assert got[:2] == whole[:2] and all(np.array_equal(a, b) for a, b in zip(got[2:], whole[2:]))
    assert [a.dtype for a in got[2:]] == [np.uint64, np.uint32, np.uint64, np.uint64, np.uint64]
    assert all(s.calls == [("mixing", True)] for s in g.subs)
    s = g.mixing()
    want = host.mixing_summary(*whole)
    assert sorted(s) == sorted(want) and all(np.array_equal(s[k], want[k], equal_nan=True) for k in want)
    assert g.mixing_layout() == (0, N_SITES, K)
    # windows: 7 divides neither the cut nor the genome, the shards' contributions add up
    ns, mp, win = g.mixing_windows(7)
    assert (ns, mp) == whole[:2] and win.dtype == np.uint64 and np.array_equal(win, mixing_ref.windows(whole[3], 7))
    assert g.subs[1].calls[-1] == ("mixing_windows", 7, 0, 6)
    assert np.array_equal(g.mixing_windows(7, 2, 3)[2], mixing_ref.windows(whole[3], 7)[2:5])
    with pytest.raises(ValueError):
        g.mixing_windows(0)


def test_group_refuses_shards_of_different_runs(group):
    g, _ = group
    c = g.subs[1].c
    g.subs[1].c = c[:2] + (c[2] + np.array([0, 0, 1, 0], np.uint64),) + c[3:]          # pairs[2] differs
    with pytest.raises(RuntimeError, match="pair counts differ"):
        g.mixing(counts=True)
    g.subs[1].c = (c[0], c[1] - 1) + c[2:]                                               # moved_pairs differs
    for call in (lambda: g.mixing(counts=True), lambda: g.mixing_windows(7)):
        with pytest.raises(RuntimeError, match="pair counts differ"):
            call()
    g.subs[1].c = (c[0] + 1,) + c[1:]                                                    # the samples differ
    with pytest.raises(RuntimeError) as e:
        g.mixing(counts=True)
    assert str(e.value) == "the shards of the group hold different numbers of mixing samples"


def test_group_lifecycle_and_its_guard(group):
    g, whole = group
    assert g.enable_mixing(5) is None and g.reset_mixing() is None
    assert all(s.calls == [("enable_mixing", (5,), {}), ("reset_mixing", (), {})] for s in g.subs)
    assert g.mixing_samples() == whole[0]
    for s in g.subs:
        del s.calls[:]
    with pytest.raises(RuntimeError) as e:                 # before the first reset() the shards' ranges overlap
        g.accumulate_mixing()
    assert str(e.value) == "reset() the group before taking a mixing sample"
    assert not g.subs[0].calls and not g.subs[1].calls
    g.halo_mode = True
    assert g.accumulate_mixing() is None
    assert all(s.calls == [("accumulate_mixing", (), {})] for s in g.subs)


def test_surface():
    from epievo_amd import sampler, summaries
    from epievo_amd.parallel import LocalGroup, ShardedSampler
    from epievo_amd.sampler import DeviceSampler, SingleSiteSampler
    assert len(summaries.SUMMARIES) == 9 and "mixing" not in [s.stem for s in summaries.SUMMARIES]
    assert [(s.stem, s.article, s.noun) for s in summaries.DIAGNOSTICS] == [("mixing", "a", "mixing")]
    stems = [s.stem for s in summaries.SUMMARIES] + ["mixing"]
    assert len(stems) == 10
    for stem in stems:                                      # the ten lifecycles on the four classes
        for name in ("enable_" + stem, "reset_" + stem, "accumulate_" + stem, stem + "_samples"):
            assert name in summaries.LIFECYCLE
            for cls in (DeviceSampler, SingleSiteSampler, ShardedSampler, LocalGroup):
                assert inspect.isfunction(vars(cls).get(name)), (cls, name)
    for cls in (DeviceSampler, SingleSiteSampler, ShardedSampler, LocalGroup):
        for name in ("mixing", "mixing_layout", "mixing_windows"):
            assert callable(getattr(cls, name, None)), (cls, name)
    assert str(inspect.signature(DeviceSampler.enable_mixing)) == "(self, max_lag=8)"
    assert inspect.signature(SingleSiteSampler.enable_mixing) == inspect.signature(DeviceSampler.enable_mixing)
    assert str(inspect.signature(DeviceSampler.mixing)) == "(self, counts=False)"
    assert str(inspect.signature(DeviceSampler.mixing_windows)) == "(self, W, first_window=0, n_windows=None)"
    for name in ("epv_set_mixing", "epv_reset_mixing", "epv_accumulate_mixing", "epv_mixing_samples", "epv_mixing_layout",
                 "epv_mixing_pairs", "epv_mixing_counts", "epv_mixing_windows"):
        assert name in sampler.ABI_SYMBOLS
    assert sampler.MIXING_MAX_LAG == 16


# ---- ShardedSampler over stand-ins for the device and the collective
class _Buf:
    def __init__(self, nbytes):
        self.data = np.zeros(nbytes, np.uint8)

    def free(self):
        pass


class _RankDev:
    """what ShardedSampler asks of its device: this rank's counts, and host-side buffers"""

    def __init__(self, counts, first):
        self.c, self.first = counts, first

    def mixing(self, counts=False):
        assert counts
        return self.c

    def mixing_windows(self, W):
        return self.c[0], self.c[1], mixing_ref.windows(self.c[3], W, self.first, N_SITES)

    def alloc(self, nbytes):
        return _Buf(nbytes)

    def write(self, buf, offset, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf.data[offset:offset + raw.size] = raw

    def read(self, buf, offset, count, dtype=np.float64):
        return buf.data[offset:offset + count * np.dtype(dtype).itemsize].view(dtype).copy()


class _Comm:
    """an all-gather among ranks that run one after the other: pieces are remembered by rank and call"""

    def __init__(self, world, rank, pieces):
        self.world, self.rank, self.pieces, self.calls = world, rank, pieces, 0

    def all_gather(self, dev, piece, gathered):
        key = self.calls
        self.calls += 1
        self.pieces.setdefault(key, {})[self.rank] = piece.data.copy()
        k = piece.data.size
        for r, p in self.pieces[key].items():
            if p.size == k:
                gathered.data[r * k:(r + 1) * k] = p


@pytest.fixture()
def ranks():
    from epievo_amd.parallel import ShardedSampler
    cuts = [0, 11, CUT, N_SITES]                           # unequal widths: the padding matters
    rng = np.random.default_rng(13)
    xs = rng.integers(0, 2 ** 20, (9, N_SITES))            # sums beyond 32 bits: both words of a cell travel
    moved = rng.integers(0, 8, N_SITES).astype(np.uint32)
    ns, mp, pairs, S1, S2, C = mixing_ref.counts_of_chain(xs, K)
    assert (S2 > 2 ** 32).any()
    pieces, out = {}, []
    for r in range(3):
        a, b = cuts[r], cuts[r + 1]
        s = object.__new__(ShardedSampler)
        s.comm, s.cuts = _Comm(3, r, pieces), cuts
        s.dev = _RankDev((ns, mp, pairs.copy(), moved[a:b], S1[a:b], S2[a:b], C[:, a:b]), a)
        out.append(s)
    return out, (ns, mp, pairs, moved, S1, S2, C)


def _round(shards, call):
    """every rank makes the call once so that all pieces are there (the first ranks see some missing), then again"""
    for s in shards:
        try:
            call(s)
        except RuntimeError:
            pass
        s.comm.calls = 0
    out = [call(s) for s in shards]
    for s in shards:
        s.comm.calls = 0
    return out


def test_sharded_mixing_concatenates_in_genome_order(ranks):
    shards, whole = ranks
    for got in _round(shards, lambda s: s.mixing(counts=True)):
        assert got[:2] == whole[:2] and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got[2:], whole[2:]))
    assert all(len(s.comm.pieces) == 1 for s in shards)    # one collective
    want = host.mixing_summary(*whole)
    for got in _round(shards, lambda s: s.mixing()):
        assert all(np.array_equal(got[k], want[k], equal_nan=True) for k in want)
    for ns, mp, win in _round(shards, lambda s: s.mixing_windows(7)):
        assert (ns, mp) == whole[:2] and np.array_equal(win, mixing_ref.windows(whole[3], 7))
    # a rank whose runs differ
    c = shards[1].dev.c
    shards[1].dev.c = c[:2] + (c[2] + np.array([0, 1, 0, 0], np.uint64),) + c[3:]
    for s in shards:
        with pytest.raises(RuntimeError, match="pair counts differ|different numbers"):
            s.mixing(counts=True)
        s.comm.calls = 0
    shards[1].dev.c = (c[0] + 1,) + c[1:]
    for s in (shards[1], shards[0]):
        with pytest.raises(RuntimeError) as e:
            s.mixing(counts=True)
        s.comm.calls = 0
        assert str(e.value) == "the ranks hold different numbers of mixing samples"
