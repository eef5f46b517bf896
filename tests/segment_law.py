"""The law of a segment of the two-state chain given both of its ends, in closed form (mpmath, 50 digits), and the
goodness-of-fit statistics that compare a sampler's draws with it.  A helper, not a test module; nothing here comes from
the code under test.  tests/test_segment_law.py holds the reference's self-checks and the CPU legs,
tests/test_segment_law_gpu.py the device legs.

Notation: start state a, end state b, length T, rates r0 and r1 of leaving 0 and 1; ra = the rate of leaving a, rb that
of leaving the other state, l = ra + rb.

  P_xx(t) = (r_other + r_x e^{-l t}) / l,  P_xy(t) = r_x (1 - e^{-l t}) / l  (x != y)
  P(N_t = i | start a) = entry [0, i] of expm(G t), G the generator of the counting chain (bidiagonal, the rate out of
      i is the rate of leaving a xor (i & 1)).  Its Laplace transform is c_i / ((s + ra)^m (s + rb)^n) with
      m = i // 2 + 1, m + n = i + 1, c_i = ra^ceil(i/2) rb^floor(i/2): the convolution of two gamma densities,
      P(N_t = i) = c_i t^i / i! e^{-rb t} 1F1(m; i + 1; -(ra - rb) t)
      (i = 0: e^{-ra t}; i = 1: ra (e^{-rb t} - e^{-ra t}) / (ra - rb), ra t e^{-ra t} at ra == rb).
      tests/test_segment_law.py checks it against mpmath's expm of G t
  (i)   P(N = k | a, b, T) = P(N_T = k | a) / P_ab(T) for k of the parity of a != b, 0 otherwise
  (ii)  S_j(t) = P(tau_j > t | a, b, T) = sum_{i < j} P(N_t = i | a) P_{a xor (i & 1), b}(T - t) / P_ab(T), j = 1, 2
  (iii) the chain is reversible: T - tau_last given a -> b has the law of tau_1 given b -> a.

Statistics: chi-square goodness of fit.  Jump count: bins whose expected count is at least 10 stand alone, the rest are
pooled, a pool still below 10 joins its neighbour (the standalone bin of the largest count).  Jump times: 20 bins of equal
reference probability given that the jump exists, the edges from bisection on S_j, the bins' probabilities then taken
from S_j at the edges as doubles; skipped where the reference expects fewer than 2 000 draws with that jump.

Decision rule: with M statistics in a test module every p-value must be at least 1e-6 / M.  Seeds are fixed; a correct
sampler fails a module with probability at most 1e-6."""
import functools

import mpmath as mp
import numpy as np

DPS = 50
DRAWS = 1 << 18             # per row on the device and in the numpy model
CPU_DRAWS = 40000           # per row of the Python restatement and of the oracle's sampler
ALPHA = 1e-6
TIME_BINS = 20
MIN_EXPECTED = 10.0
MIN_TIME_DRAWS = 2000.0
KAT_SLOTS, KAT_TIMES = 64, 8      # epv_direct_kat: room, stored times
TRIAL_GROUPS, TRIAL_WINDOW = 16, 8
STATS = ("count", "tau1", "tau2", "last")

# ---------------------------------------------------------------------------------------------------------
# the settings: (a, b, T, r0, r1)
LAW = ((0, 0, 0.5, 1.3, 0.7), (0, 1, 0.5, 1.3, 0.7), (1, 1, 2.0, 3.0, 0.4), (1, 0, 0.05, 0.2, 5.0), (0, 0, 3.0, 4.0, 0.5))
_AB = ((0, 0), (0, 1), (1, 0), (1, 1))


def _all_ab(T, r0, r1):
    return tuple((a, b, T, r0, r1) for a, b in _AB)


# one triple per model of model_cases.MODELS, in that order: of the triples test_direct_sampler.model_space_segments()
# holds for the model, the one with the largest max(r0, r1) T whose row meets row_conditions() (ties: the smallest
# triple).  One (a, b) each, the four in turn: with all four the table would pass its 40 rows.
# test_segment_law.test_model_rows_are_the_rules_choice recomputes them.
MODEL_ROWS = (
    (0, 0, 10.0, 0.23633156236762334, 10.200988978527025),        # ref: max rate x T = 102
    (0, 1, 0.3, 0.2091638054283354, 75.50813375962893),           # anti: 22.65
    (1, 0, 1.0, 0.5096843491766153, 124.88540765700007),          # mixed: 124.9
    (1, 1, 1.0, 0.22879248842433147, 228335.13223997084),         # skew: 2.283e5
    (0, 0, 1.0, 0.23297126032034346, 2283.351322399682),          # skewm: 2283
    (0, 1, 1.0, 2.3633156236762337e-10, 1.0200988978527026e-08),  # slow: 1.02e-8
    (1, 0, 1.0, 419.5433810767991, 8.694152309497515),            # fast: 419.5 (the second largest: the largest has
                                                                  # P(N > 64) x draws above 0.01)
    (1, 1, 1.0, 41954.33810767991, 8.694152309497515e-06),        # ratio: 4.195e4
)

# 37 rows.  Equal rates make (1, 1) the law of (0, 0) and (1, 0) that of (0, 1): those two settings take two rows each
ROWS = (LAW
        + _all_ab(0.8, 4.2e4, 8.7e-6) + _all_ab(0.8, 8.7e-6, 4.2e4)          # ratio's worst pair and its mirror
        + _all_ab(0.3, 125.0, 1.7e-4) + _all_ab(0.3, 1.7e-4, 125.0)          # mixed
        + ((0, 0, 1.0, 20.0, 20.0), (0, 1, 1.0, 20.0, 20.0))                 # about 20 jumps, within the 64 slots
        + _all_ab(1e-6, 1e-3, 1e-6)
        + ((0, 1, 1.0, 1e-9, 1e-9), (1, 1, 1.0, 1e-9, 1e-9))
        + MODEL_ROWS)


# ---------------------------------------------------------------------------------------------------------
# the reference
def _with_precision(f):
    @functools.wraps(f)
    def g(*args, **kw):
        with mp.workdps(DPS):
            return f(*args, **kw)
    return g


class SegmentLaw(object):
    """the closed forms of one row; every method returns mpmath numbers at DPS digits"""

    @_with_precision
    def __init__(self, a, b, T, r0, r1):
        self.a, self.b = int(a), int(b)
        self.T, self.r = mp.mpf(T), (mp.mpf(r0), mp.mpf(r1))
        self.ra, self.rb = self.r[self.a], self.r[1 - self.a]
        self.l = self.ra + self.rb
        self._pmf = None

    @_with_precision
    def trans(self, x, y, t):
        """P_xy(t)"""
        rx, ro = self.r[x], self.r[1 - x]
        if x == y:
            return (ro + rx * mp.exp(-self.l * t)) / self.l
        return -rx * mp.expm1(-self.l * t) / self.l

    @_with_precision
    def count_at(self, i, t):
        """P(N_t = i | start a), any i"""
        t = mp.mpf(t)
        c = self.ra ** ((i + 1) // 2) * self.rb ** (i // 2)
        return c * t ** i / mp.factorial(i) * mp.exp(-self.rb * t) * mp.hyp1f1(i // 2 + 1, i + 1, -(self.ra - self.rb) * t)

    @_with_precision
    def count01_at(self, i, t):
        """P(N_t = i | start a) for i = 0, 1 in the elementary closed forms"""
        t = mp.mpf(t)
        if i == 0:
            return mp.exp(-self.ra * t)
        if self.ra == self.rb:
            return self.ra * t * mp.exp(-self.ra * t)
        # e^{-rb t} - e^{-ra t} = -e^{-rb t} expm1(-(ra - rb) t)
        return -self.ra * mp.exp(-self.rb * t) * mp.expm1(-(self.ra - self.rb) * t) / (self.ra - self.rb)

    @_with_precision
    def joint(self, k):
        """P(N_T = k, end b | start a): 0 for k of the wrong parity"""
        if (k & 1) != (self.a != self.b):
            return mp.mpf(0)
        return self.count_at(k, self.T)

    @_with_precision
    def pmf(self):
        """law (i) as a list over k = 0 .. K, K where the mass left is below 1e-40"""
        if self._pmf is None:
            pab, out, tot, k = self.trans(self.a, self.b, self.T), [], mp.mpf(0), 0
            while True:
                out.append(self.joint(k) / pab)
                tot += out[-1]
                k += 1
                if abs(1 - tot) < mp.mpf(10) ** -40 and (k & 1) != (self.a != self.b):
                    break
                assert k < 2000, "the jump count's law does not close"
            self._pmf = out
        return self._pmf

    @_with_precision
    def more_than(self, k):
        """P(N > k | a, b, T)"""
        return max(mp.mpf(0), 1 - mp.fsum(self.pmf()[:k + 1]))

    @_with_precision
    def fewer_than(self, j):
        """P(N < j | a, b, T)"""
        return mp.fsum(self.pmf()[:j])

    @_with_precision
    def survival(self, j, t):
        """law (ii): S_j(t) = P(tau_j > t | a, b, T), j = 1, 2 (tau_j = infinity where there is no j-th jump)"""
        t = mp.mpf(t)
        tot = mp.mpf(0)
        for i in range(j):
            tot += self.count01_at(i, t) * self.trans(self.a ^ (i & 1), self.b, self.T - t)
        return tot / self.trans(self.a, self.b, self.T)

    def reversed(self):
        """law (iii): T - tau_last of this row has the law of tau_1 of the returned row"""
        return law(self.b, self.a, float(self.T), float(self.r[0]), float(self.r[1]))

    @_with_precision
    def trial_success(self):
        """the probability that ONE trial of the default sampler succeeds: a kept state by forward rejection, P_aa(T);
        a state change by Nielsen's first jump, the integral of the truncated-exponential density against
        P_bb(T - tau)"""
        if self.a == self.b:
            return self.trans(self.a, self.a, self.T)
        w = -mp.expm1(-self.ra * self.T)
        return mp.quad(lambda x: self.ra * mp.exp(-self.ra * x) / w * self.trans(self.b, self.b, self.T - x),
                       mp.linspace(0, self.T, 9))


@functools.lru_cache(maxsize=None)
def law(a, b, T, r0, r1):
    return SegmentLaw(a, b, T, r0, r1)


# ---------------------------------------------------------------------------------------------------------
# conditions on a row, from the reference alone
def row_conditions(row, draws=DRAWS):
    """P(N > 64 | end) x draws < 0.01: no draw of the device test overflows the known-answer entry's 64 slots"""
    return float(law(*row).more_than(KAT_SLOTS) * draws) < 0.01


def last_allowed(row, draws=DRAWS, stored=KAT_TIMES):
    """the last jump is among the times an entry returns: P(N > stored | end) x draws < 0.01 (stored None: all are)"""
    return stored is None or float(law(*row).more_than(stored) * draws) < 0.01


def trial_leg(row, draws=DRAWS):
    """the default sampler's leg runs the row: epv_trial_kat accepts it (rates above 1e-3, T x max rate <= 64, the
    bracket 1 - exp(-ra T) of a state change below 1 as a double: ra T <= 36 leaves e^{-36} = 2.3e-16 > 2^-53) and the
    search of 128 trials leaves no item unresolved: (1 - p)^128 x draws < 0.01"""
    a, b, T, r0, r1 = row
    if not (min(r0, r1) > 1e-3 and T * max(r0, r1) <= 64.0):
        return False
    if a != b and (r1 if a else r0) * T > 36.0:
        return False
    with mp.workdps(DPS):
        return float((1 - law(*row).trial_success()) ** (TRIAL_GROUPS * TRIAL_WINDOW) * draws) < 0.01


# ---------------------------------------------------------------------------------------------------------
# statistics
def chi2_p(observed, expected):
    """(p-value, chi-square, degrees of freedom) of observed counts against expected ones; p = 1 with a single bin"""
    o, e = np.asarray(observed, float), np.asarray(expected, float)
    assert o.shape == e.shape and np.all(e > 0.0)
    if len(e) < 2:
        return 1.0, 0.0, 0
    x = float(((o - e) ** 2 / e).sum())
    with mp.workdps(30):
        p = mp.gammainc(mp.mpf(len(e) - 1) / 2, mp.mpf(x) / 2, mp.inf, regularized=True)
        return float(p), x, len(e) - 1


def count_bins(row, draws):
    """the jump count's bins: ([k, ...] per bin, expected count per bin); the last bin also takes every k beyond the
    list of pmf() (mass below 1e-40)"""
    pm = law(*row).pmf()
    ks = [k for k in range(len(pm)) if (k & 1) == (row[0] != row[1])]
    alone = [k for k in ks if float(pm[k] * draws) >= MIN_EXPECTED]
    pool = [k for k in ks if k not in alone]
    bins = [[k] for k in alone]
    exp_pool = float(mp.fsum(pm[k] for k in pool) * draws)
    if exp_pool >= MIN_EXPECTED or not bins:
        bins.append(pool)
    else:
        bins[-1] = bins[-1] + pool
    return bins, [float(mp.fsum(pm[k] for k in ks_) * draws) for ks_ in bins]


def count_p(row, counts):
    counts = np.asarray(counts, np.int64)
    assert np.all((counts & 1) == (row[0] != row[1])), "a jump count of the wrong parity"
    bins, expected = count_bins(row, len(counts))
    where = {}
    for i, ks in enumerate(bins):
        for k in ks:
            where[k] = i
    hist = np.bincount(counts)
    obs = np.zeros(len(bins))
    for k, c in enumerate(hist):
        if c:
            obs[where.get(k, len(bins) - 1)] += c
    return chi2_p(obs, expected)


@functools.lru_cache(maxsize=None)
def time_edges(row, j):
    """(the 19 inner edges as doubles, the 20 bins' probabilities given that the j-th jump exists) of tau_j"""
    L = law(*row)
    T = float(L.T)
    with mp.workdps(DPS):
        s_end = L.fewer_than(j)

        def cdf(t):
            return (1 - L.survival(j, t)) / (1 - s_end)
        edges = []
        for q in range(1, TIME_BINS):
            lo, hi, target = 0.0, T, mp.mpf(q) / TIME_BINS
            for _ in range(80):
                mid = 0.5 * (lo + hi)
                if mid <= lo or mid >= hi:
                    break
                if cdf(mid) < target:
                    lo = mid
                else:
                    hi = mid
            edges.append(hi)
        c = [mp.mpf(0)] + [cdf(e) for e in edges] + [mp.mpf(1)]
        return np.array(edges), np.array([float(c[i + 1] - c[i]) for i in range(TIME_BINS)])


def time_p(row, j, times):
    """times: tau_j of the draws that have a j-th jump, measured from the segment's start"""
    times = np.asarray(times, float)
    assert len(times) and times.min() > 0.0 and times.max() < row[2], "a jump time outside its segment"
    edges, prob = time_edges(row, j)
    obs = np.bincount(np.searchsorted(edges, times, side="right"), minlength=TIME_BINS)
    return chi2_p(obs, prob * len(times))


def planned(row, draws, stored=KAT_TIMES, which=STATS):
    """the statistics a leg computes on the row, from the reference alone"""
    L, out = law(*row), []
    for name in which:
        if name == "count":
            out.append(name)
        elif name in ("tau1", "tau2"):
            if float((1 - L.fewer_than(int(name[3]))) * draws) >= MIN_TIME_DRAWS:
                out.append(name)
        elif float((1 - L.fewer_than(1)) * draws) >= MIN_TIME_DRAWS and last_allowed(row, draws, stored):
            out.append(name)
    return out


def statistics(row, sample, stored=KAT_TIMES, which=STATS):
    """sample: dict of count [n], tau1, tau2, last [n] (from the segment's start; read only where the jump exists).
    -> {name: (p, chi-square, degrees of freedom)} of the planned statistics"""
    n, cnt, out = len(sample["count"]), np.asarray(sample["count"]), {}
    for name in planned(row, n, stored, which):
        if name == "count":
            out[name] = count_p(row, cnt)
        elif name == "last":
            a, b, T, r0, r1 = row
            out[name] = time_p((b, a, T, r0, r1), 1, T - np.asarray(sample["last"])[cnt >= 1])
        else:
            j = int(name[3])
            out[name] = time_p(row, j, np.asarray(sample[name])[cnt >= j])
    return out


def sample_of_paths(paths):
    """a list of arrays of jump times -> sample"""
    n = len(paths)
    s = dict(count=np.array([len(t) for t in paths]), tau1=np.full(n, np.nan), tau2=np.full(n, np.nan), last=np.full(n, np.nan))
    for i, t in enumerate(paths):
        if len(t) >= 1:
            s["tau1"][i], s["last"][i] = t[0], t[-1]
        if len(t) >= 2:
            s["tau2"][i] = t[1]
    return s


def check(tag, row, stats, n_statistics):
    """print every p-value, then the decision rule"""
    floor = ALPHA / n_statistics
    for name, (p, x, df) in sorted(stats.items()):
        print("%-10s %-40r %-6s p = %-12.4g chi2 = %.2f on %d" % (tag, row, name, p, x, df))
    for name, (p, x, df) in stats.items():
        assert p >= floor, (tag, row, name, p, floor)
    return min([v[0] for v in stats.values()] or [1.0])


# ---------------------------------------------------------------------------------------------------------
# the algorithm of run_direct (epv_direct.h) over many segments at once: numpy, libm's exp and log, numpy's generator --
# neither the device's bits nor its Philox stream.  `variant` breaks one line of it (the power of the statistics).
VARIANTS = ("keep-accepts-all", "w2-is-wb", "p0-swapped")


def model_direct(row, n, seed, variant=None):
    assert variant is None or variant in VARIANTS
    a0, end, T, r0, r1 = row
    rng = np.random.default_rng(seed)
    lam = r0 + r1
    a, base, nj, live = np.full(n, a0), np.zeros(n), np.zeros(n, np.int64), np.ones(n, bool)
    s_out = dict(count=nj, tau1=np.full(n, np.nan), tau2=np.full(n, np.nan), last=np.full(n, np.nan))
    for _ in range(4096):
        idx = np.flatnonzero(live)
        if not len(idx):
            break
        s = T - base[idx]
        ra, rb = np.where(a[idx] == 1, r1, r0), np.where(a[idx] == 1, r0, r1)
        ea, el = np.exp(-ra * s), np.exp(-lam * s)
        keep = a[idx] == end
        p0 = np.exp(-rb * s) / ((ra + rb * el) / lam) if variant == "p0-swapped" else ea / ((rb + ra * el) / lam)
        stop = keep & (1.0 - rng.random(len(idx)) < p0)
        live[idx[stop]] = False
        go = ~stop
        idx, s, ra, rb, ea, el, keep = idx[go], s[go], ra[go], rb[go], ea[go], el[go], keep[go]
        tau = np.zeros(len(idx))
        todo = np.ones(len(idx), bool)
        w1, wb = 1.0 - ea, 1.0 - np.exp(-rb * s)
        w2 = wb if variant == "w2-is-wb" else ea * wb
        wl = 1.0 - el
        for _ in range(4096):
            q = np.flatnonzero(todo)
            if not len(q):
                break
            u, v = rng.random(len(q)), rng.random(len(q))
            k = keep[q]
            t_keep = -np.log(1.0 - u * w1[q]) / ra[q]
            ok_keep = v * wl[q] < 1.0 - np.exp(-lam * (s[q] - t_keep))
            if variant == "keep-accepts-all":
                ok_keep = np.ones(len(q), bool)
            arm1 = u * (w1[q] + w2[q]) < w1[q]
            t_flip = np.where(arm1, -np.log(1.0 - v * w1[q]) / ra[q], s[q] - -np.log(1.0 - v * wb[q]) / rb[q])
            t = np.where(k, t_keep, t_flip)
            tn = base[idx[q]] + t
            ok = (t < s[q]) & (tn > base[idx[q]]) & (tn < T) & (ok_keep | ~k)
            tau[q[ok]] = t[ok]
            todo[q[ok]] = False
        assert not todo.any()
        base[idx] = base[idx] + tau
        a[idx] ^= 1
        nj[idx] += 1
        s_out["tau1"][idx[nj[idx] == 1]] = base[idx[nj[idx] == 1]]
        s_out["tau2"][idx[nj[idx] == 2]] = base[idx[nj[idx] == 2]]
        s_out["last"][idx] = base[idx]
    assert not live.any()
    return s_out
