"""Known answers for the arithmetic under the MCMC kernels (epv_math_kat): epv_exp / epv_log, the segment
matrices, the two draw transforms, the fixed-point rounding of the statistics, and the float bound the
no-jump shortcut rests on -- each on the inputs of math_cases.py, where whole MCMC runs never go.

The unmarked tests hold the oracle's own functions against mpmath and exact integers on those inputs; the
GPU tests then demand the device's bits (and those of the library's host pass) equal the oracle's, and judge
the float bound, which the oracle has no counterpart of, with mpmath directly."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import math_cases as mc
import orc
from test_math_rng import _ulp_err

EXP_SETS = ("exp_ranges", "exp_seams_lo", "exp_seams_hi", "exp_tails")
LOG_SETS = ("log_ranges", "log_seams", "log_subnormal", "log_near_one", "log_edges")
DBL_MAX = float(np.finfo(np.float64).max)


def _mp(prec=200):
    import mpmath
    mpmath.mp.prec = prec
    return mpmath


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    """uint64 views equal; a NaN equals any NaN; +0 and -0 differ"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb])


# ------------------------------------------------------------------ the oracle's answers, computed once
@functools.lru_cache(maxsize=None)
def _oracle_exp_log(name):
    e, l = orc.kat_exp_log(mc.all_sets()[name])
    return e, l


@functools.lru_cache(maxsize=None)
def _oracle_matrices():
    m = mc.all_sets()["matrices"]
    return orc.kat_seg_matrices(m[:, 0], m[:, 1], m[:, 2])


@functools.lru_cache(maxsize=None)
def _oracle_draws():
    d = mc.all_sets()["draws"]
    return orc.kat_hold_time(d[:, 0], d[:, 2]), orc.kat_trunc_exp_time(d[:, 0], d[:, 1], d[:, 2])


@functools.lru_cache(maxsize=None)
def _exact_stat_fix():
    s = mc.all_sets()["stat_fix"]
    return np.array([round(Fraction(float(dt)) * Fraction(float(sc))) for dt, sc in s], dtype=np.int64)


# ------------------------------------------------------------------ CPU: the inputs are what they claim
def test_cases_cover_the_seams_and_stay_small():
    S = mc.all_sets()
    for name, a in S.items():
        assert 0 < a.shape[0] <= mc.MAX_ITEMS, name
    has = lambda a, v: bool(np.any(_bits(a) == _bits(np.array([v]))[0]))

    # exp: a lattice of 129 doubles around every k ln2 / 2, both values of round(x / ln2) at every odd k
    seams = np.concatenate([S["exp_seams_lo"], S["exp_seams_hi"]]).reshape(len(mc.EXP_SEAM_K), 129)
    assert np.array_equal(seams[:, 64], mc.EXP_SEAM_K * (mc.LN2 / 2))
    assert np.all(np.diff(seams[mc.EXP_SEAM_K != 0], axis=1) > 0)
    kr = seams * 1.44269504088896338700e+00
    k = (kr + np.where(seams < 0, -0.5, 0.5)).astype(np.int64)
    odd = mc.EXP_SEAM_K % 2 != 0
    assert np.all(k[odd].min(1) + 1 == k[odd].max(1)) and np.all(k[~odd].min(1) == k[~odd].max(1))
    t = S["exp_tails"]
    tk = t[np.isfinite(t)] / mc.LN2
    assert np.sum((tk < -1021.5) & (t[np.isfinite(t)] >= mc.EXP_UNDERFLOW)) >= 4096      # two-step scaling down
    assert np.sum((tk > 1023.5) & (t[np.isfinite(t)] <= mc.EXP_OVERFLOW)) >= 512         # ... and up
    assert np.any(t[np.isfinite(t)] > mc.EXP_OVERFLOW) and np.any(t < mc.EXP_UNDERFLOW)
    assert np.nanmin(t) <= -745.2 and np.sum((t >= 709.0) & (t <= 709.79)) >= 2048
    for v in mc.SPECIALS:
        assert (np.isnan(t).any() if v != v else has(t, v)), v
        assert (np.isnan(S["log_edges"]).any() if v != v else has(S["log_edges"], v)), v
    for r in ((-40, 0), (-1e-3, 1e-3), (-404, -1e-13), (0, 30)):
        assert np.sum((S["exp_ranges"] >= r[0]) & (S["exp_ranges"] <= r[1])) >= 300, r

    # log: the mantissa where epv_log splits, one place either side, over the exponents; 1.0; every subnormal binade
    ls = S["log_seams"]
    man = _bits(ls) & np.uint64(0x000fffffffffffff)
    ex = (_bits(ls) >> np.uint64(52)).astype(np.int64) & 0x7ff
    for d in (-1, 0, 1):
        at = man == np.uint64(0x6a09e667f3bcd + d)
        assert len(set(ex[at & (ls > 0)])) >= 15, d
        assert np.any(at & (ex == 0x3fe)) and np.any(at & (ex == 0x3ff))       # sqrt(1/2) and sqrt(2) themselves
    assert np.any(at & (ex == 1)) and np.any(at & (ex == 0x7fe))
    for j in range(-64, 65):
        assert has(ls, float(mc.step(1.0, j)))
    q = S["log_subnormal"].view(np.int64)
    assert np.all((q > 0) & (q < 1 << 52))
    assert np.array_equal(np.bincount([int(v).bit_length() - 1 for v in q], minlength=52), np.full(52, 64))
    n1 = S["log_near_one"]
    assert len(n1) == 4096 and np.array_equal((1.0 - n1) * 2.0 ** 53, np.arange(4096.0))
    e = S["log_edges"]
    assert np.sum(e < 0) >= 4 and has(e, np.inf) and has(e, DBL_MAX)
    assert np.sum(S["log_ranges"] < 1e-200) and np.sum(S["log_ranges"] > 1e200)

    # the no-jump bound: floats with both double neighbours, the doubles up to the cut-off, the cut-off, beyond
    x = S["nojump_x"]
    f = x[: 1 << 15]
    assert np.array_equal(f, f.astype(np.float32).astype(np.float64)) and len(np.unique(f)) > 32000
    assert np.array_equal(x[1 << 15: 2 << 15], np.nextafter(f, -np.inf)) and np.array_equal(x[2 << 15: 3 << 15], np.nextafter(f, np.inf))
    for j in range(-256, 2):
        assert has(x, float(mc.step(mc.NOJUMP_CUT, j))), j
    assert has(x, 1e3) and has(x, 0.0) and x.min() < 1e-290 and np.sum((x > 0) & (x < 1e-30)) > 1000

    # matrices: every length with every pair; equal rates, ratios of 1e8 either way, the models' own pairs
    m = S["matrices"]
    lens, pairs = np.unique(m[:, 0]), np.unique(m[:, 1:], axis=0)
    assert len(np.unique(m, axis=0)) == len(lens) * len(pairs)
    for v in mc.MATRIX_FIXED_LEN:
        assert v in lens
    assert np.sum((lens >= 1e-6) & (lens <= 10)) >= 20
    ratio = pairs[:, 0] / pairs[:, 1]
    assert np.sum(ratio == 1.0) >= 8 and np.sum(np.abs(ratio / 1e8 - 1) < 1e-9) >= 4 and np.sum(np.abs(ratio * 1e8 - 1) < 1e-9) >= 4
    for p in mc.model_rate_pairs():
        assert np.any(np.all(pairs == p, axis=1)), p
    xs = m[:, 0] * (m[:, 1] + m[:, 2])
    assert np.sum(xs > 745.2) > 100 and np.sum(xs > 709.8) > np.sum(xs > 745.2) and np.sum(xs == 0) >= len(pairs)

    # draws
    d = S["draws"]
    for v in (0.0, 2.0 ** -53, 0.5, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53 * 4095):
        assert has(d[:, 0], v), v
    assert np.all((d[:, 0] >= 0) & (d[:, 0] < 1)) and np.all((d[:, 1] > 0) & (d[:, 1] <= 1))
    assert d[:, 2].min() < 1e-5 and d[:, 2].max() > 100 and d[:, 3].min() < 1e-7 and d[:, 3].max() > 5

    # stat_fix: exact products; ties above even and odd integers, their neighbours, the 2^50 ceiling, 0, one quantum
    s = S["stat_fix"]
    for kk in mc.STAT_FIX_K:
        p = s[s[:, 1] == 2.0 ** kk]
        prod = p[:, 0] * p[:, 1]
        assert all(Fraction(float(a)) * Fraction(float(b)) == Fraction(float(c)) for a, b, c in zip(p[:, 0], p[:, 1], prod))
        tie = prod[prod % 1 == 0.5]
        assert np.sum(np.floor(tie) % 2 == 0) > 50 and np.sum(np.floor(tie) % 2 == 1) > 50
        for v in (0.0, 1.0, 0.5, 1.5, 2.0 ** 50 - 0.5, 2.0 ** 50 - 1, float(mc.step(2.5, -1)), float(mc.step(2.5, 1))):
            assert v in prod, (kk, v)
        assert prod.max() < 2.0 ** 50 and prod.min() > -2.0 ** 50 and np.sum(prod < 0) > 500
    tr = mc.tree_stat_rows()
    assert len(tr) > 100 and np.all(tr[:, 0] * tr[:, 1] < 2.0 ** 50) and len(np.unique(tr[:, 1])) >= 6

    # the shortcut's edge
    c = S["shortcut"]
    xs = c[:, 1] * c[:, 2]
    n_lat = mc.SHORTCUT_POINTS * (257 + 17)
    assert np.all(xs[:n_lat] < 39.995) and xs[:n_lat].min() < 1e-5 and np.all(xs[n_lat:] >= mc.NOJUMP_CUT)
    assert has(xs[n_lat:], 40.0) and has(xs[n_lat:], float(mc.step(40.0, 1)))
    assert len(mc.SHORTCUT_EPS) == 257 and mc.SHORTCUT_EPS[0] == -2e-4 and mc.SHORTCUT_EPS[-1] == 2e-4 and mc.SHORTCUT_EPS[128] == 0.0
    assert np.all((c[:, 0] >= 0) & (c[:, 0] <= 1))


# ------------------------------------------------------------------ CPU: the oracle against mpmath
def _ulp_err_clamped(got, x, fn):
    """_ulp_err with the ulp of a subnormal result: 2^-1074, the spacing of the doubles there (a double has
    fewer than 53 bits below 2^-1022, so 2^(e - 52) is not its ulp)"""
    mp = _mp()
    worst = 0.0
    for g, xi in zip(got, x):
        exact = fn(mp.mpf(float(xi)))
        ulp = mp.mpf(2) ** (max(mp.floor(mp.log(abs(exact), 2)), -1022) - 52)
        worst = max(worst, float(abs(mp.mpf(float(g)) - exact) / ulp))
    return worst


@pytest.mark.parametrize("name", EXP_SETS)
def test_oracle_exp_within_one_ulp(name):
    mp = _mp()
    x = mc.all_sets()[name]
    e = _oracle_exp_log(name)[0]
    nan = np.isnan(x)
    assert np.all(np.isnan(e[nan]))
    x, e = x[~nan], e[~nan]
    # a result past the largest double is inf, one that is representable is finite
    over = np.array([mp.exp(mp.mpf(float(v))) > mp.mpf(DBL_MAX) for v in x[x > 709.0]], dtype=bool)
    big = np.zeros(len(x), bool)
    big[x > 709.0] = over
    assert np.all(e[big] == np.inf) and np.all(np.isfinite(e[~big]))
    x, e = x[~big], e[~big]
    assert np.all(e[x == -np.inf] == 0.0)
    keep = x != -np.inf
    x, e = x[keep], e[keep]
    sub = x < -708.0
    assert _ulp_err(e[~sub], x[~sub], mp.exp) < 1.0
    if sub.any():
        assert _ulp_err_clamped(e[sub], x[sub], mp.exp) < 1.0


@pytest.mark.parametrize("name", LOG_SETS + ("exp_tails",))
def test_oracle_log_within_one_ulp(name):
    mp = _mp()
    x = mc.all_sets()[name]
    l = _oracle_exp_log(name)[1]
    assert np.all(np.isnan(l[np.isnan(x) | (x < 0)]))
    assert np.all(l[x == 0] == -np.inf) and np.all(l[x == np.inf] == np.inf)
    ok = (x > 0) & np.isfinite(x)
    assert np.all(l[ok & (x == 1.0)] == 0.0) and not np.any(np.signbit(l[ok & (x == 1.0)]))
    assert _ulp_err(l[ok], x[ok], mp.log) < 1.0


def test_oracle_exp_log_special_values():
    """test_exp_log_special_values' expectations through the array entry the GPU tests compare with"""
    e, l = orc.kat_exp_log(np.array([0.0, -0.0, 1.0, -1e4, 1e4, np.inf, -np.inf, np.nan, -1.0, -740.0, 5e-324, -5e-324]))
    assert e[0] == 1.0 and e[1] == 1.0 and l[2] == 0.0 and e[3] == 0.0 and e[4] == np.inf
    assert e[5] == np.inf and e[6] == 0.0 and np.isnan(e[7]) and np.isnan(l[7])
    assert l[0] == -np.inf and l[1] == -np.inf and np.isnan(l[8]) and l[5] == np.inf and np.isnan(l[6])
    assert 0 < e[9] < 1e-300 and abs(l[10] - np.log(5e-324)) < 1e-12 * 745 and np.isnan(l[11])
    assert e[10] == 1.0 and e[11] == 1.0


def _mp_matrices(rows):
    mp = _mp()
    out = np.zeros((len(rows), 4), dtype=object)
    for i, (t, r0, r1) in enumerate(rows):
        t, r0, r1 = mp.mpf(float(t)), mp.mpf(float(r0)), mp.mpf(float(r1))
        h = mp.exp(-t * (r0 + r1))
        p00, p11 = (r0 * h + r1) / (r0 + r1), (r0 + r1 * h) / (r0 + r1)
        out[i] = (p00, p11, p00, 1 - p11)
    return out


def test_oracle_matrices_against_mpmath():
    """absolute error of P00, P11 (trans_prob_mat: h = 1 / exp) and PT00, PT10 (get_trans_prob: h = exp(-.);
    PT10 = 1 - prob loses relative accuracy by cancellation, so all four are judged on absolute error)"""
    mp = _mp()
    rows = mc.all_sets()["matrices"]
    got = _oracle_matrices()
    assert np.all(np.isfinite(got)) and np.all((got >= 0) & (got <= 1))
    want = _mp_matrices(rows)
    worst = [max(float(abs(mp.mpf(float(g)) - w)) for g, w in zip(got[:, j], want[:, j])) for j in range(4)]
    print("oracle matrices, worst absolute error of P00, P11, PT00, PT10 against mpmath:", worst)
    # measured against mpmath on these rows: P00 2.82e-16, P11 2.91e-16, PT00 2.77e-16, PT10 2.81e-16
    for j, recorded in enumerate((2.82e-16, 2.91e-16, 2.77e-16, 2.81e-16)):
        assert worst[j] < 2 * recorded, (j, worst)


# worst errors of the oracle's draw transforms against mpmath on the rows of math_cases.draw_sets(), as measured by
# the test below: of the time itself, and of rate * time (the exponential variate, which is what rounds)
RECORDED_DRAWS = {"hold": 3.21e-9, "first": 5.10e-11, "rate * hold": 6.30e-15, "rate * first": 3.83e-14,
                  "rate * first, 1 - u trunc < 2^-10": 4.33e-13}


def test_oracle_draw_transforms_against_mpmath():
    """-log(1 - u) / r and -log(1 - u trunc) / r against the real-valued expressions of the same inputs, on absolute
    error.  The times span thirty decades with the rates, so the error of rate * time is recorded as well.  u trunc
    and 1 - u trunc each round once on the scale of 1, which the logarithm magnifies by 1 / (1 - u trunc): the
    reference evaluates the same expression, so it is the sampler's law, and the draws with 1 - u trunc < 2^-10 are
    judged on their own."""
    mp = _mp()
    d = mc.all_sets()["draws"]
    hold, first = _oracle_draws()
    assert not np.any(np.isnan(hold)) and not np.any(np.isnan(first)) and np.all(hold >= 0) and np.all(first >= 0)
    worst = dict.fromkeys(RECORDED_DRAWS, 0.0)
    for (u, tr, r, _), h, f in zip(d, hold, first):
        u, tr, r = mp.mpf(float(u)), mp.mpf(float(tr)), mp.mpf(float(r))
        dh, df = abs(mp.mpf(float(h)) + mp.log(1 - u) / r), abs(mp.mpf(float(f)) + mp.log(1 - u * tr) / r)
        key = "rate * first" if 1 - u * tr >= mp.mpf(2) ** -10 else "rate * first, 1 - u trunc < 2^-10"
        for k, v in (("hold", dh), ("first", df), ("rate * hold", dh * r), (key, df * r)):
            worst[k] = max(worst[k], float(v))
    print("oracle draw transforms, worst absolute error against mpmath:", worst)
    for k, recorded in RECORDED_DRAWS.items():
        assert worst[k] < 2 * recorded, (k, worst)


def test_oracle_stat_fix_is_round_half_even():
    s = mc.all_sets()["stat_fix"]
    got = orc.kat_stat_fix(s[:, 0], s[:, 1])
    assert np.array_equal(got, _exact_stat_fix())


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dev():
    from epievo_amd.sampler import DeviceSampler
    d = DeviceSampler(0)
    yield d
    d.close()


def _both(dev, op, items, n_out):
    """the op in its own kernel and in the library's host pass; the slots past the op's outputs are zero"""
    k, h = dev.math_kat(op, items, 0), dev.math_kat(op, items, 1)
    assert k.shape == (len(items), 6) and not np.any(_bits(k[:, n_out:])) and not np.any(_bits(h[:, n_out:]))
    return k, h


@pytest.mark.gpu
@pytest.mark.parametrize("name", EXP_SETS + LOG_SETS)
def test_device_exp_log_bits(dev, name):
    x = mc.all_sets()[name]
    k, h = _both(dev, 0, x, 2)
    e, l = _oracle_exp_log(name)
    for got in (k, h):
        assert _same_bits(got[:, 0], e) and _same_bits(got[:, 1], l)


@pytest.mark.gpu
def test_device_matrices_bits(dev):
    rows = mc.all_sets()["matrices"]
    k, h = dev.math_kat(2, rows, 0), dev.math_kat(2, rows, 1)
    want = _oracle_matrices()
    assert _same_bits(k[:, :4], want) and _same_bits(h[:, :4], want)
    assert not np.any(_bits(h[:, 4:]))


@pytest.mark.gpu
def test_device_draw_transforms_bits(dev):
    d = mc.all_sets()["draws"]
    hold, first = _oracle_draws()
    for op, items, want in ((3, d[:, [0, 2]], hold), (4, d[:, :3], first)):
        k, h = _both(dev, op, items, 1)
        assert _same_bits(k[:, 0], want) and _same_bits(h[:, 0], want), op


@pytest.mark.gpu
def test_device_stat_fix_bits(dev):
    s = mc.all_sets()["stat_fix"]
    k, h = _both(dev, 5, s, 1)
    want = orc.kat_stat_fix(s[:, 0], s[:, 1])
    for got in (k, h):
        assert np.array_equal(got[:, 0].copy().view(np.int64), want)
        assert np.array_equal(got[:, 0].copy().view(np.int64), _exact_stat_fix())


def _judge_bound(x, b):
    """the proof obligation of the no-jump shortcut, mpmath the judge, no tolerance: for x >= 40 the bound is 0;
    below, exp(-x) (1 - 2e-4) <= b <= exp(-x) (1 - 2^-40).  The upper limit: the exact test the bound stands in for,
    !(-log(1 - u) / rate < T), is one epv_log (< 1 ulp), one division and the rounding of len * rate on an
    exponent of at most 40 -- below 2^-44 relative in 1 - u.  The lower limit: the 1e-4 guard and as much again
    for the float error it was sized for; it catches a shortcut that stops firing.
    Returns the worst relative error of b / 0.9999 against exp(-x)."""
    mp = _mp(120)
    x, b = np.asarray(x, np.float64), np.asarray(b, np.float64)
    assert x.shape == b.shape and not np.any(np.isnan(x))
    assert not np.any(_bits(b[x >= mc.NOJUMP_CUT])), "a bound from the float exp at x >= 40"
    hi, lo, shrink = 1 - mp.mpf(2) ** -40, 1 - mp.mpf(2) / 10000, mp.mpf(9999) / 10000
    xs, first = np.unique(x[x < mc.NOJUMP_CUT], return_index=True)
    exact = {float(v): mp.exp(-mp.mpf(float(v))) for v in xs}
    worst, above, below = mp.mpf(0), [], []
    for xi, bi in zip(x[x < mc.NOJUMP_CUT], b[x < mc.NOJUMP_CUT]):
        E, bm = exact[float(xi)], mp.mpf(float(bi))
        if bm > E * hi:
            above.append((float(xi), float(bi), float(bm / E - 1)))
        if bm < E * lo:
            below.append((float(xi), float(bi), float(bm / E - 1)))
        worst = max(worst, abs(bm / shrink - E) / E)
    assert not above, "bound above exp(-x) (1 - 2^-40): (x, b, b / exp(-x) - 1) = %s" % above[:8]
    assert not below, "bound below exp(-x) (1 - 2e-4): (x, b, b / exp(-x) - 1) = %s" % below[:8]
    return float(worst)


@pytest.mark.gpu
def test_device_nojump_bound_is_below_exp(dev):
    """Measured on gfx950 by this test: the worst relative error of the float exponential under the bound,
    |b / 0.9999 - exp(-x)| / exp(-x) over every x of the set, is 3.72e-6 (printed below; DESIGN.md and the comment
    above run_trial in epv_kernels.h quote it)."""
    x = mc.all_sets()["nojump_x"]
    out = dev.math_kat(1, x, 0)
    assert not np.any(_bits(out[:, 1:]))
    worst = _judge_bound(x, out[:, 0])
    print("nojump_bound: worst relative error of b / 0.9999 against exp(-x) over %d x: %.3e" % (len(x), worst))


@pytest.mark.gpu
def test_device_matrix_bounds_are_below_exp(dev):
    """the bounds epv_seg_matrices hands out with the matrices: x = len * r0 and len * r1 in fp64, as formed there"""
    rows = mc.all_sets()["matrices"]
    out = dev.math_kat(2, rows, 0)
    x = np.concatenate([rows[:, 0] * rows[:, 1], rows[:, 0] * rows[:, 2]])
    worst = _judge_bound(x, np.concatenate([out[:, 4], out[:, 5]]))
    print("epv_seg_matrices: worst relative error of bound / 0.9999 against exp(-x) over %d x: %.3e" % (len(x), worst))


@pytest.mark.gpu
def test_device_shortcut_never_contradicts_the_exact_test(dev):
    """on the lattice around 1 - u = exp(-r T): the shortcut firing implies the exact test's "no jump"; it fires
    wherever 1 - u (the fp64 difference the kernel forms) is below exp(-r T) (1 - 2e-4) -- every lattice point
    with eps <= -2e-4 that the spacing of the draws lets stand there -- and never at r T >= 40"""
    mp = _mp(120)
    c = mc.all_sets()["shortcut"]
    out = dev.math_kat(6, c, 0)
    assert not np.any(_bits(out[:, 2:])) and np.all((out[:, :2] == 0.0) | (out[:, :2] == 1.0))
    fires, exact = out[:, 0] == 1.0, out[:, 1] == 1.0
    bad = np.flatnonzero(fires & ~exact)
    assert len(bad) == 0, "shortcut fired where -log(1 - u) / r < T: (u, T, r) = %s" % c[bad[:8]].tolist()
    x = c[:, 1] * c[:, 2]
    assert not np.any(fires[x >= mc.NOJUMP_CUT])
    # must fire: 1 - u < exp(-x) (1 - 2e-4).  fp64 decides away from the threshold, mpmath next to it
    w = 1.0 - c[:, 0]
    lo = 1 - mp.mpf(2) / 10000
    thr = {float(v): mp.exp(-mp.mpf(float(v))) * lo for v in np.unique(x[x < mc.NOJUMP_CUT])}
    thr_f = np.array([float(thr[float(v)]) if v < mc.NOJUMP_CUT else 0.0 for v in x])
    must = w < thr_f * (1 - 1e-12)
    for i in np.flatnonzero((w >= thr_f * (1 - 1e-12)) & (w <= thr_f * (1 + 1e-12)) & (x < mc.NOJUMP_CUT)):
        must[i] = mp.mpf(float(w[i])) < thr[float(x[i])]
    # ... and the lattice's own eps = -2e-4 column wherever a draw can stand there: u is a multiple of 2^-53, which
    # moves 1 - u by less than 1e-5 of exp(-x) -- a tenth of what the guard leaves below that column -- for x <= 25
    n_lat = mc.SHORTCUT_POINTS * 274
    eps_col = np.tile(np.concatenate([mc.SHORTCUT_EPS, np.full(17, 0.0)]), mc.SHORTCUT_POINTS)
    column = np.zeros(len(c), bool)
    column[:n_lat] = (eps_col <= -2e-4) & (x[:n_lat] <= 25.0)
    assert column.sum() == np.sum(x[:n_lat:274] <= 25.0) > mc.SHORTCUT_POINTS // 2
    must |= column
    silent = np.flatnonzero(must & ~fires)
    assert len(silent) == 0, "shortcut silent below exp(-x) (1 - 2e-4): (u, T, r) = %s" % c[silent[:8]].tolist()
    print("shortcut lattice: %d points, fired on %d, required on %d, exact no-jump on %d"
          % (len(c), fires.sum(), must.sum(), exact.sum()))


@pytest.mark.gpu
def test_math_kat_rejects_what_it_cannot_do(dev):
    from epievo_amd.sampler import EPV_ERR_ARG, EpvError
    for op, where in ((7, 0), (0, 2), (1, 1), (6, 1)):
        with pytest.raises(EpvError) as e:
            dev.math_kat(op, np.zeros(4), where)
        assert e.value.code == EPV_ERR_ARG
