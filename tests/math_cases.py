"""Inputs of the device numerics known-answer tests (test_device_math.py): the same arrays judge the oracle
against mpmath on the CPU and the device against the oracle on the GPU.  Plain numpy, fixed seeds.

Every function returns a dict name -> array; an array is one `math_kat` call, so none has more than MAX_ITEMS
rows.  Columns are the inputs of the op (include/epievo_mi355x.h, epv_math_kat)."""
import functools

import numpy as np

MAX_ITEMS = 1 << 18
LN2 = float(np.log(2.0))
SQRT_HALF = float(np.sqrt(0.5))           # 0x3fe6a09e667f3bcd: where epv_log splits the mantissa
EXP_OVERFLOW = 709.782712893384           # epv_exp returns inf above, 0 below EXP_UNDERFLOW
EXP_UNDERFLOW = -745.2
NOJUMP_CUT = 40.0                         # nojump_bound is 0 from here on
GUARD = 1e-4                              # ... and exp(-x) shrunk by this below


def step(x, j):
    """the double j places above x in the order of the reals (j < 0: below); -0 and +0 are one place"""
    i = np.array(x, np.float64).view(np.int64)
    key = np.where(i >= 0, i, -(i & np.int64(0x7fffffffffffffff))) + np.asarray(j, np.int64)
    back = np.where(key >= 0, key, (-key) | np.int64(-0x8000000000000000))
    return back.view(np.float64)


def lattice(centres, half=64):
    """the 2 half + 1 neighbouring doubles around every centre"""
    c = np.ascontiguousarray(centres, np.float64).reshape(-1, 1)
    return step(np.broadcast_to(c, (c.shape[0], 2 * half + 1)).copy(), np.arange(-half, half + 1)[None, :]).reshape(-1)


def loguniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 1e-300, -1e-300])
EXP_SEAM_K = np.arange(-1080, 1031)       # x = k ln2 / 2: odd k = where round(x / ln2) steps, even k = r ~ 0


@functools.lru_cache(maxsize=None)
def exp_sets():
    rng = np.random.RandomState(0)
    ranges = np.concatenate([rng.uniform(-40, 0, 1500), rng.uniform(-1e-3, 1e-3, 300),
                             -np.exp(rng.uniform(-30, 6, 700)), rng.uniform(0, 30, 300)])
    seams = lattice(EXP_SEAM_K * (LN2 / 2))
    cut = len(seams) // 2 // 129 * 129
    tails = np.concatenate([
        rng.uniform(EXP_UNDERFLOW, -708.0, 4096),                         # subnormal results: k < -1021
        lattice([EXP_UNDERFLOW, -1074.5 * LN2, -1074 * LN2, -1022.5 * LN2, -1022 * LN2, -1021.5 * LN2, -708.0]),
        rng.uniform(709.0, 709.79, 2048),                                 # k > 1023, and past the overflow cut
        lattice([1023.5 * LN2, EXP_OVERFLOW, 709.79]),
        SPECIALS])
    return {"exp_ranges": ranges, "exp_seams_lo": seams[:cut], "exp_seams_hi": seams[cut:], "exp_tails": tails}


LOG_SEAM_E = (-1074, -1060, -1030, -1023, -1022, -1021, -600, -53, -2, -1, 0, 1, 2, 52, 53, 600, 1022, 1023)
LOG_NEAR_ONE_J = 4096                     # 1 - 2^-53 j: the 1 - u of the draws next to 1


@functools.lru_cache(maxsize=None)
def log_sets():
    rng = np.random.RandomState(1)
    ranges = np.concatenate([rng.uniform(0, 1, 1500), 1.0 - np.exp(rng.uniform(-36, -1, 500)),
                             np.exp(rng.uniform(-700, 700, 500)), rng.uniform(0.5, 2.0, 500)])
    # 2^e sqrt(1/2) and 2^e sqrt(2) = 2^(e+1) sqrt(1/2): one mantissa, the seam of the split
    seam_centres = np.concatenate([np.ldexp(SQRT_HALF, np.array(LOG_SEAM_E)), np.ldexp(SQRT_HALF, np.array(LOG_SEAM_E) + 1)])
    seam_centres = seam_centres[np.isfinite(seam_centres) & (seam_centres > 0)]
    sub = []
    for b in range(52):                   # binade b of the subnormals: [2^b, 2^(b+1)) quanta of 2^-1074
        q = rng.randint(0, 1 << 30, 64).astype(np.int64) * (1 << 22) + rng.randint(0, 1 << 22, 64)
        q = (q % (1 << b)) + (1 << b)
        q[0], q[1] = 1 << b, (2 << b) - 1
        sub.append(q)
    sub = np.concatenate(sub).view(np.float64)
    near_one = 1.0 - np.ldexp(np.arange(LOG_NEAR_ONE_J, dtype=np.float64), -53)
    edges = np.concatenate([SPECIALS, [-1.0, -0.5, -1e300, np.ldexp(1.0, -1022), step(np.ldexp(1.0, -1022), -1),
                                       np.finfo(np.float64).max]])
    return {"log_ranges": ranges, "log_seams": np.concatenate([lattice(seam_centres), lattice([1.0])]),
            "log_subnormal": sub, "log_near_one": near_one, "log_edges": edges}


@functools.lru_cache(maxsize=None)
def nojump_sets():
    rng = np.random.RandomState(2)
    f = rng.uniform(0, 40, 1 << 15).astype(np.float32)
    f = f[f < np.float32(40.0)]
    assert len(f) == 1 << 15
    f = f.astype(np.float64)
    x = np.concatenate([f, step(f, -1), step(f, 1), loguniform(rng, 1e-300, 40, 1 << 15), rng.uniform(0, 40, 1 << 15),
                        step(np.full(256, NOJUMP_CUT), -np.arange(1, 257)), [NOJUMP_CUT, float(step(NOJUMP_CUT, 1)), 1e3, 0.0]])
    return {"nojump_x": x}


def model_rate_pairs():
    """(r0, r1) of the four neighbour contexts of test.param, of the two dense models and of the models of
    model_cases.py: rates[trip0], rates[trip0 | 2]"""
    import dense_cases
    import model_cases
    from common import ref_test_model
    out = []
    models = [ref_test_model(), dense_cases.model("weak"), dense_cases.model("flat")]
    models += [model_cases.model(name) for name in model_cases.MODELS if name != "ref"]
    for m in models:
        out += [(float(m.rates[t]), float(m.rates[t | 2])) for t in (0, 1, 4, 5)]
    return np.array(out)


MATRIX_FIXED_LEN = (0.0, 5e-324, 1e-300, 1e-12, 50.0, 400.0, 1e4)


@functools.lru_cache(maxsize=None)
def matrix_sets():
    """rows len, r0, r1: every length with every rate pair"""
    rng = np.random.RandomState(3)
    lens = np.concatenate([MATRIX_FIXED_LEN, loguniform(rng, 1e-6, 10, 25)])
    eq = loguniform(rng, 1e-6, 1e3, 6)
    big = loguniform(rng, 1e-3, 1e3, 6)
    pairs = np.concatenate([
        np.stack([eq, eq], 1), [[1.0, 1.0], [1e-6, 1e-6], [1e3, 1e3]],                  # r0 == r1
        np.stack([big, big * 1e-8], 1), np.stack([big * 1e-8, big], 1),                 # ratios 1e+-8
        model_rate_pairs(),
        np.stack([loguniform(rng, 1e-6, 1e3, 200), loguniform(rng, 1e-6, 1e3, 200)], 1)])
    L, P = np.meshgrid(lens, np.arange(len(pairs)), indexing="ij")
    return {"matrices": np.stack([L.reshape(-1), pairs[P.reshape(-1), 0], pairs[P.reshape(-1), 1]], 1)}


@functools.lru_cache(maxsize=None)
def draw_sets():
    """rows u, trunc, r (and T in column 3): trunc = 1 - exp(-r T) with the project's exp, formed as
    the kernels form it -- 1.0 - epv_exp(-(rate) * len)"""
    import orc
    rng = np.random.RandomState(4)
    j = np.arange(1, 4096, dtype=np.float64)
    u = np.concatenate([np.repeat([0.0, 2.0 ** -53, 0.5, 1.0 - 2.0 ** -53], 64), 1.0 - np.ldexp(j, -53), rng.uniform(0, 1, 4096)])
    r = loguniform(rng, 1e-6, 1e3, len(u))
    T = loguniform(rng, 1e-8, 10, len(u))
    trunc = 1.0 - orc.kat_exp_log(-(r) * T)[0]
    return {"draws": np.stack([u, trunc, r, T], 1)}


STAT_FIX_K = (-10, 0, 20, 45, 60)
STAT_TREES = ("tree", "pair", "bal16", "cat6", "multi", "star4", "cherry", "cat20")
STAT_GENOMES = (8, 4096, 10 ** 7)


def tree_stat_rows():
    """(T_b, 2^k_b) of every branch of the test trees at the k_b the oracle picks for each genome length"""
    import orc
    from common import config, ref_test_model
    from epievo_amd import host
    rows = []
    m = ref_test_model()
    for name in STAT_TREES:
        t = config(name)
        o = orc.Oracle(t, m, host.simulate(m, t, 8, 1), "B")
        for n in STAT_GENOMES:
            o.L.orc_set_shard(o.h, 0, n)
            sc = np.zeros(t.n_nodes)
            o.L.orc_stat_scales(o.h, orc._p(sc, orc.C.c_double))
            rows += [(float(t.branches[b]), float(sc[b])) for b in range(1, t.n_nodes)]
        o.close()
    return np.array(rows)


@functools.lru_cache(maxsize=None)
def stat_fix_sets():
    """rows dt, scale.  The products dt * scale below are exact (scale is a power of two), so the targets are
    what the rounding sees."""
    rng = np.random.RandomState(5)
    m = np.concatenate([[0, 1, 2, 3, 10, 11, 1 << 20, (1 << 20) + 1, 1 << 40, (1 << 40) + 1, 1 << 49, (1 << 49) + 1,
                         (1 << 50) - 2, (1 << 50) - 1], rng.randint(0, 1 << 25, 200).astype(np.int64) * (1 << 25) + rng.randint(0, 1 << 25, 200)])
    ties = m.astype(np.float64) + 0.5
    assert np.all(ties - m == 0.5) and ties.max() == 2.0 ** 50 - 0.5
    whole = np.concatenate([rng.randint(0, 1 << 25, 200).astype(np.int64) * (1 << 25) + rng.randint(0, 1 << 25, 200),
                            [0, 1, (1 << 50) - 1]]).astype(np.float64)
    frac = np.concatenate([rng.uniform(0, 2.0 ** 50 - 1, 300), loguniform(rng, 1e-3, 2.0 ** 50 - 1, 300), [0.25, 0.75, 1.25]])
    targets = np.concatenate([ties, step(ties, -1), step(ties, 1), whole, frac])
    targets = np.concatenate([targets, -targets])        # a difference of times is never negative; the rounding takes either sign
    rows = [np.stack([np.ldexp(targets, -k), np.full(len(targets), 2.0 ** k)], 1) for k in STAT_FIX_K]
    return {"stat_fix": np.concatenate(rows + [tree_stat_rows()])}


SHORTCUT_EPS = np.linspace(-2e-4, 2e-4, 257)
SHORTCUT_POINTS = 768


@functools.lru_cache(maxsize=None)
def shortcut_sets():
    """rows u, T, r around the edge of the no-jump shortcut: 1 - u = exp(-r T) (1 + eps), and the doubles next
    to exp(-r T); then products from the cut-off on, where the shortcut must stay silent"""
    rng = np.random.RandomState(6)
    x = loguniform(rng, 1e-6, 39.99, SHORTCUT_POINTS)
    r = loguniform(rng, 1e-6, 1e3, SHORTCUT_POINTS)
    T = x / r
    assert np.all(T * r < NOJUMP_CUT)
    w0 = np.exp(-(T * r))
    w = np.concatenate([w0[:, None] * (1.0 + SHORTCUT_EPS[None, :]),
                        step(np.repeat(w0[:, None], 17, 1), np.arange(-8, 9)[None, :])], 1)
    u = np.maximum(1.0 - w, 0.0)         # a draw is never negative
    rows = np.stack([u, np.broadcast_to(T[:, None], u.shape), np.broadcast_to(r[:, None], u.shape)], 2).reshape(-1, 3)
    xb = np.concatenate([[NOJUMP_CUT, float(step(NOJUMP_CUT, 1)), 41.0, 100.0, 745.0, 1e3, 1e6], rng.uniform(40, 80, 57)])
    rb = loguniform(rng, 1e-6, 1e3, len(xb))
    rb[:2] = 1.0                          # T r is the product itself at the cut-off and one place above
    Tb = xb / rb
    Tb = np.where(Tb * rb < NOJUMP_CUT, step(Tb, 1), Tb)
    assert np.all(Tb * rb >= NOJUMP_CUT)
    ub = np.array([1.0 - 2.0 ** -53, 1.0 - 2.0 ** -52, 1.0 - 1e-12, 0.5, 0.0])
    beyond = np.stack([np.tile(ub, len(xb)), np.repeat(Tb, len(ub)), np.repeat(rb, len(ub))], 1)
    return {"shortcut": np.concatenate([rows, beyond])}


def all_sets():
    out = {}
    for f in (exp_sets, log_sets, nojump_sets, matrix_sets, draw_sets, stat_fix_sets, shortcut_sets):
        out.update(f())
    for a in out.values():
        a.setflags(write=False)           # shared by every test: nobody edits them
    return out
