"""The direct end-conditioned sampler (EPV_OPT_DIRECT_SAMPLER), CPU part: the restatement of
tests/direct_ref.py against cases worked out by hand, against the law (the oracle's own segment sampler,
orc_kat_end_cond_paths: forward rejection and Nielsen's method draw the same conditional law) and on the extremes
of the model space, where the trial search does not end.  The GPU part (tests/test_direct_sampler_gpu.py) pins the
device to this restatement bit for bit.  Nothing here runs the oracle's chain on model_cases.UNRUNNABLE."""
import ctypes as C
import functools

import numpy as np
import pytest

import model_cases as mc
import orc
from direct_ref import (GIVEUP, MAX_ROOM, OK, OVERFLOW, ROUNDS, direct_segment, draw, draw_address, exp_, stream)
from test_trial_body import KAT_SEED, block, first_draw, trunc_exp_time, trunc_of

BIG = MAX_ROOM


def _find(pred, a0, end, T, r0, r1, room=BIG, start=0.0, sweep=3, b=2, k=1, limit=4000):
    """the first site whose segment satisfies pred(result): (site, result)"""
    for site in range(limit):
        res = direct_segment(KAT_SEED, site, sweep, b, k, a0, end, T, r0, r1, room, start)
        if pred(res):
            return site, res
    raise AssertionError("no site found")


def _p0(ra, rb, s):
    lam = ra + rb
    return exp_(-ra * s) / ((rb + ra * exp_(-lam * s)) / lam)


# ---------------------------------------------------------------------------------------------------------
# hand-worked cases
def test_draw_addresses():
    s = (KAT_SEED, 77, 5, 9, 3)
    assert draw(*s, 0) == first_draw(*s, 1) == block(*s, 0, 0)[1]
    assert draw(*s, 1) == block(*s, 1, 0)[0] and draw(*s, 2) == block(*s, 1, 0)[1] and draw(*s, 3) == block(*s, 1, 1)[0]
    # draw 508 is the last of trial word 1 (block 253, second half), draw 509 the first of trial word 2
    assert draw_address(508) == (1, 253, 1) and draw_address(509) == (2, 0, 0) and draw_address(1017) == (3, 0, 0)
    assert draw(*s, 509) == block(*s, 2, 0)[0]
    seen = {draw_address(d) for d in range(1, 5000)}
    assert len(seen) == 4999                                   # no address is read twice
    assert max(a[1] for a in seen) == 253                      # block 255 (the trials' first draws) is never used
    u = stream(*s)
    assert [u(d) for d in (0, 1, 2, 3, 508, 509, 510)] == [draw(*s, d) for d in (0, 1, 2, 3, 508, 509, 510)]


def test_keep_without_a_jump():
    T, r0, r1 = 0.5, 1.3, 0.7
    site, res = _find(lambda r: r[2] == 1, 0, 0, T, r0, r1)
    u0 = draw(KAT_SEED, site, 3, 2, 1, 0)
    assert 1.0 - u0 < _p0(r0, r1, T)
    assert res == (OK, [], 1, 0)
    # p0 >= exp(-ra s): a draw that proves "no jump" to a proposal kernel (1 - u < the no-jump bound) stops here too
    assert _p0(r0, r1, T) >= exp_(-r0 * T) == 1.0 - trunc_of(0, T, r0, r1)
    # the other state's rate leaves state 1
    site, res = _find(lambda r: r[2] == 1, 1, 1, T, r0, r1)
    assert 1.0 - draw(KAT_SEED, site, 3, 2, 1, 0) < _p0(r1, r0, T) and res == (OK, [], 1, 0)


@pytest.mark.parametrize("arm", (1, 2))
def test_flip_by_each_mixture_arm(arm):
    T, r0, r1, start = 0.5, 1.3, 0.7, 0.25
    w1 = 1.0 - exp_(-r0 * T)
    wb = 1.0 - exp_(-r1 * T)
    w2 = exp_(-r0 * T) * wb

    for site in range(4000):
        u, v = draw(KAT_SEED, site, 3, 2, 1, 0), draw(KAT_SEED, site, 3, 2, 1, 1)
        if (u * (w1 + w2) < w1) != (arm == 1):
            continue
        res = direct_segment(KAT_SEED, site, 3, 2, 1, 0, 1, T, r0, r1, BIG, start)
        if res[0] == OK and len(res[1]) == 1:
            break
    else:
        raise AssertionError("no site found")
    tau = trunc_exp_time(v, w1, r0) if arm == 1 else T - trunc_exp_time(v, wb, r1)
    assert 0.0 < tau < T
    # draws: the arm, the inversion, then the keep decision of state 1 over what is left
    assert 1.0 - draw(KAT_SEED, site, 3, 2, 1, 2) < _p0(r1, r0, T - tau)
    assert res == (OK, [tau + start], 3, 1)


def test_keep_with_two_rejection_rounds():
    T, r0, r1 = 2.0, 3.0, 0.4
    site, res = _find(lambda r: r[0] == OK and r[3] == 2 and len(r[1]) == 2, 1, 1, T, r0, r1)
    d = [draw(KAT_SEED, site, 3, 2, 1, i) for i in range(9)]
    lam = r0 + r1
    # decisions in the order of the draws, by hand.  Draw 0: a jump follows
    assert not 1.0 - d[0] < _p0(r1, r0, T)
    w, wl = 1.0 - exp_(-r1 * T), 1.0 - exp_(-lam * T)
    taus = [trunc_exp_time(d[1], w, r1), trunc_exp_time(d[3], w, r1)]
    acc = [t < T and v * wl < 1.0 - exp_(-lam * (T - t)) for t, v in zip(taus, (d[2], d[4]))]
    if acc == [False, True]:          # the two rounds belong to the first jump
        t1 = taus[1]
        s = T - t1
        w1, wb = 1.0 - exp_(-r0 * s), 1.0 - exp_(-r1 * s)
        w2 = exp_(-r0 * s) * wb
        tau = trunc_exp_time(d[6], w1, r0) if d[5] * (w1 + w2) < w1 else s - trunc_exp_time(d[6], wb, r1)
        assert res[1] == [t1, t1 + tau] and res[2] == 8
        assert 1.0 - d[7] < _p0(r1, r0, T - (t1 + tau))
    else:                             # (the run of two came later in the segment)
        assert acc[0] and res[2] >= 8
    assert res[1][0] < res[1][1] < T


def test_room_overflows():
    T, r0, r1 = 0.5, 1.3, 0.7
    # a state change needs a jump: no room, no draw
    assert direct_segment(KAT_SEED, 5, 3, 2, 1, 0, 1, T, r0, r1, 0, 0.0) == (OVERFLOW, [], 0, 0)
    # a kept state overflows room 0 only when its first draw asks for a jump
    site, res = _find(lambda r: r[0] == OVERFLOW, 0, 0, T, r0, r1, room=0)
    assert res == (OVERFLOW, [], 1, 0) and not 1.0 - draw(KAT_SEED, site, 3, 2, 1, 0) < _p0(r0, r1, T)
    site0, res0 = _find(lambda r: r[0] == OK, 0, 0, T, r0, r1, room=0)
    assert res0 == (OK, [], 1, 0)
    # room 1: the kept state jumps once and must jump back; the flip's arm finds no room (no further draw)
    full = direct_segment(KAT_SEED, site, 3, 2, 1, 0, 0, T, r0, r1, BIG, 0.0)
    res1 = direct_segment(KAT_SEED, site, 3, 2, 1, 0, 0, T, r0, r1, 1, 0.0)
    assert full[0] == OK and len(full[1]) >= 2
    assert res1[0] == OVERFLOW and res1[1] == full[1][:1] and res1[2] == 1 + 2 * res1[3]
    # room 1 holds a flip of one jump; one of three jumps overflows after its first
    site, res = _find(lambda r: r[0] == OK and len(r[1]) == 3, 0, 1, 2.0, 3.0, 2.0)
    cut = direct_segment(KAT_SEED, site, 3, 2, 1, 0, 1, 2.0, 3.0, 2.0, 1, 0.0)
    assert cut[0] == OVERFLOW and cut[1] == res[1][:1]
    assert direct_segment(KAT_SEED, site, 3, 2, 1, 0, 1, 2.0, 3.0, 2.0, 3, 0.0) == res


def test_draw_509_moves_to_trial_word_2():
    # ~400 jumps: more than 508 draws, read through a recording stream
    s = (KAT_SEED, 11, 3, 2, 1)
    u, asked = stream(*s), []

    def rec(d):
        asked.append(d)
        return u(d)
    oc, times, draws, longest = direct_segment(*s, 0, 0, 1.0, 400.0, 400.0, BIG, 0.0, uniforms=rec)
    assert oc == OK and draws > 509 and asked == list(range(draws))        # in order, each once
    assert direct_segment(*s, 0, 0, 1.0, 400.0, 400.0, BIG, 0.0) == (oc, times, draws, longest)
    assert u(509) == block(*s, 2, 0)[0] and u(1017) == block(*s, 3, 0)[0]
    assert len(times) % 2 == 0 and all(x < y for x, y in zip(times, times[1:])) and times[-1] < 1.0


def test_nan_and_infinite_inputs_return():
    for T, r0, r1 in ((float("nan"), 1.0, 1.0), (0.5, float("nan"), 1.0), (0.5, 1.0, float("inf")),
                      (float("inf"), 1.0, 1.0)):
        for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)):
            oc, times, draws, longest = direct_segment(KAT_SEED, 3, 3, 2, 1, a, b, T, r0, r1, 8, 0.0)
            assert oc in (OK, OVERFLOW, GIVEUP) and len(times) <= 8 and draws <= 9 * (1 + 2 * ROUNDS)


# ---------------------------------------------------------------------------------------------------------
# the law: against the oracle's own segment sampler
LAW = ((0, 0, 0.5, 1.3, 0.7), (0, 1, 0.5, 1.3, 0.7), (1, 1, 2.0, 3.0, 0.4), (1, 0, 0.05, 0.2, 5.0), (0, 0, 3.0, 4.0, 0.5))
LAW_N = 40000


def _features(a, T, paths):
    """per path: jumps, jumps^2, no jump, time in state 1, its square, first jump time (nan without one)"""
    out = np.zeros((len(paths), 6))
    for i, t in enumerate(paths):
        n = len(t)
        edges = np.concatenate(([0.0], t, [T]))
        dwell = np.diff(edges)
        in1 = dwell[(1 - a)::2].sum()          # intervals 0, 2, .. are spent in a
        out[i] = (n, n * n, n == 0, in1, in1 * in1, t[0] if n else np.nan)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_paths(a, b, T, r0, r1):
    cnt, tt = np.zeros(LAW_N, np.uint32), np.zeros(64 * LAW_N)
    tot = orc.orc_lib().orc_kat_end_cond_paths(orc.RNG_PHILOX, orc.MATH_EPV, 91, r0, r1, a, b, T, LAW_N,
                                               orc._p(cnt, C.c_uint32), orc._p(tt, C.c_double), len(tt))
    assert tot <= len(tt)
    off = np.concatenate(([0], np.cumsum(cnt.astype(np.int64))))
    return [tt[off[i]:off[i + 1]] for i in range(LAW_N)]


@pytest.mark.parametrize("a,b,T,r0,r1", LAW)
def test_law_matches_the_oracles_segment_sampler(a, b, T, r0, r1):
    mine = []
    for site in range(LAW_N):
        oc, times, draws, longest = direct_segment(KAT_SEED, site, 1, 4, 0, a, b, T, r0, r1, BIG, 0.0)
        assert oc == OK and len(times) % 2 == (a != b) and longest <= 20
        mine.append(np.array(times))
    f, g = _features(a, T, mine), _features(a, T, _oracle_paths(a, b, T, r0, r1))
    for c, name in enumerate(("jumps", "jumps^2", "P(no jump)", "time in 1", "(time in 1)^2", "first jump")):
        x, y = f[:, c], g[:, c]
        x, y = x[~np.isnan(x)], y[~np.isnan(y)]
        if len(x) == 0 and len(y) == 0:
            continue
        se = np.sqrt(x.var(ddof=1) / len(x) + y.var(ddof=1) / len(y))
        print("%-14s direct %.6g  oracle %.6g  diff / se %.2f" % (name, x.mean(), y.mean(),
                                                                  (x.mean() - y.mean()) / se if se > 0 else 0.0))
        assert abs(x.mean() - y.mean()) <= 5.0 * se, (name, x.mean(), y.mean(), se)


# ---------------------------------------------------------------------------------------------------------
# extremes
def _check_segment(a, b, T, r0, r1, site, room=BIG):
    oc, times, draws, longest = direct_segment(KAT_SEED, site, 2, 7, 3, a, b, T, r0, r1, room, 0.0)
    assert oc == OK, (a, b, T, r0, r1, oc)                                  # finished, nothing gave up
    assert len(times) % 2 == (a != b)
    assert all(x < y for x, y in zip(times, times[1:])) and (not times or 0.0 < times[0] and times[-1] < T)
    assert longest <= 20
    return len(times), draws


def test_extreme_ratio_pair_and_its_mirror():
    # ratio's worst pair: forward rejection from 0 back to 0 needs about exp(4.2e4 x 0.8) trials
    for r0, r1 in ((4.2e4, 8.7e-6), (8.7e-6, 4.2e4)):
        for a in (0, 1):
            for b in (0, 1):
                for site in range(50):
                    nj, draws = _check_segment(a, b, 0.8, r0, r1, site)
                    assert nj <= 3 and draws <= 12
    nj, draws = _check_segment(0, 0, 0.8, 4.2e4, 8.7e-6, 0)
    assert nj == 2                                                          # out at once, back just before the end


def test_extreme_tiny_rate():
    for r0, r1, T in ((1e-9, 1e-9, 1.0), (2.0, 0.5, 1e-9 / 2.0), (1e-3, 1e-6, 1e-6)):
        for a in (0, 1):
            for b in (0, 1):
                for site in range(50):
                    nj, _ = _check_segment(a, b, T, r0, r1, site)
                    assert nj == (a != b)


def model_space_segments():
    """every (r0, r1) pair of a named model (the two rates of a context of the neighbours) at every distinct branch
    length of a row that samples under it"""
    out = set()
    for r in mc.ROWS:
        rates = mc.model(r[2]).rates
        for T in sorted(set(np.round(mc.scaled_tree(r[3], r[4]).branches[1:], 12))):
            for trip0 in (0, 1, 4, 5):
                out.add((float(rates[trip0]), float(rates[trip0 | 2]), float(T)))
    # the unrunnable row's own segments: ratio on the branches of tree (no oracle chain runs on it)
    for _, sm, t, _ in mc.UNRUNNABLE:
        rates = mc.model(sm).rates
        for T in mc.scaled_tree(t, 1).branches[1:]:
            for trip0 in (0, 1, 4, 5):
                out.add((float(rates[trip0]), float(rates[trip0 | 2]), float(T)))
    return sorted(out)


def test_extremes_of_the_model_space():
    segs = model_space_segments()
    assert len(segs) >= 100
    worst = 0.0
    for i, (r0, r1, T) in enumerate(segs):
        worst = max(worst, max(r0, r1) * T)
        for a in (0, 1):
            for b in (0, 1):
                _check_segment(a, b, T, r0, r1, i)
    assert worst > mc.EXP_UNDERFLOW


# ---------------------------------------------------------------------------------------------------------
# the single branch under `weak` of the GPU part's stationary-law test: what its length rests on.
# WEAK_T = 1.5 was chosen on the CPU: at rates 0.67 .. 1.33 a path then has about 1.5 jumps, a kept site jumps out and
# back more often than not, and orc_exact_posterior still keeps its 20 000 histories in about 1.9e6 trials of the
# 4e8 it may make (T = 1.0 gives a share of 0.34 of paths with two or more jumps, 1.5 gives 0.54, 2.0 gives 0.68).
WEAK_T = 1.5


def weak_model():
    import dense_cases as dc
    return dc.model("weak")


@functools.lru_cache(maxsize=None)
def weak_exact(want=20000):
    """test_mcmc_posterior._exact at WEAK_T under `weak`: means and standard errors of J and D over exact draws"""
    from test_mcmc_posterior import LEAF, ROOT
    m = weak_model()
    Jm, Dm, J2, D2 = (np.zeros(8) for _ in range(4))
    kept = orc.orc_lib().orc_exact_posterior(orc._p(m.rates, C.c_double), len(ROOT), orc._p(ROOT, C.c_uint8),
                                             orc._p(LEAF, C.c_uint8), WEAK_T, 3, want, 400000000,
                                             orc._p(Jm, C.c_double), orc._p(Dm, C.c_double), orc._p(J2, C.c_double),
                                             orc._p(D2, C.c_double))
    assert kept == want                                       # within its cap
    return Jm, Dm, np.sqrt(np.maximum(J2 - Jm ** 2, 1e-12) / want), np.sqrt(np.maximum(D2 - Dm ** 2, 1e-12) / want)


def weak_check(Jc, Dc, n_eff, exact):
    """test_mcmc_posterior._check with this branch's length in the conservation of time"""
    from test_mcmc_posterior import ROOT
    Jm, Dm, Jse, Dse = exact
    tolJ = 6.0 * (Jse * np.sqrt(20000.0 / n_eff) + 1e-3) + 0.01
    tolD = 6.0 * (Dse * np.sqrt(20000.0 / n_eff) + 1e-3) + 0.005
    assert np.all(np.abs(Jc - Jm) < tolJ), (Jc, Jm)
    assert np.all(np.abs(Dc - Dm) < tolD), (Dc, Dm)
    assert abs(Dc.sum() - (len(ROOT) - 2) * WEAK_T) < 1e-9


def weak_initial_paths():
    from epievo_amd import host
    from test_mcmc_posterior import LEAF, ROOT
    cnt = (ROOT != LEAF).astype(np.int64)
    off = np.zeros(len(ROOT) + 1, np.uint64)
    off[1:] = np.cumsum(cnt)
    return host.FlatPaths(len(ROOT), 2, ROOT.copy(), off, np.full(int(cnt.sum()), WEAK_T / 2))


def test_weak_branch_length_makes_the_keep_arm_matter():
    """at least a fifth of the exact draws' paths have two or more jumps.  orc_exact_posterior returns moments per
    context, not paths, so the share comes from the same whole-sequence rejection written out here (Gillespie over the
    interior sites from the root sequence, kept when it ends in the leaf sequence): 300 kept histories, 1 800 paths;
    a share of 0.2 would lie 25 of its standard errors below the 0.54 found."""
    from test_mcmc_posterior import LEAF, ROOT
    exact = weak_exact()
    assert exact[0].sum() > 2.0 * 1.2                        # far more jumps than the two observed flips
    r, n, rng = weak_model().rates, len(ROOT), np.random.RandomState(1)
    kept = ge2 = 0
    while kept < 300:
        seq, cnt, t = ROOT.astype(int), np.zeros(n, int), 0.0
        while True:
            rates = [r[4 * seq[s - 1] + 2 * seq[s] + seq[s + 1]] for s in range(1, n - 1)]
            t += rng.exponential(1.0 / sum(rates))
            if t >= WEAK_T:
                break
            x, k = rng.uniform() * sum(rates), 0
            while x >= rates[k] and k < n - 3:
                x -= rates[k]
                k += 1
            seq[k + 1] ^= 1
            cnt[k + 1] += 1
        if np.array_equal(seq, LEAF):
            kept += 1
            ge2 += int((cnt[1:-1] >= 2).sum())
    share = ge2 / (kept * (n - 2.0))
    print("share of paths with two or more jumps", share)
    assert share >= 0.2


def test_weak_branch_oracle_chain_matches_exact_posterior():
    """the criteria hold for the oracle's chain (default sampler) at this length: they are not too tight for it"""
    from epievo_amd import host
    o = orc.Oracle(host.Tree.single_branch(WEAK_T), weak_model(), weak_initial_paths(), "B", cap=48, seed=17)
    o.reset()
    J, D, nacc, acc = o.run_mcmc(500, 20000)
    weak_check(J, D, 2000.0, weak_exact())
    assert o.counters()["overflow"] == 0
