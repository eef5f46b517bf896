"""The law of the segment samplers against closed forms, CPU part (the helper and the decision rule: tests/segment_law.py;
the device: tests/test_segment_law_gpu.py).

  * the reference checks itself: the jump count's closed form against mpmath's expm of the counting chain's generator,
    its sum, its mean against the reference implementation's expectations (tests/golden/kat.npz), detailed balance,
    the survival functions' ends and monotony, one trial's success probability;
  * the table of settings holds what it should, and every condition on a row follows from the reference alone;
  * the Python restatement of the direct sampler (direct_ref.direct_segment) on every row, 40 000 draws;
  * the oracle's own segment sampler (orc_kat_end_cond_paths: Nielsen's first jump, forward rejection) on the rows
    its trial search can run, 40 000 draws: today's yardstick tied to the closed forms;
  * power: a numpy model of the direct sampler's algorithm passes every statistic at 2^18 draws per row, and each of
    three one-line variants of it is rejected.
Every p-value is printed; with M statistics in this module each must be at least 1e-6 / M."""
import ctypes as C
import functools
import os

import mpmath as mp
import numpy as np
import pytest

import segment_law as sl
from segment_law import ROWS, law

POWER_ROWS = ((1, 1, 2.0, 3.0, 0.4), (0, 1, 0.5, 1.3, 0.7), (0, 0, 3.0, 4.0, 0.5))
ORACLE_ROWS = tuple(r for r in ROWS if sl.trial_leg(r))


@functools.lru_cache(maxsize=None)
def n_statistics():
    """M of this module: the restatement and the model on every row, the oracle on its rows, the variants on theirs"""
    m = sum(len(sl.planned(r, sl.CPU_DRAWS, None)) for r in ROWS)
    m += sum(len(sl.planned(r, sl.CPU_DRAWS, None)) for r in ORACLE_ROWS)
    m += sum(len(sl.planned(r, sl.DRAWS, None)) for r in ROWS)
    m += len(sl.VARIANTS) * sum(len(sl.planned(r, sl.DRAWS, None)) for r in POWER_ROWS)
    return m


def _ids(rows):
    return ["%d%d-T%g-%g-%g" % r for r in rows]


# ---------------------------------------------------------------------------------------------------------
# the reference checks itself
SELF_ROWS = ((0, 0, 0.5, 1.3, 0.7), (1, 0, 0.05, 0.2, 5.0), (0, 1, 1.0, 20.0, 20.0), (1, 1, 0.3, 125.0, 1.7e-4),
             (0, 1, 1e-6, 1e-3, 1e-6), (1, 1, 1.0, 1e-9, 1e-9))


@pytest.mark.parametrize("row", SELF_ROWS, ids=_ids(SELF_ROWS))
def test_count_law_is_the_counting_chains_expm(row):
    L, K = law(*row), 12
    with mp.workdps(sl.DPS + 30):                 # (scaling and squaring loses digits at rate x T = 37)
        G = mp.zeros(K + 1, K + 1)
        for i in range(K + 1):
            q = L.r[L.a ^ (i & 1)]
            G[i, i] = -q
            if i < K:
                G[i, i + 1] = q
        for t in (L.T, L.T / 3):
            E = mp.expm(G * t, method="taylor")
            for i in range(K):                    # (the leading block of a triangular matrix's exponential is exact)
                got = L.count_at(i, t)
                # (expm is good to the working precision in absolute terms: its entries are below 1)
                assert abs(got - E[0, i]) <= mp.mpf(10) ** -35 * abs(E[0, i]) + mp.mpf(10) ** -70, (row, i, got, E[0, i])
                if i < 2:
                    assert abs(L.count01_at(i, t) - got) <= mp.mpf(10) ** -35 * got, (row, i)


@pytest.mark.parametrize("row", ROWS, ids=_ids(ROWS))
def test_pmf_sums_to_one_and_has_the_parity(row):
    pm = law(*row).pmf()
    assert abs(mp.fsum(pm) - 1) < mp.mpf(10) ** -30
    assert all(p == 0 for k, p in enumerate(pm) if (k & 1) != (row[0] != row[1]))
    assert all(p > 0 for k, p in enumerate(pm) if (k & 1) == (row[0] != row[1]))


def test_mean_count_is_the_reference_implementations_expectation():
    from common import GOLDEN
    g = np.load(os.path.join(GOLDEN, "kat.npz"))
    assert len(g["exp_grid"]) == 12
    for (r0, r1, T), e in zip(g["exp_grid"], g["exp_JD"]):
        J0, J1 = e[0:4].reshape(2, 2), e[4:8].reshape(2, 2)
        for a in (0, 1):
            for b in (0, 1):
                pm = law(a, b, float(T), float(r0), float(r1)).pmf()
                mean = float(mp.fsum(k * p for k, p in enumerate(pm)))
                want = J0[a, b] + J1[a, b]
                assert abs(mean - want) <= 1e-9 * want, (r0, r1, T, a, b, mean, want)


@pytest.mark.parametrize("row", ROWS, ids=_ids(ROWS))
def test_detailed_balance_of_the_joint_count(row):
    a, b, T, r0, r1 = row
    L, R = law(*row), law(b, a, T, r0, r1)
    with mp.workdps(sl.DPS):
        pi = (L.r[1] / L.l, L.r[0] / L.l)
        for k in range(12):
            x, y = pi[a] * L.joint(k), pi[b] * R.joint(k)
            assert abs(x - y) <= mp.mpf(10) ** -35 * abs(x), (row, k)


@pytest.mark.parametrize("row", ROWS, ids=_ids(ROWS))
def test_survival_decreases_from_one_to_the_mass_without_the_jump(row):
    L = law(*row)
    with mp.workdps(sl.DPS):
        for j in (1, 2):
            grid = [L.T * i / 64 for i in range(65)] + [L.T * mp.mpf(2) ** -e for e in (10, 30, 60)]
            grid += [L.T * (1 - mp.mpf(2) ** -e) for e in (10, 30, 60)]
            s = [L.survival(j, t) for t in sorted(grid)]
            assert abs(s[0] - 1) < mp.mpf(10) ** -40
            assert abs(s[-1] - L.fewer_than(j)) < mp.mpf(10) ** -35
            # (values of at most 1 from a few operations at 50 digits: steps below 1e-45 are rounding)
            assert all(x >= y - mp.mpf(10) ** -45 for x, y in zip(s, s[1:])), (row, j)
            if L.fewer_than(j) < 1 - mp.mpf(10) ** -30:
                assert s[0] > s[-1]


@pytest.mark.parametrize("row", [r for r in ROWS if r[0] != r[1]][::3])
def test_one_nielsen_trials_success_is_the_integral(row):
    """the integral of trial_success() is P_ab(T) / (1 - e^{-ra T}): the first jump falls below T, the rest ends in b"""
    L = law(*row)
    with mp.workdps(sl.DPS):
        want = L.trans(L.a, L.b, L.T) / -mp.expm1(-L.ra * L.T)
        assert abs(L.trial_success() - want) <= mp.mpf(10) ** -20 * want and 0 < want <= 1


# ---------------------------------------------------------------------------------------------------------
# the table
def test_table_holds_the_settings_it_should():
    from test_direct_sampler import LAW
    assert 20 <= len(ROWS) <= 40 and len(set(ROWS)) == len(ROWS)
    assert sl.LAW == LAW and set(LAW) <= set(ROWS)
    for T, r0, r1 in ((0.8, 4.2e4, 8.7e-6), (0.8, 8.7e-6, 4.2e4), (0.3, 125.0, 1.7e-4), (0.3, 1.7e-4, 125.0),
                      (1e-6, 1e-3, 1e-6)):
        assert {(a, b, T, r0, r1) for a in (0, 1) for b in (0, 1)} <= set(ROWS)
    # equal rates: state 1 is state 0 renamed, so (0, 0) and (0, 1) -- or their mirrors -- are all there is
    for T, r in ((1.0, 20.0), (1.0, 1e-9)):
        assert {r_[0] != r_[1] for r_ in ROWS if r_[2:] == (T, r, r)} == {False, True}
    assert set(POWER_ROWS) <= set(ROWS)
    # the device test interleaves a row that keeps its state with one that changes it
    assert {r[0] == r[1] for r in ROWS} == {False, True}


@pytest.mark.parametrize("row", ROWS, ids=_ids(ROWS))
def test_row_meets_the_conditions(row):
    """from the reference alone: nothing overflows the 64 slots, the last jump is used only where it is returned, the
    default sampler's leg only where 128 trials resolve every item"""
    L = law(*row)
    assert float(L.more_than(sl.KAT_SLOTS) * sl.DRAWS) < 0.01 and sl.row_conditions(row)
    plan = sl.planned(row, sl.DRAWS)
    assert plan[0] == "count"
    if "last" in plan:
        assert float(L.more_than(sl.KAT_TIMES) * sl.DRAWS) < 0.01
    for j in (1, 2):
        assert ("tau%d" % j in plan) == (float((1 - L.fewer_than(j)) * sl.DRAWS) >= 2000.0)
    if sl.trial_leg(row):
        a, b, T, r0, r1 = row
        assert min(r0, r1) > 1e-3 and T * max(r0, r1) <= 64.0
        with mp.workdps(sl.DPS):
            assert a == b or float(1 - mp.exp(-L.ra * L.T)) < 1.0
            p = L.trial_success()
            assert 0 < p <= 1 and float((1 - p) ** 128 * sl.DRAWS) < 0.01
        assert "last" not in sl.planned(row, sl.DRAWS, 2, sl.STATS[:3])


def test_default_samplers_leg_has_rows_of_both_kinds():
    assert {r[0] == r[1] for r in ORACLE_ROWS} == {False, True} and len(ORACLE_ROWS) >= 6


def _model_triples(name):
    """test_direct_sampler.model_space_segments() for one sampler model"""
    import model_cases as mc
    rates, out = mc.model(name).rates, set()
    lengths = [T for r in mc.ROWS if r[2] == name for T in np.round(mc.scaled_tree(r[3], r[4]).branches[1:], 12)]
    lengths += [T for _, sm, t, _ in mc.UNRUNNABLE if sm == name for T in mc.scaled_tree(t, 1).branches[1:]]
    for T in lengths:
        for trip0 in (0, 1, 4, 5):
            out.add((float(rates[trip0]), float(rates[trip0 | 2]), float(T)))
    return out


def test_model_rows_are_the_rules_choice():
    import model_cases as mc
    from test_direct_sampler import model_space_segments
    every = set(model_space_segments())
    assert len(sl.MODEL_ROWS) == len(mc.MODELS)
    for i, name in enumerate(mc.MODELS):
        mine = _model_triples(name) & every
        assert mine
        a, b = sl._AB[i % 4]
        for r0, r1, T in sorted(mine, key=lambda x: (-max(x[0], x[1]) * x[2], x)):
            if sl.row_conditions((a, b, T, r0, r1)):
                break
        else:
            raise AssertionError("no triple of %s meets the conditions" % name)
        assert sl.MODEL_ROWS[i] == (a, b, T, r0, r1), (name, sl.MODEL_ROWS[i], (a, b, T, r0, r1))


# ---------------------------------------------------------------------------------------------------------
# the restatement, and the oracle's sampler
@pytest.mark.parametrize("row", ROWS, ids=_ids(ROWS))
def test_restatement_draws_the_law(row):
    from direct_ref import MAX_ROOM, OK, direct_segment
    from test_trial_body import KAT_SEED
    a, b, T, r0, r1 = row
    paths = []
    for site in range(sl.CPU_DRAWS):
        oc, times, draws, longest = direct_segment(KAT_SEED, site, ROWS.index(row), 4, 0, a, b, T, r0, r1, MAX_ROOM, 0.0)
        assert oc == OK and longest <= 20
        paths.append(times)
    sl.check("restated", row, sl.statistics(row, sl.sample_of_paths(paths), None), n_statistics())


@pytest.mark.parametrize("row", ORACLE_ROWS, ids=_ids(ORACLE_ROWS))
def test_oracles_segment_sampler_draws_the_law(row):
    import orc
    a, b, T, r0, r1 = row
    n = sl.CPU_DRAWS
    cnt, tt = np.zeros(n, np.uint32), np.zeros(64 * n)
    tot = orc.orc_lib().orc_kat_end_cond_paths(orc.RNG_PHILOX, orc.MATH_EPV, 91, r0, r1, a, b, T, n,
                                               orc._p(cnt, C.c_uint32), orc._p(tt, C.c_double), len(tt))
    assert tot <= len(tt)
    off = np.concatenate(([0], np.cumsum(cnt.astype(np.int64))))
    paths = [tt[off[i]:off[i + 1]] for i in range(n)]
    sl.check("oracle", row, sl.statistics(row, sl.sample_of_paths(paths), None), n_statistics())


# ---------------------------------------------------------------------------------------------------------
# power
@pytest.mark.parametrize("row", ROWS, ids=_ids(ROWS))
def test_model_of_the_algorithm_passes(row):
    sample = sl.model_direct(row, sl.DRAWS, 1000 + ROWS.index(row))
    sl.check("model", row, sl.statistics(row, sample, None), n_statistics())


@pytest.mark.parametrize("variant", sl.VARIANTS)
def test_one_line_variant_is_rejected(variant):
    floor = sl.ALPHA / n_statistics()
    smallest = 1.0
    for row in POWER_ROWS:
        stats = sl.statistics(row, sl.model_direct(row, sl.DRAWS, 2000 + ROWS.index(row), variant), None)
        for name, (p, x, df) in sorted(stats.items()):
            print("%-18s %-26r %-6s p = %-12.4g chi2 = %.2f on %d" % (variant, row, name, p, x, df))
            smallest = min(smallest, p)
    assert smallest < floor, (variant, smallest, floor)
