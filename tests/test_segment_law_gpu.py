"""The law of the segment samplers against closed forms, on the device (the reference, the statistics and the decision
rule: tests/segment_law.py; its self-checks, the rows' conditions and the CPU legs: tests/test_segment_law.py).

  * the direct end-conditioned sampler (run_direct through epv_direct_kat): 2^18 draws per row of segment_law.ROWS in
    calls of 65 536 items; item i has site i, the row's index as sweep, room 64, first draw index 0.  A call interleaves
    a row that keeps its state with one that changes it, so the lanes of a wave mix both arms.  One row starts at 0.25,
    taken off again before the comparison.  Every outcome is OK (no overflow, nothing gave up: the rows' conditions
    rule both out) and no jump took more than 20 rounds.  Statistics: the jump count, tau_1, tau_2, and the last jump
    where the entry's eight times hold it;
  * the default sampler (Nielsen's first jump, forward rejection, through epv_trial_kat's scan over 8 trials) on the
    rows segment_law.trial_leg() admits: trials 1 .. 8, then 9 .. 16 for the items that failed, ... at most 16 groups;
    no item is left unresolved.  Statistics: the jump count and the first two times of the winning trial.
Every p-value is printed; with M statistics in this module each must be at least 1e-6 / M."""
import functools

import numpy as np
import pytest

import segment_law as sl
from segment_law import DRAWS, ROWS

pytestmark = pytest.mark.gpu

CALL = 1 << 16
NODE, SEGMENT = 4, 0
START_ROW, START = 1, 0.25
KEEP = [i for i, r in enumerate(ROWS) if r[0] == r[1]]
CHANGE = [i for i, r in enumerate(ROWS) if r[0] != r[1]]
TRIAL_ROWS = [i for i, r in enumerate(ROWS) if sl.trial_leg(r)]
TRIAL_STATS = sl.STATS[:3]


def _pairs(keep, change):
    """row -> (a row that keeps its state, one that changes it), the row among them; mates share a pair"""
    out = {}
    for j, i in enumerate(keep):
        out[i] = (i, change[j % len(change)])
    for j, i in enumerate(change):
        out[i] = (keep[j % len(keep)], i)
    return out


DIRECT_PAIR = _pairs(KEEP, CHANGE)
TRIAL_PAIR = _pairs([i for i in TRIAL_ROWS if i in KEEP], [i for i in TRIAL_ROWS if i in CHANGE])


def _in_pair_order(pairs):
    """the rows with mates next to each other: the second finds the pair's draws still cached"""
    return sorted(pairs, key=lambda i: (pairs[i], i))


def _id(i):
    return "%d-%d%d-T%g-%g-%g" % ((i,) + ROWS[i])


@functools.lru_cache(maxsize=None)
def n_statistics():
    return (sum(len(sl.planned(r, DRAWS)) for r in ROWS)
            + sum(len(sl.planned(ROWS[i], DRAWS, 2, TRIAL_STATS)) for i in TRIAL_ROWS))


@pytest.fixture(scope="module")
def dev():
    from epievo_amd.sampler import DeviceSampler
    d = DeviceSampler(0)
    yield d
    d.close()


def _pair_items(pair, words, reals):
    """[2 DRAWS, 8] item words and the reals of a pair, the two rows alternating; site = the draw's index in its row"""
    items, re = np.zeros((2 * DRAWS, 8), np.uint32), np.zeros((2 * DRAWS, len(reals(pair[0]))))
    for lane, i in enumerate(pair):
        items[lane::2, 0] = np.arange(DRAWS)
        items[lane::2, 1:] = [i, NODE, SEGMENT] + list(words(i))
        re[lane::2] = reals(i)
    return items, re


# ---------------------------------------------------------------------------------------------------------
# the direct sampler
_direct_cache = {}


def _direct_draws(dev, pair):
    """-> {row: sample} of the pair's two rows, checked for outcome and rounds"""
    from direct_ref import OK
    from test_trial_body import KAT_SEED
    if pair in _direct_cache:
        return _direct_cache[pair]
    _direct_cache.clear()

    def words(i):
        return sl.KAT_SLOTS, ROWS[i][0] | ROWS[i][1] << 1, 0, 0

    def reals(i):
        return ROWS[i][2], ROWS[i][3], ROWS[i][4], START if i == START_ROW else 0.0
    items, re = _pair_items(pair, words, reals)
    w, t = np.zeros((2 * DRAWS, 4), np.uint32), np.zeros((2 * DRAWS, 8))
    for c in range(0, 2 * DRAWS, CALL):
        w[c:c + CALL], t[c:c + CALL] = dev.direct_kat(KAT_SEED, items[c:c + CALL], re[c:c + CALL])
    out = {}
    for lane, i in enumerate(pair):
        wi, ti = w[lane::2], t[lane::2] - reals(i)[3]
        assert np.all(wi[:, 0] == OK), (ROWS[i], np.bincount(wi[:, 0]))              # no overflow, nothing gave up
        assert wi[:, 3].max() <= 20, (ROWS[i], wi[:, 3].max())
        nj = wi[:, 1].astype(np.int64)
        # (the last jump is read only where segment_law.last_allowed says all jumps are among the eight times)
        out[i] = dict(count=nj, tau1=ti[:, 0], tau2=ti[:, 1], last=ti[np.arange(DRAWS), np.clip(nj, 1, sl.KAT_TIMES) - 1])
    _direct_cache[pair] = out
    return out


@pytest.mark.parametrize("i", _in_pair_order(DIRECT_PAIR), ids=_id)
def test_direct_sampler_draws_the_law(dev, i):
    pair = DIRECT_PAIR[i]
    assert ROWS[pair[0]][0] == ROWS[pair[0]][1] and ROWS[pair[1]][0] != ROWS[pair[1]][1] and i in pair
    sample = _direct_draws(dev, pair)[i]
    assert len(sample["count"]) == DRAWS
    sl.check("direct", ROWS[i], sl.statistics(ROWS[i], sample), n_statistics())


# ---------------------------------------------------------------------------------------------------------
# the default sampler
_trial_cache = {}


def _trial_draws(dev, pair):
    from test_trial_body import FAIL, KAT_SEED, NO_ROOM_LIMIT, OK, trunc_of
    if pair in _trial_cache:
        return _trial_cache[pair]
    _trial_cache.clear()

    def words(i):
        return 1, NO_ROOM_LIMIT, ROWS[i][0] | ROWS[i][1] << 1 | 4, 0

    def reals(i):
        a, b, T, r0, r1 = ROWS[i]
        return T, r0, r1, trunc_of(a, T, r0, r1) if a != b else 0.0, 0.5, 0.0
    items, re = _pair_items(pair, words, reals)
    assert np.all(re[:, 3] < 1.0)
    nj, times = np.zeros(2 * DRAWS, np.int64), np.zeros((2 * DRAWS, 2))
    pending = np.arange(2 * DRAWS)
    for group in range(sl.TRIAL_GROUPS):
        items[:, 4] = 1 + sl.TRIAL_WINDOW * group
        failed = []
        for c in range(0, len(pending), CALL):
            q = pending[c:c + CALL]
            W, _, tt = dev.trial_kat(KAT_SEED, items[q], re[q])
            oc = W[:, 4, 0]                                                          # scan_trials over 8 trials
            assert np.all((oc == OK) | (oc == FAIL)), np.bincount(oc)
            won = oc == OK
            assert np.all((W[won, 4, 1] >= items[q[won], 4]) & (W[won, 4, 1] < items[q[won], 4] + sl.TRIAL_WINDOW))
            nj[q[won]], times[q[won]] = W[won, 4, 2], tt[won, 4]
            failed.append(q[~won])
        pending = np.concatenate(failed)
        if not len(pending):
            break
    assert len(pending) == 0, "%d items unresolved after %d trials" % (len(pending), sl.TRIAL_GROUPS * sl.TRIAL_WINDOW)
    out = {i: dict(count=nj[lane::2], tau1=times[lane::2, 0], tau2=times[lane::2, 1]) for lane, i in enumerate(pair)}
    _trial_cache[pair] = out
    return out


@pytest.mark.parametrize("i", _in_pair_order(TRIAL_PAIR), ids=_id)
def test_default_sampler_draws_the_law(dev, i):
    pair = TRIAL_PAIR[i]
    assert ROWS[pair[0]][0] == ROWS[pair[0]][1] and ROWS[pair[1]][0] != ROWS[pair[1]][1] and i in pair
    sample = _trial_draws(dev, pair)[i]
    sl.check("default", ROWS[i], sl.statistics(ROWS[i], sample, 2, TRIAL_STATS), n_statistics())
