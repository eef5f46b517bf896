"""The trial evaluator of the end-conditioned sampler (run_trial, scan_trials, first_draw in epv_kernels.h)
evaluates, in the fused colour phase, ONE Philox block for a trial's first draw, whichever trial it is, and the
grouped search evaluates its one trial per lane without the scan's loop (scan_trial1).  Which blocks are read,
which operations make a value and their order stay what they were; the restatement below knows neither form, only
the law (so it also held the one-loop run_trial that was tried and not kept).  This file is the CPU part:

  * a restatement of one trial and of the scan over trials in Python: Philox4x32-10 with the counter layout of
    epv_philox.h, hold times and the truncated first jump through the oracle's known-answer entries
    (orc.kat_hold_time / orc.kat_trunc_exp_time), so the bits are the oracle's; sums are IEEE doubles.  The
    no-jump shortcut is execution only and has no place in it;
  * the restatement against cases worked out by hand (Philox against the published vectors of Random123);
  * the case generator of the GPU part (tests/test_trial_body_gpu.py) and what it claims to cover;
  * what the GPU part's whole runs rest on, from the oracle alone: flips and keepers, second trials, overflow
    not everywhere, and the cap on the trials of the forward-rejection run."""
import ctypes as C
import functools

import numpy as np
import pytest

import orc

FAIL, OK, OVERFLOW = 0, 1, 2
INLINE_TRIALS = 8          # EPV_INLINE_TRIALS
FIRST_DRAW_BLOCK = 255     # EPV_FIRST_DRAW_BLOCK
NO_ROOM_LIMIT = 0xFFFFFFFF
KAT_SEED = 0x9E3779B97F4A7C15
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------
# the restatement
def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


@functools.lru_cache(maxsize=None)
def block(seed, site, sweep, b, k, t, blk):
    """(d0, d1) of the block at (site, sweep, trial t, branch b << 20 | segment k << 8 | blk), key = seed"""
    w = philox4x32_10((site, sweep, t, (b << 20) | (k << 8) | blk), (seed & M32, seed >> 32))
    return ((w[1] << 32 | w[0]) >> 11) * 2.0 ** -53, ((w[3] << 32 | w[2]) >> 11) * 2.0 ** -53


def first_draw(seed, site, sweep, b, k, t):
    if t == 1:
        return block(seed, site, sweep, b, k, 0, 0)[1]
    return block(seed, site, sweep, b, k, t >> 1, FIRST_DRAW_BLOCK)[t & 1]


def _kat1(fn, *xs):
    cs = [C.c_double(x) for x in xs]
    out = C.c_double(0.0)
    fn(orc.MATH_EPV, 1, *[C.byref(c) for c in cs], C.byref(out))
    return out.value


def hold_time(u, rate):
    return _kat1(orc.orc_lib().orc_kat_hold_time_array, u, rate)


def trunc_exp_time(u, trunc, rate):
    return _kat1(orc.orc_lib().orc_kat_trunc_exp_time_array, u, trunc, rate)


def trunc_of(a0, T, r0, r1):
    """sample_trunc_exp's bracket 1 - exp(-rate_a0 T) with the oracle's exp"""
    return 1.0 - float(orc.kat_exp_log([-(r1 if a0 else r0) * T])[0][0])


def run_trial(seed, site, sweep, b, k, t, u0, a0, end, T, r0, r1, trunc, room, nielsen=True, start=0.0):
    """one trial: (outcome, jumps, stored times).  a0 == end, or forward rejection: hold times from a0 until T
    is passed, success when the chain stands in `end`.  A state change under Nielsen: the first jump from the
    truncated exponential (a draw that does not land below T fails), then hold times from the other state."""
    rate = (r0, r1)
    a, tau, nj, d, times, u = a0, 0.0, 0, 0, [], u0
    blk = None
    if nielsen and a0 != end:
        tau = trunc_exp_time(u0, trunc, rate[a0])
        if not tau < T:
            return FAIL, 0, times
        if room == 0:
            return OVERFLOW, 0, times
        a ^= 1
        times.append(tau + start)
        nj = 1
        blk = block(seed, site, sweep, b, k, t, 0)
        u, d = blk[0], 1
    while True:
        tau = tau + hold_time(u, rate[a])
        if not tau < T:
            return (OK if a == end else FAIL), nj, times
        if nj >= room:
            return OVERFLOW, nj, times
        a ^= 1
        times.append(tau + start)
        nj += 1
        if d & 1 == 0:
            blk = block(seed, site, sweep, b, k, t, d >> 1)
        u = blk[d & 1]
        d += 1


def scan_trials(seed, site, sweep, b, k, t0, W, a0, end, T, r0, r1, trunc, room, nielsen=True, start=0.0):
    """trials t0 .. t0 + W - 1 in order: (outcome, winning trial, its jumps, its times, M = the most jumps of any
    trial evaluated, drawn = (trial, draws) of every trial evaluated); FAIL when all W fail"""
    maxm, drawn = 0, []
    for t in range(t0, t0 + W):
        oc, nj, times = run_trial(seed, site, sweep, b, k, t, first_draw(seed, site, sweep, b, k, t), a0, end, T, r0,
                                  r1, trunc, room, nielsen, start)
        maxm = max(maxm, nj)
        drawn.append((t, oc, nj))
        if oc != FAIL:
            return oc, t, nj, times, maxm, drawn
    return FAIL, 0, 0, [], maxm, drawn


# ---------------------------------------------------------------------------------------------------------
# hand-worked cases
def test_philox_published_vectors():
    # Random123's known answers for philox4x32_10 (kat_vectors)
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((M32,) * 4, (M32, M32)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_block_layout_and_first_draw_addresses():
    # the all-ones vector again through the counter layout: site, sweep, trial, branch << 20 | segment << 8 | block
    d0, d1 = block(M32 << 32 | M32, M32, M32, 0xFFF, 0xFFF, M32, 0xFF)
    assert d0 == ((0x41C83B0E << 32 | 0x408F276D) >> 11) * 2.0 ** -53
    assert d1 == ((0x6D5451FD << 32 | 0xA20BC7C6) >> 11) * 2.0 ** -53
    s = (77, 5, 9, 3, 2)
    # trial 1 shares the end-state block; trials 2m and 2m + 1 share block (m, 255)
    assert first_draw(*s, 1) == block(*s, 0, 0)[1]
    assert first_draw(*s, 2) == block(*s, 1, 255)[0] and first_draw(*s, 3) == block(*s, 1, 255)[1]
    assert first_draw(*s, 8) == block(*s, 4, 255)[0] and first_draw(*s, 9) == block(*s, 4, 255)[1]
    # the unified form: counter word t >> 1 and half t & 1 for EVERY t, only the block index depends on t == 1
    for t in range(1, 40):
        assert first_draw(*s, t) == block(*s, t >> 1, 0 if t == 1 else 255)[t & 1]


def test_hold_times_are_the_formulas():
    # u = 0: log(1) = 0 exactly, so no time passes, whatever the rate
    assert hold_time(0.0, 1.5) == 0.0 and trunc_exp_time(0.0, 0.75, 1.5) == 0.0
    assert trunc_exp_time(0.5, 0.0, 2.0) == 0.0
    # a truncated draw with trunc = 1 is a plain hold time
    for u in (0.125, 0.5, 0.999):
        assert trunc_exp_time(u, 1.0, 0.7) == hold_time(u, 0.7)
    assert abs(hold_time(0.5, 2.0) - np.log(2.0) / 2.0) < 1e-15


def test_restatement_by_hand():
    s = (KAT_SEED, 12, 3, 2, 1)
    # a keeper whose first hold time passes T: success without a jump, no further draw
    u = 0.25
    T = hold_time(u, 2.0) * 0.5
    assert run_trial(*s, 4, u, 0, 0, T, 2.0, 1.0, 0.0, NO_ROOM_LIMIT) == (OK, 0, [])
    # ... in forward-rejection mode on a state change the same draw fails
    assert run_trial(*s, 4, u, 0, 1, T, 2.0, 1.0, 0.0, NO_ROOM_LIMIT, nielsen=False) == (FAIL, 0, [])
    # one jump at h0, and the second draw is block (t, 0).d0 at the OTHER state's rate
    h0 = hold_time(u, 2.0)
    h1 = hold_time(block(*s, 4, 0)[0], 1.0)
    T = h0 + 0.5 * h1
    assert run_trial(*s, 4, u, 0, 0, T, 2.0, 1.0, 0.0, NO_ROOM_LIMIT) == (FAIL, 1, [h0])        # ends in state 1
    assert run_trial(*s, 4, u, 0, 1, T, 2.0, 1.0, 0.0, NO_ROOM_LIMIT, nielsen=False) == (OK, 1, [h0])
    assert run_trial(*s, 4, u, 0, 0, T, 2.0, 1.0, 0.0, 0) == (OVERFLOW, 0, [])
    assert run_trial(*s, 4, u, 0, 0, T, 2.0, 1.0, 0.0, NO_ROOM_LIMIT, start=3.0) == (FAIL, 1, [h0 + 3.0])
    # third draw: block (t, 0).d1 at the first state's rate; fourth: block (t, 1).d0
    h2 = hold_time(block(*s, 4, 0)[1], 2.0)
    h3 = hold_time(block(*s, 4, 1)[0], 1.0)
    T = ((h0 + h1) + h2) + 0.5 * h3
    assert run_trial(*s, 4, u, 0, 1, T, 2.0, 1.0, 0.0, NO_ROOM_LIMIT, nielsen=False) == (OK, 3, [h0, h0 + h1, (h0 + h1) + h2])
    assert run_trial(*s, 4, u, 0, 1, T, 2.0, 1.0, 0.0, 2, nielsen=False) == (OVERFLOW, 2, [h0, h0 + h1])
    # Nielsen: the first jump IS the truncated time (not 0 + it), the next draw block (t, 0).d0 from the end state
    T, trunc = 0.5, trunc_of(0, 0.5, 2.0, 1.0)
    n0 = trunc_exp_time(u, trunc, 2.0)
    assert n0 < T
    g1 = hold_time(block(*s, 4, 0)[0], 1.0)
    oc, nj, times = run_trial(*s, 4, u, 0, 1, T, 2.0, 1.0, trunc, NO_ROOM_LIMIT)
    assert times[0] == n0
    if n0 + g1 < T:
        assert nj >= 2 and times[1] == n0 + g1
    else:
        assert (oc, nj, times) == (OK, 1, [n0])
    assert run_trial(*s, 4, u, 0, 1, T, 2.0, 1.0, trunc, 0) == (OVERFLOW, 0, [])
    # the scan: first non-failing trial, M over every trial evaluated
    oc, tstar, nj, times, maxm, drawn = scan_trials(*s, 1, 8, 0, 0, 3.0, 2.0, 1.0, 0.0, NO_ROOM_LIMIT)
    assert [x[0] for x in drawn] == list(range(1, len(drawn) + 1)) and all(x[1] == FAIL for x in drawn[:-1])
    assert maxm == max(x[2] for x in drawn) and (oc == FAIL or (tstar, nj) == (drawn[-1][0], drawn[-1][2]))


# ---------------------------------------------------------------------------------------------------------
# the cases of the GPU part: dicts of site, sweep, node, k, t0, room, a0, end, nielsen, T, r0, r1, trunc, u0, start
def _case(rng, **kw):
    c = dict(site=int(rng.randint(0, 2 ** 31)), sweep=int(rng.randint(0, 2 ** 20)), node=int(rng.randint(1, 4096)),
             k=int(rng.randint(0, 4096)), t0=1, room=NO_ROOM_LIMIT, a0=int(rng.randint(2)), end=int(rng.randint(2)),
             nielsen=True, T=0.3, r0=float(rng.uniform(0.4, 3.0)), r1=float(rng.uniform(0.4, 3.0)), start=0.0, u0=None)
    c.update(kw)
    c["trunc"] = trunc_of(c["a0"], c["T"], c["r0"], c["r1"]) if c["a0"] != c["end"] else 0.0
    if c["u0"] is None:
        c["u0"] = first_draw(KAT_SEED, c["site"], c["sweep"], c["node"], c["k"], c["t0"])
    return c


def _key(c):
    return (KAT_SEED, c["site"], c["sweep"], c["node"], c["k"])


def _seg(c):
    return (c["a0"], c["end"], c["T"], c["r0"], c["r1"], c["trunc"])


def expected(c):
    """what epv_trial_kat returns for the case: first draw, and (outcome, trial, jumps, M, two times) of the five
    evaluations"""
    out = []

    def row(oc, t, nj, times, mm):
        tt = (list(times) + [0.0, 0.0])[:2]
        return (oc, t, nj, mm, tt[0], tt[1])
    u = first_draw(*_key(c), c["t0"])
    oc, nj, times = run_trial(*_key(c), c["t0"], u, *_seg(c), c["room"], c["nielsen"], c["start"])
    out.append(row(oc, c["t0"], nj, times, nj))
    oc, nj, times = run_trial(*_key(c), c["t0"], c["u0"], *_seg(c), c["room"], c["nielsen"], c["start"])
    out.append(row(oc, c["t0"], nj, times, nj))
    for W in (1, 4, 8):
        oc, t, nj, times, mm, _ = scan_trials(*_key(c), c["t0"], W, *_seg(c), c["room"], c["nielsen"], c["start"])
        # (a scan that fails reports no trial and no jumps; its stored times are those of the last trial that
        # stored any, which the callers never read: compared only on success and overflow)
        out.append(row(oc, t, nj, times, mm) if oc != FAIL else (FAIL, None, 0, mm, None, None))
    return u, out


@functools.lru_cache(maxsize=None)
def trial_cases():
    rng = np.random.RandomState(2024)
    cases = []
    lengths = (0.02, 0.2, 0.7, 1.5, 4.0, 9.0)
    firsts = (1, 1, 1, 2, 3, 4, 5, 9, 13, 17)
    rooms = (NO_ROOM_LIMIT, NO_ROOM_LIMIT, NO_ROOM_LIMIT, 0, 1, 2, 3)
    for i in range(256):
        cases.append(_case(rng, T=lengths[i % 6], t0=firsts[(i // 2) % 10], room=rooms[(i // 3) % 7],
                           nielsen=(i % 8 != 5), start=(0.0 if i % 4 else 0.3125)))
    # forward rejection on a flip over a short segment: many trials, the winner beyond the inline window
    for i in range(24):
        cases.append(_case(rng, T=0.12, a0=i & 1, end=(i & 1) ^ 1, nielsen=False, t0=(1, 9)[i % 2]))
    # Nielsen draws handed to run_trial within rounding of 1: some land at or beyond T and fail there
    for i in range(32):
        cases.append(_case(rng, T=float(rng.uniform(0.05, 2.0)), a0=i & 1, end=(i & 1) ^ 1, u0=1.0 - 2.0 ** -53,
                           t0=(1, 2)[i % 2]))
    return tuple(cases)


def test_cases_cover_what_they_claim():
    cases = trial_cases()
    assert 200 <= len(cases) <= 512
    seen = set()
    winners = set()
    for c in cases:
        flip = c["nielsen"] and c["a0"] != c["end"]
        kind = "flip" if flip else ("keep" if c["a0"] == c["end"] else "forward-flip")
        u, rows = expected(c)
        seen.add(kind)
        seen.add(("t0 is 1", c["t0"] == 1))
        # the unlimited-room scan from the case's first trial: who wins, with how many jumps
        oc, t, nj, times, mm, drawn = scan_trials(*_key(c), c["t0"], 64, *_seg(c), NO_ROOM_LIMIT, c["nielsen"])
        if oc == OK:
            winners.add(t)
            seen.add((kind, "jumps", nj if nj < 3 else ">= 3"))
            if c["t0"] == 1:
                seen.add(("winner", "1" if t == 1 else "even" if t % 2 == 0 and t <= INLINE_TRIALS else
                          "odd" if t <= INLINE_TRIALS else "beyond inline"))
            if nj >= 4:
                seen.add("block 1 read")                  # draws 0 .. 4: the first, then (t, 0).d0, d1 and (t, 1).d0
            if mm > nj:
                seen.add("a failed trial with more jumps than the winner")
                if mm > c["room"] >= nj:
                    seen.add("M decides the overflow")
        if c["room"] == 0:
            seen.add("room 0")
        if rows[1][0] == FAIL and flip and rows[1][2] == 0 and not trunc_exp_time(c["u0"], c["trunc"], (c["r0"], c["r1"])[c["a0"]]) < c["T"]:
            seen.add("Nielsen's draw fails tau < T")
        if rows[0][0] == OVERFLOW or rows[4][0] == OVERFLOW:
            seen.add("overflow")
    want = {"flip", "keep", "forward-flip", ("t0 is 1", True), ("t0 is 1", False), "block 1 read", "room 0", "overflow",
            "a failed trial with more jumps than the winner", "M decides the overflow", "Nielsen's draw fails tau < T",
            ("winner", "1"), ("winner", "even"), ("winner", "odd"), ("winner", "beyond inline")}
    # (a keeper ends where it began: an even number of jumps; a flip makes an odd number)
    want |= {("keep", "jumps", 0), ("keep", "jumps", 2), ("keep", "jumps", ">= 3"), ("flip", "jumps", 1),
             ("flip", "jumps", ">= 3"), ("forward-flip", "jumps", 1)}
    assert want <= seen, sorted(map(str, want - seen))
    assert {2, 3} <= winners
    # the lanes of one wave (64 consecutive cases) mix flips with keepers and t == 1 with t >= 2
    for w in range(0, len(cases) - 63, 64):
        wave = cases[w:w + 64]
        assert {c["a0"] != c["end"] for c in wave} == {True, False} and {c["t0"] == 1 for c in wave} == {True, False}


# ---------------------------------------------------------------------------------------------------------
# the whole runs of the GPU part: inputs, and what they rest on (the oracle alone)
RUN_SEED = 31
RUNS = ("tree193", "tree-window", "pair257")
FR_SEED, FR_TRIAL_CAP = 5, 2000000


def run_inputs(name):
    """model, tree, paths, capacity"""
    from common import simulate
    if name == "tree193":           # a partial last wave
        model, tree, fp = simulate("tree", 193, seed=8)
    elif name == "pair257":         # a long branch: several jumps per trial, many trials
        model, tree, fp = simulate("pair", 257, seed=8)
    else:                           # tree.nwk, n = 1000, a window of 0 .. 3 jumps per path at capacity 4
        from test_fused_merge_select import _inputs
        return _inputs("tree", "mixed", 1000)
    return model, tree, fp, int(max(16, 2 * fp.counts().max() + 8))


def _flips_and_keepers(tree, before, after):
    """branches of sites whose path an accepted proposal replaced: an odd number of jumps holds a segment that
    changed state, none at all holds keepers only"""
    B, n = tree.n_nodes - 1, before.n_sites
    cb, ca = before.counts().reshape(B, n), after.counts().reshape(B, n)
    ib, ia = before.init.reshape(B, n), after.init.reshape(B, n)
    moved = ((cb != ca) | (ib != ia)).any(axis=0)
    return int(((ca % 2 == 1) & moved).sum()), int(((ca == 0) & moved).sum())


@pytest.mark.parametrize("name", RUNS)
def test_whole_run_inputs_exercise_the_trial_body(name):
    model, tree, fp, cap = run_inputs(name)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=RUN_SEED)
    o.reset()
    _, _, nacc, _ = o.run_mcmc(1, 2)
    c = o.counters()
    assert nacc > 0
    assert c["overflow"] < fp.n_sites - 2, c                 # no run overflows every site
    assert c["trials"] > c["segments"] > 0, c                # some segment needs a second trial
    flips, keepers = _flips_and_keepers(tree, fp, o.paths())
    assert flips > 0 and keepers > 0, (flips, keepers)


def test_forward_rejection_run_is_short():
    model, tree, fp, cap = run_inputs("tree193")
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=FR_SEED)
    o.set_sampler(True)
    o.reset()
    _, _, nacc, _ = o.run_mcmc(1, 1)
    c = o.counters()
    assert nacc > 0 and c["overflow"] < fp.n_sites - 2, c
    assert c["segments"] < c["trials"] <= FR_TRIAL_CAP, c
    flips, keepers = _flips_and_keepers(tree, fp, o.paths())
    assert flips > 0 and keepers > 0, (flips, keepers)
