"""The direct end-conditioned sampler (run_direct, epievo_amd/csrc/epv_direct.h) restated in Python.

The CPU oracle has no such mode.  As tests/test_trial_body.py does for the trial evaluator, the restatement takes its
bits from the oracle's known-answer entries: Philox blocks through test_trial_body.block, exp through the entry behind
orc.kat_exp_log, the truncated-exponential transform through test_trial_body.trunc_exp_time; everything else is IEEE
double arithmetic in the order the device writes it.

  direct_segment(seed, site, sweep, b, k, a0, end, T, r0, r1, room, start)
      -> (outcome, times, draws, longest_round_run)

Draw 0 of a segment is trial 1's first draw, (b, k, t = 0, blk = 0).d1; draw d >= 1 sits at trial word
1 + (d - 1) // 508, block ((d - 1) % 508) >> 1, half (d - 1) & 1 (the row "direct sampler" of epv_philox.h)."""
import ctypes as C

import orc
from test_trial_body import block, first_draw, trunc_exp_time

FAIL, OK, OVERFLOW, GIVEUP = 0, 1, 2, 3
ROUNDS = 64                 # EPV_DIRECT_ROUNDS
WORD_DRAWS = 508            # EPV_DIRECT_WORD_DRAWS
MAX_ROOM = 4096             # EPV_DIRECT_MAX_ROOM


def draw_address(d):
    """(trial word, block, half) of draw d >= 1"""
    e = d - 1
    return 1 + e // WORD_DRAWS, (e % WORD_DRAWS) >> 1, e & 1


def draw(seed, site, sweep, b, k, d):
    if d == 0:
        return first_draw(seed, site, sweep, b, k, 1)
    t, blk, half = draw_address(d)
    return block(seed, site, sweep, b, k, t, blk)[half]


def stream(seed, site, sweep, b, k):
    """d -> draw d, the blocks evaluated outside test_trial_body.block's cache (a law test draws a million)"""
    raw = block.__wrapped__
    last = [None, None]

    def u(d):
        if d == 0:
            return raw(seed, site, sweep, b, k, 0, 0)[1]
        t, blk, half = draw_address(d)
        if last[0] != (t, blk):
            last[0], last[1] = (t, blk), raw(seed, site, sweep, b, k, t, blk)
        return last[1][half]
    return u


_x, _e, _l = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)


def exp_(x):
    """orc.kat_exp_log's exp of one value (the same entry, without the arrays)"""
    _x.value = x
    orc.orc_lib().orc_kat_exp_log_array(C.byref(_x), 1, C.byref(_e), C.byref(_l))
    return _e.value


def branch_segments(left, l_init, right, r_init, T):
    """the segments of a branch in the merge order of the jump kernels (Segment.cpp:35-79: the earlier neighbour jump
    ends a segment, ties go to the right neighbour): [(length, context 4 l + r)] -- lengths are differences of
    consecutive neighbour jump times"""
    out, i, j, start, trip0 = [], 0, 0, 0.0, 4 * int(l_init) + int(r_init)
    inf = float("inf")
    while True:
        last = not (i < len(left) or j < len(right))
        tl, tr = (left[i] if i < len(left) else inf), (right[j] if j < len(right) else inf)
        take_left = tl < tr
        end = T if last else (tl if take_left else tr)
        out.append((end - start, trip0))
        if last:
            return out
        if take_left:
            trip0 ^= 4
            i += 1
        else:
            trip0 ^= 1
            j += 1
        start = end


def replay_branch(seed, gsite, sweep, node, segs, rates, start_state, new_times, capacity):
    """the branch's jump times as the jump kernels lay them down in direct mode: direct_segment over the segments in
    order, each segment's end state read off the new path (its state at the segment's end), its start time the
    running sum of the lengths, its room what the capacity leaves.  -> (times, longest run of rounds)"""
    out, cnt, passed, prev, longest = [], 0, 0.0, int(start_state), 0
    for k, (length, trip0) in enumerate(segs):
        if k == len(segs) - 1:
            upto = len(new_times)
        else:
            bound = passed + length
            upto = cnt
            while upto < len(new_times) and new_times[upto] < bound:
                upto += 1
        sampled = int(start_state) ^ (upto & 1)
        oc, times, _, run = direct_segment(seed, gsite, sweep, node, k, prev, sampled, length, float(rates[trip0]),
                                           float(rates[trip0 | 2]), capacity - cnt, passed)
        if oc != OK:
            return None, longest
        out += times
        cnt += len(times)
        longest = max(longest, run)
        prev = sampled
        passed += length
    return out, longest


def replay_phase(seed, sweep, colour, rates, branches, before, after, capacity, only_changed):
    """every interior site of the colour (global site % 3 == colour) and every branch: the new path against
    replay_branch from the old neighbours.  only_changed: (site, branch) pairs whose path is the old one are left
    out (a rejected proposal leaves no trace).  -> (pairs compared, [(site, branch)] that differ, longest run)"""
    n, B = before.n_sites, before.n_nodes - 1
    ob, oa = [int(x) for x in before.offsets], [int(x) for x in after.offsets]
    jb, ja = before.jumps.tolist(), after.jumps.tolist()
    compared, bad, longest = 0, [], 0
    for site in range(1, n - 1):
        if site % 3 != colour:
            continue
        for b in range(B):
            e = b * n + site
            new = ja[oa[e]:oa[e + 1]]
            if only_changed and new == jb[ob[e]:ob[e + 1]] and before.init[e] == after.init[e]:
                continue
            el, er = e - 1, e + 1
            segs = branch_segments(jb[ob[el]:ob[el + 1]], before.init[el], jb[ob[er]:ob[er + 1]], before.init[er],
                                   float(branches[b + 1]))
            got, run = replay_branch(seed, site, sweep, b + 1, segs, rates, after.init[e], new, capacity)
            compared += 1
            longest = max(longest, run)
            if got != new:
                bad.append((site, b))
    return compared, bad, longest


def direct_segment(seed, site, sweep, b, k, a0, end, T, r0, r1, room, start, uniforms=None, first_draw_index=0):
    """uniforms (tests of the law only): a callable d -> draw d instead of the Philox stream.  first_draw_index
    (epv_direct_kat's item word 6): the draws begin at this index of the stream, and `draws` is the index after the
    last one"""
    if uniforms is None:
        uniforms = stream(seed, site, sweep, b, k)
    room = min(room, MAX_ROOM)
    lam = r0 + r1
    a, nj, d, longest, base, times = a0, 0, int(first_draw_index), 0, 0.0, []
    for _ in range(room + 1):
        s = T - base
        ra, rb = (r1, r0) if a else (r0, r1)
        ea = exp_(-ra * s)
        tn, landed, run = 0.0, False, 0
        if a == end:
            el = exp_(-lam * s)
            p0 = ea / ((rb + ra * el) / lam)
            u0 = uniforms(d)
            d += 1
            if 1.0 - u0 < p0:
                return OK, times, d, longest
            if nj >= room:
                return OVERFLOW, times, d, longest
            w, wl = 1.0 - ea, 1.0 - el
            while run < ROUNDS and not landed:
                u, v = uniforms(d), uniforms(d + 1)
                d += 2
                run += 1
                tau = trunc_exp_time(u, w, ra)
                tn = base + tau
                if tau < s and tn > base and tn < T:
                    landed = v * wl < 1.0 - exp_(-lam * (s - tau))
        else:
            if nj >= room:
                return OVERFLOW, times, d, longest
            eb = exp_(-rb * s)
            w1, wb = 1.0 - ea, 1.0 - eb
            w2 = ea * wb
            while run < ROUNDS and not landed:
                u, v = uniforms(d), uniforms(d + 1)
                d += 2
                run += 1
                if u * (w1 + w2) < w1:
                    tau = trunc_exp_time(v, w1, ra)
                else:
                    tau = s - trunc_exp_time(v, wb, rb)
                tn = base + tau
                landed = tau < s and tn > base and tn < T
        longest = max(longest, run)
        if not landed:
            return GIVEUP, times, d, longest
        a ^= 1
        times.append(tn + start)
        nj += 1
        base = tn
    return GIVEUP, times, d, longest
