"""numpy yardstick of the domain turnover (include/epievo_mi355x.h, epv_set_domain_turnover): the rows of a
sampled history (per branch the state at its start and at its end), the PART a stretch of sites contributes with
every run kept or turned over, how adjacent parts merge and how a part is closed to the result; and `brute`, the
closed result by a plain per-site walk over the init states and jump counts that shares no code with the rest."""
import numpy as np

from domains_ref import BINS, WHOLE, bin_of, bins_of

KEPT = 1 << 61
LEN_MASK = KEPT - 1


def rows(fp):
    """uint8 [2 B, n]: row 2 b = the init state a of branch b, row 2 b + 1 = a XOR (k & 1)"""
    B, n = fp.n_nodes - 1, fp.n_sites
    a = fp.init.reshape(B, n).astype(np.uint8)
    k = fp.counts().reshape(B, n)
    x = np.zeros((2 * B, n), np.uint8)
    x[0::2] = a
    x[1::2] = a ^ (k & 1).astype(np.uint8)
    return x


def record(length, state, kept, whole=False):
    return int(length) | (int(state) << 63) | (KEPT if kept else 0) | (WHOLE if whole else 0)


def part(x):
    """one sample over a stretch of sites, x [R, cnt] (R even; the partner of row r is r ^ 1) ->
    (hist uint64 [R, 2, 2, 128], len_sum uint64 [R, 2, 2], edges uint64 [1, R, 2])"""
    x = np.asarray(x, np.uint8)
    R, cnt = x.shape
    assert R % 2 == 0
    hist, len_sum = np.zeros((R, 2, 2, BINS), np.uint64), np.zeros((R, 2, 2), np.uint64)
    edges = np.zeros((1, R, 2), np.uint64)
    if cnt == 0:
        return hist, len_sum, edges
    for r in range(R):
        same = np.concatenate([[0], np.cumsum(x[r] == x[r ^ 1])])   # same[i] = unchanged sites among the first i
        ends = np.nonzero(x[r, :-1] != x[r, 1:])[0]
        if len(ends) == 0:
            edges[0, r, :] = record(cnt, x[r, 0], same[cnt] > 0, True)
            continue
        edges[0, r, 0] = record(ends[0] + 1, x[r, ends[0]], same[ends[0] + 1] > 0)
        edges[0, r, 1] = record(cnt - 1 - ends[-1], x[r, -1], same[cnt] - same[ends[-1] + 1] > 0)
        lengths, states = np.diff(ends), x[r, ends[1:]]
        kept = (same[ends[1:] + 1] - same[ends[:-1] + 1]) > 0
        for st in (0, 1):
            for kp in (0, 1):
                sel = lengths[(states == st) & (kept == bool(kp))]
                hist[r, st, kp] = np.bincount(bins_of(sel), minlength=BINS).astype(np.uint64)
                len_sum[r, st, kp] = sel.sum()
    return hist, len_sum, edges


def add_parts(a, b):
    """two samples of the same stretch: hist and len_sum add, the records of b's samples follow a's"""
    return a[0] + b[0], a[1] + b[1], np.concatenate([a[2], b[2]], axis=0)


def _unpack(rec):
    return rec >> 63, (rec >> 61) & 1, rec & LEN_MASK


def merge(parts):
    """adjacent parts (of the same samples), in genome order -> the part of their union; a run joined from pieces is
    kept iff any piece is kept"""
    R, ns = parts[0][0].shape[0], parts[0][2].shape[0]
    hist = sum((p[0] for p in parts), np.zeros((R, 2, 2, BINS), np.uint64))
    len_sum = sum((p[1] for p in parts), np.zeros((R, 2, 2), np.uint64))
    edges = np.zeros((ns, R, 2), np.uint64)
    for s in range(ns):
        for r in range(R):
            open_run, first = None, None           # (state, kept, length)

            def close_run(state, kept, length):
                nonlocal first
                if first is None:
                    first = (state, kept, length)
                else:
                    hist[r, state, kept, bin_of(length)] += np.uint64(1)
                    len_sum[r, state, kept] += np.uint64(length)

            for p in parts:
                f, l = int(p[2][s, r, 0]), int(p[2][s, r, 1])
                if f == 0 and l == 0:
                    continue
                fs, fk, fl = _unpack(f)
                if f & WHOLE:
                    if open_run is not None and open_run[0] == fs:
                        open_run = (fs, open_run[1] | fk, open_run[2] + fl)
                    else:
                        if open_run is not None:
                            close_run(*open_run)
                        open_run = (fs, fk, fl)
                    continue
                if open_run is not None and open_run[0] == fs:
                    close_run(fs, open_run[1] | fk, open_run[2] + fl)
                else:
                    if open_run is not None:
                        close_run(*open_run)
                    close_run(fs, fk, fl)
                open_run = _unpack(l)
            if open_run is None:
                continue
            if first is None:
                edges[s, r, :] = record(open_run[2], open_run[0], open_run[1], True)
            else:
                edges[s, r, 0] = record(first[2], first[0], first[1])
                edges[s, r, 1] = record(open_run[2], open_run[0], open_run[1])
    return hist, len_sum, edges


def close(hist, len_sum, edges):
    """a part -> the result (hist, len_sum): the first and last records are binned, a whole record once"""
    hist, len_sum = hist.copy(), len_sum.copy()
    ns, R = edges.shape[:2]
    for s in range(ns):
        for r in range(R):
            f, l = int(edges[s, r, 0]), int(edges[s, r, 1])
            if f == 0 and l == 0:
                continue
            for rec in ((f,) if f & WHOLE else (f, l)):
                st, kp, ln = _unpack(rec)
                hist[r, st, kp, bin_of(ln)] += np.uint64(1)
                len_sum[r, st, kp] += np.uint64(ln)
    return hist, len_sum


def brute(init, counts):
    """the closed result of one sample from init [B][n] and jump counts [B][n], site by site in plain Python: a
    maximal run of the start (or end) state of a branch is turned over iff the jump count is odd at every site"""
    B, n = len(init), len(init[0])
    hist, len_sum = np.zeros((2 * B, 2, 2, BINS), np.uint64), np.zeros((2 * B, 2, 2), np.uint64)
    for b in range(B):
        for at_end in (0, 1):
            state = length = unchanged = None
            for s in range(n + 1):
                if s < n:
                    here = int(init[b][s])
                    odd = int(counts[b][s]) % 2
                    if at_end and odd:
                        here = 1 - here
                if s == n or (state is not None and here != state):
                    bits = length.bit_length() - 1
                    slot = length if length < 16 else 16 + 4 * (bits - 4) + ((length >> (bits - 2)) & 3)
                    flag = 1 if unchanged > 0 else 0
                    hist[2 * b + at_end, state, flag, slot] += np.uint64(1)
                    len_sum[2 * b + at_end, state, flag] += np.uint64(length)
                    state = None
                if s == n:
                    break
                if state is None:
                    state, length, unchanged = here, 0, 0
                length += 1
                unchanged += 1 - odd
    return hist, len_sum


def turned_over_counts(hist):
    """(born, died, filled, opened) runs of a closed result, summed over the branches"""
    runs = np.asarray(hist).sum(axis=3).reshape(-1, 2, 2, 2)   # [b, row, state, kept]
    return (int(runs[:, 1, 1, 0].sum()), int(runs[:, 0, 1, 0].sum()), int(runs[:, 0, 0, 0].sum()),
            int(runs[:, 1, 0, 0].sum()))
