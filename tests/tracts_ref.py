"""numpy yardstick of the change tracts (include/epievo_mi355x.h, epv_set_change_tracts): from the rows of a sampled
history (turnover_ref.rows: per branch the state at its start and at its end) the PART a stretch of sites
contributes, how adjacent parts merge and how a part is closed to the result; and `brute`, the closed result by a
plain per-site walk over the init states and jump counts that shares no code with the rest."""
import numpy as np

from domains_ref import BINS, bin_of, bins_of
from turnover_ref import rows  # noqa: F401  (the rows are the turnover's)

CLASSES = 27
NONE = 2
LEN_MASK = (1 << 56) - 1
Y_SHIFT, GAIN_SHIFT, LOSS_SHIFT, FLANK_SHIFT = 56, 57, 58, 59
WHOLE = 1 << 62
SET = 1 << 63


def cls_of(direction, left, right):
    return direction * 9 + left * 3 + right


def dir_of(gain, loss):
    return (2 if gain else 1) if loss else 0


def record(length, y, gain=0, loss=0, flank=0, whole=False):
    """a record of a stretch of at least one site"""
    return (SET | int(length) | (int(y) << Y_SHIFT) | (int(bool(gain)) << GAIN_SHIFT) | (int(bool(loss)) << LOSS_SHIFT) |
            (int(flank) << FLANK_SHIFT) | (WHOLE if whole else 0))


def _unpack(rec):
    return (rec & LEN_MASK, (rec >> Y_SHIFT) & 1, (rec >> GAIN_SHIFT) & 1, (rec >> LOSS_SHIFT) & 1, (rec >> FLANK_SHIFT) & 1)


def part(x):
    """one sample over a stretch of sites, x [2 B, cnt] (row 2 b the start state a, row 2 b + 1 the end state y) ->
    (hist uint64 [B, 27, 128], len_sum uint64 [B, 27], edges uint64 [1, B, 2])"""
    x = np.asarray(x, np.uint8)
    R, cnt = x.shape
    assert R % 2 == 0
    B = R // 2
    hist, len_sum = np.zeros((B, CLASSES, BINS), np.uint64), np.zeros((B, CLASSES), np.uint64)
    edges = np.zeros((1, B, 2), np.uint64)
    if cnt == 0:
        return hist, len_sum, edges
    for b in range(B):
        y = x[2 * b + 1].astype(np.int64)
        c = (x[2 * b] ^ x[2 * b + 1]).astype(np.int64)
        step = np.diff(np.concatenate([[0], c, [0]]))
        s, t = np.nonzero(step == 1)[0], np.nonzero(step == -1)[0] - 1      # first and last site of every tract
        ones = np.concatenate([[0], np.cumsum(c & y)])                      # gained sites among the first i
        gain = ones[t + 1] - ones[s] > 0
        loss = (t + 1 - s) - (ones[t + 1] - ones[s]) > 0
        if len(s) == 1 and s[0] == 0 and t[0] == cnt - 1:
            edges[0, b, 0] = record(cnt, y[0], gain[0], loss[0], 0, True)
            edges[0, b, 1] = record(cnt, y[-1], gain[0], loss[0], 0, True)
            continue
        edges[0, b, 0], edges[0, b, 1] = record(0, y[0]), record(0, y[-1])
        inner = np.ones(len(s), bool)
        if len(s) and s[0] == 0:
            edges[0, b, 0] = record(t[0] + 1, y[0], gain[0], loss[0], y[t[0] + 1])
            inner[0] = False
        if len(s) and t[-1] == cnt - 1:
            edges[0, b, 1] = record(cnt - s[-1], y[-1], gain[-1], loss[-1], y[s[-1] - 1])
            inner[-1] = False
        s, t, gain, loss = s[inner], t[inner], gain[inner], loss[inner]
        k = np.where(loss, np.where(gain, 2, 1), 0) * 9 + y[s - 1] * 3 + y[t + 1]
        for q in np.unique(k):
            sel = (t - s + 1)[k == q]
            hist[b, q] = np.bincount(bins_of(sel), minlength=BINS).astype(np.uint64)
            len_sum[b, q] = sel.sum()
    return hist, len_sum, edges


def add_parts(a, b):
    """two samples of the same stretch: hist and len_sum add, the records of b's samples follow a's"""
    return a[0] + b[0], a[1] + b[1], np.concatenate([a[2], b[2]], axis=0)


def merge(parts):
    """adjacent parts (of the same samples), in genome order -> the part of their union"""
    B, ns = parts[0][0].shape[0], parts[0][2].shape[0]
    hist = sum((p[0] for p in parts), np.zeros((B, CLASSES, BINS), np.uint64))
    len_sum = sum((p[1] for p in parts), np.zeros((B, CLASSES), np.uint64))
    edges = np.zeros((ns, B, 2), np.uint64)
    for s in range(ns):
        for b in range(B):
            recs = [(int(p[2][s, b, 0]), int(p[2][s, b, 1])) for p in parts]
            recs = [(f, l) for f, l in recs if f or l]
            if not recs:
                continue
            y_first, y_last = _unpack(recs[0][0])[1], _unpack(recs[-1][1])[1]
            # the pieces as a list of items in genome order: ("tract", len, gain, loss, left, right) with a flank
            # None where the piece does not know it, and ("site", y) for an unchanged boundary site
            items = []
            for f, l in recs:
                fl, fy, fg, fo, ff = _unpack(f)
                ll, ly, lg, lo, lf = _unpack(l)
                if f & WHOLE:
                    items.append(["tract", fl, fg, fo, None, None])
                    continue
                items.append(["tract", fl, fg, fo, None, ff] if fl else ["site", fy])
                items.append(["tract", ll, lg, lo, lf, None] if ll else ["site", ly])
            joined = []
            for it in items:
                if it[0] == "tract" and joined and joined[-1][0] == "tract" and joined[-1][5] is None and it[4] is None:
                    last = joined[-1]
                    last[1], last[2], last[3], last[5] = last[1] + it[1], last[2] | it[2], last[3] | it[3], it[5]
                else:
                    joined.append(list(it))
            for i, it in enumerate(joined):                # a tract that ends at a cut: the neighbour's site
                if it[0] == "tract":
                    if it[4] is None and i > 0:
                        it[4] = joined[i - 1][1]
                    if it[5] is None and i + 1 < len(joined):
                        it[5] = joined[i + 1][1]
            first, last = joined[0], joined[-1]
            if len(joined) == 1 and first[0] == "tract":
                edges[s, b, 0] = record(first[1], y_first, first[2], first[3], 0, True)
                edges[s, b, 1] = record(first[1], y_last, first[2], first[3], 0, True)
                continue
            edges[s, b, 0] = record(first[1], y_first, first[2], first[3], first[5]) if first[0] == "tract" else record(0, y_first)
            edges[s, b, 1] = record(last[1], y_last, last[2], last[3], last[4]) if last[0] == "tract" else record(0, y_last)
            for it in joined[1:-1]:
                if it[0] == "tract":
                    q = cls_of(dir_of(it[2], it[3]), it[4], it[5])
                    hist[b, q, bin_of(it[1])] += np.uint64(1)
                    len_sum[b, q] += np.uint64(it[1])
    return hist, len_sum, edges


def close(hist, len_sum, edges):
    """a part -> the result (hist, len_sum): the tracts open at the two ends are binned with flank none"""
    hist, len_sum = hist.copy(), len_sum.copy()
    ns, B = edges.shape[:2]
    for s in range(ns):
        for b in range(B):
            f, l = int(edges[s, b, 0]), int(edges[s, b, 1])
            if f == 0 and l == 0:
                continue
            fl, _, fg, fo, ff = _unpack(f)
            ll, _, lg, lo, lf = _unpack(l)
            todo = [(fl, fg, fo, NONE, NONE)] if f & WHOLE else [(fl, fg, fo, NONE, ff), (ll, lg, lo, lf, NONE)]
            for ln, g, o, left, right in todo:
                if ln:
                    q = cls_of(dir_of(g, o), left, right)
                    hist[b, q, bin_of(ln)] += np.uint64(1)
                    len_sum[b, q] += np.uint64(ln)
    return hist, len_sum


def brute(init, counts):
    """the closed result of one sample from init [B][n] and jump counts [B][n], site by site in plain Python"""
    B, n = len(init), len(init[0])
    hist, len_sum = np.zeros((B, CLASSES, BINS), np.uint64), np.zeros((B, CLASSES), np.uint64)
    for b in range(B):
        length = 0                                         # sites of the tract that is open
        ups = downs = 0
        before = "none"                                    # the end state of the last unchanged site, as a word
        for s in range(n + 1):
            odd = s < n and int(counts[b][s]) % 2 == 1
            if odd:
                length += 1
                if int(init[b][s]) == 0:
                    ups += 1                               # 0 -> 1
                else:
                    downs += 1
                continue
            after = "none" if s == n else ("one" if int(init[b][s]) == 1 else "zero")
            if length > 0:
                direction = "gain" if downs == 0 else ("loss" if ups == 0 else "mixed")
                k = (("gain", "loss", "mixed").index(direction) * 9 + ("zero", "one", "none").index(before) * 3 +
                     ("zero", "one", "none").index(after))
                top = length.bit_length() - 1
                slot = length if length < 16 else 16 + 4 * (top - 4) + ((length >> (top - 2)) & 3)
                hist[b, k, slot] += np.uint64(1)
                len_sum[b, k] += np.uint64(length)
            length = ups = downs = 0
            before = after
    return hist, len_sum


def pure_counts(hist):
    """{(direction, left, right): tracts} of a closed result over all branches, flanks 0 and 1 only"""
    t = np.asarray(hist).sum(axis=(0, 2)).reshape(3, 3, 3)
    return {(d, l, r): int(t[d, l, r]) for d in range(3) for l in (0, 1) for r in (0, 1)}
