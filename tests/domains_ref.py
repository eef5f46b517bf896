"""numpy yardstick of the domain size spectra (include/epievo_mi355x.h, epv_set_domain_stats): the node states of
a sampled history, the bins, the PART a stretch of sites contributes, how adjacent parts merge and how a part is
closed to the result; and the closed result by a plain per-site walk."""
import numpy as np

BINS = 128
WHOLE = 1 << 62
LEN_MASK = WHOLE - 1


def bin_of(l):
    """the bin of a run of l sites (plain Python, the definition)"""
    if l < 16:
        return l
    e = l.bit_length() - 1
    return 16 + 4 * (e - 4) + ((l >> (e - 2)) & 3)


def bin_range(b):
    """(lo, hi), both included, of bin b >= 1"""
    if b < 16:
        return b, b
    e, q = 4 + (b - 16) // 4, (b - 16) % 4
    lo = (4 + q) << (e - 2)
    return lo, lo + (1 << (e - 2)) - 1


def bins_of(lengths):
    """bin_of over an integer array (lengths < 2^53)"""
    l = np.asarray(lengths, np.int64)
    e = np.frexp(l.astype(np.float64))[1].astype(np.int64) - 1
    e = np.maximum(e, 4)
    return np.where(l < 16, l, 16 + 4 * (e - 4) + ((l >> (e - 2)) & 3))


def node_states(fp, tree):
    """uint8 [N, n]: x_v = a XOR (k & 1) for v >= 1; x_0 = the init state of the branch of the root's
    lowest-numbered child"""
    B, n = fp.n_nodes - 1, fp.n_sites
    a = fp.init.reshape(B, n).astype(np.uint8)
    k = fp.counts().reshape(B, n)
    child0 = min(v for v in range(1, tree.n_nodes) if tree.parent_ids[v] == 0)
    x = np.zeros((B + 1, n), np.uint8)
    x[1:] = a ^ (k & 1).astype(np.uint8)
    x[0] = a[child0 - 1]
    return x


def record(length, state, whole=False):
    return int(length) | (int(state) << 63) | (WHOLE if whole else 0)


def part(x):
    """one sample over a stretch of sites, x [N, cnt] -> (hist uint64 [N, 2, 128], len_sum uint64 [N, 2],
    edges uint64 [1, N, 2])"""
    x = np.asarray(x, np.uint8)
    N, cnt = x.shape
    hist, len_sum = np.zeros((N, 2, BINS), np.uint64), np.zeros((N, 2), np.uint64)
    edges = np.zeros((1, N, 2), np.uint64)
    if cnt == 0:
        return hist, len_sum, edges
    for v in range(N):
        ends = np.nonzero(x[v, :-1] != x[v, 1:])[0]
        if len(ends) == 0:
            edges[0, v, :] = record(cnt, x[v, 0], True)
            continue
        edges[0, v, 0] = record(ends[0] + 1, x[v, ends[0]])
        edges[0, v, 1] = record(cnt - 1 - ends[-1], x[v, -1])
        lengths, states = np.diff(ends), x[v, ends[1:]]
        for st in (0, 1):
            sel = lengths[states == st]
            hist[v, st] = np.bincount(bins_of(sel), minlength=BINS).astype(np.uint64)
            len_sum[v, st] = sel.sum()
    return hist, len_sum, edges


def add_parts(a, b):
    """two samples of the same stretch: hist and len_sum add, the records of b's samples follow a's"""
    return a[0] + b[0], a[1] + b[1], np.concatenate([a[2], b[2]], axis=0)


def merge(parts):
    """adjacent parts (of the same samples), in genome order -> the part of their union"""
    N, ns = parts[0][0].shape[0], parts[0][2].shape[0]
    hist = sum((p[0] for p in parts), np.zeros((N, 2, BINS), np.uint64))
    len_sum = sum((p[1] for p in parts), np.zeros((N, 2), np.uint64))
    edges = np.zeros((ns, N, 2), np.uint64)
    for s in range(ns):
        for v in range(N):
            open_run, first = None, None           # (state, length)

            def close_run(state, length):
                nonlocal first
                if first is None:
                    first = (state, length)
                else:
                    hist[v, state, bin_of(length)] += np.uint64(1)
                    len_sum[v, state] += np.uint64(length)

            for p in parts:
                f, l = int(p[2][s, v, 0]), int(p[2][s, v, 1])
                if f == 0 and l == 0:
                    continue
                fs, fl = f >> 63, f & LEN_MASK
                if f & WHOLE:
                    if open_run is not None and open_run[0] == fs:
                        open_run = (fs, open_run[1] + fl)
                    else:
                        if open_run is not None:
                            close_run(*open_run)
                        open_run = (fs, fl)
                    continue
                if open_run is not None and open_run[0] == fs:
                    close_run(fs, open_run[1] + fl)
                else:
                    if open_run is not None:
                        close_run(*open_run)
                    close_run(fs, fl)
                open_run = (l >> 63, l & LEN_MASK)
            if open_run is None:
                continue
            if first is None:
                edges[s, v, :] = record(open_run[1], open_run[0], True)
            else:
                edges[s, v, 0] = record(first[1], first[0])
                edges[s, v, 1] = record(open_run[1], open_run[0])
    return hist, len_sum, edges


def close(hist, len_sum, edges):
    """a part -> the result (hist, len_sum): the first and last records are binned, a whole record once"""
    hist, len_sum = hist.copy(), len_sum.copy()
    ns, N = edges.shape[:2]
    for s in range(ns):
        for v in range(N):
            f, l = int(edges[s, v, 0]), int(edges[s, v, 1])
            if f == 0 and l == 0:
                continue
            for r in ((f,) if f & WHOLE else (f, l)):
                hist[v, r >> 63, bin_of(r & LEN_MASK)] += np.uint64(1)
                len_sum[v, r >> 63] += np.uint64(r & LEN_MASK)
    return hist, len_sum


def walk(x):
    """the closed result of one sample by walking every row site by site: every maximal run is binned"""
    N, cnt = x.shape
    hist, len_sum = np.zeros((N, 2, BINS), np.uint64), np.zeros((N, 2), np.uint64)
    for v in range(N):
        s = 0
        while s < cnt:
            e = s
            while e + 1 < cnt and x[v, e + 1] == x[v, s]:
                e += 1
            hist[v, int(x[v, s]), bin_of(e - s + 1)] += np.uint64(1)
            len_sum[v, int(x[v, s])] += np.uint64(e - s + 1)
            s = e + 1
    return hist, len_sum


def tile_crossing_runs(x, tile=64):
    """how many maximal runs of x [N, cnt] hold sites of two tiles of `tile` sites"""
    total = 0
    for row in x:
        ends = np.nonzero(row[:-1] != row[1:])[0]
        starts = np.concatenate([[0], ends + 1])
        stops = np.concatenate([ends, [len(row) - 1]])
        total += int((starts // tile != stops // tile).sum())
    return total
