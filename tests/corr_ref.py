"""numpy yardstick of the spatial correlations (include/epievo_mi355x.h, epv_set_spatial_correlation): the rows of a
sampled history (the N node states, then the B net changes), the PART a stretch of sites contributes (pair counts
per lag and the first and last L bits of every row), how adjacent parts merge and how a part is closed to the
result; and `brute`, the closed result by a plain walk over init states and jump counts, site by site and pair by
pair, that shares no code with the rest."""
import numpy as np


def rows(fp, tree):
    """uint8 [N + B, n]: row v < N the state of node v (x_0 = the init state of the branch of the root's
    lowest-numbered child, x_v = a XOR (k & 1)); row N + b = k & 1 of branch b"""
    B, n = fp.n_nodes - 1, fp.n_sites
    a = fp.init.reshape(B, n).astype(np.uint8)
    c = (fp.counts().reshape(B, n) & 1).astype(np.uint8)
    child0 = min(v for v in range(1, tree.n_nodes) if tree.parent_ids[v] == 0)
    return np.concatenate([a[child0 - 1][None], a ^ c, c]).astype(np.uint8)


def pack_bits(bits, L):
    """0/1 [..., L] -> uint64 [..., ceil(L / 64)], bit j of the string in word j // 64 at position j % 64"""
    bits = np.asarray(bits, np.uint64)
    LW = (L + 63) // 64
    out = np.zeros(bits.shape[:-1] + (LW,), np.uint64)
    for j in range(L):
        out[..., j // 64] |= bits[..., j] << np.uint64(j % 64)
    return out


def unpack_bits(words, L):
    """the inverse of pack_bits: uint64 [..., LW] -> uint8 [..., L]"""
    words = np.asarray(words, np.uint64)
    j = np.arange(L)
    return ((words[..., j // 64] >> (j % 64).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


def part(x, L):
    """one sample over a stretch of sites, x [R, cnt] with cnt >= L -> (cnt, n11 uint64 [R, L + 1],
    edges uint64 [1, R, 2, LW])"""
    x = np.asarray(x, np.uint8)
    R, cnt = x.shape
    assert 1 <= L <= cnt
    xi = x.astype(np.int64)
    n11 = np.zeros((R, L + 1), np.uint64)
    for d in range(L + 1):
        n11[:, d] = (xi[:, :cnt - d] * xi[:, d:]).sum(axis=1)
    edges = np.stack([pack_bits(x[:, :L], L), pack_bits(x[:, cnt - L:], L)], axis=1)[None]
    return cnt, n11, edges


def add_parts(a, b):
    """two samples of the same stretch: the counts add, the records of b's samples follow a's"""
    assert a[0] == b[0]
    return a[0], a[1] + b[1], np.concatenate([a[2], b[2]], axis=0)


def merge(parts):
    """adjacent parts (of the same samples), in genome order, each of at least L sites -> the part of their union"""
    cnt, n11, edges = parts[0][0], parts[0][1].copy(), parts[0][2].copy()
    L = n11.shape[1] - 1
    assert cnt >= L
    for c2, n2, e2 in parts[1:]:
        assert c2 >= L
        n11 = n11 + n2
        tail = unpack_bits(edges[:, :, 1], L).astype(np.int64)      # [samples, R, L]
        head = unpack_bits(e2[:, :, 0], L).astype(np.int64)
        for d in range(1, L + 1):
            n11[:, d] += (tail[:, :, L - d:] * head[:, :, :d]).sum(axis=(0, 2)).astype(np.uint64)
        edges = np.stack([edges[:, :, 0], e2[:, :, 1]], axis=2)
        cnt += c2
    return cnt, n11, edges


def close(cnt, n11, edges):
    """a part over the whole genome -> (n11, left1, right1), each [R, L + 1]"""
    L = n11.shape[1] - 1
    head = unpack_bits(edges[:, :, 0], L).astype(np.int64).sum(axis=0)   # [R, L] ones per position, over the samples
    tail = unpack_bits(edges[:, :, 1], L).astype(np.int64).sum(axis=0)
    R = n11.shape[0]
    zero = np.zeros((R, 1), np.int64)
    in_head = np.concatenate([zero, np.cumsum(head, axis=1)], axis=1)              # the ones among the first d sites
    in_tail = np.concatenate([zero, np.cumsum(tail[:, ::-1], axis=1)], axis=1)     # among the last d sites
    ones = n11[:, :1].astype(np.int64)
    return n11.copy(), (ones - in_tail).astype(np.uint64), (ones - in_head).astype(np.uint64)


def pairs(samples, n, L):
    return np.array([samples * (n - d) for d in range(L + 1)], np.uint64)


def brute(init, counts, parent_ids, L):
    """the closed result of one sample from init [B][n] and jump counts [B][n], in plain Python: for every row, lag
    and left site, look at the two sites"""
    B, n = len(init), len(init[0])
    N = B + 1
    first_child = None
    for v in range(1, N):
        if parent_ids[v] == 0 and first_child is None:
            first_child = v

    def value(r, p):
        if r == 0:
            return int(init[first_child - 1][p])
        if r < N:
            return int(init[r - 1][p]) ^ (int(counts[r - 1][p]) % 2)
        return int(counts[r - N][p]) % 2

    n11 = [[0] * (L + 1) for _ in range(N + B)]
    left1 = [[0] * (L + 1) for _ in range(N + B)]
    right1 = [[0] * (L + 1) for _ in range(N + B)]
    for r in range(N + B):
        col = [value(r, p) for p in range(n)]
        for d in range(L + 1):
            for p in range(n - d):
                if col[p]:
                    left1[r][d] += 1
                if col[p + d]:
                    right1[r][d] += 1
                if col[p] and col[p + d]:
                    n11[r][d] += 1
    return np.array(n11, np.uint64), np.array(left1, np.uint64), np.array(right1, np.uint64)
