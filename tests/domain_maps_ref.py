"""numpy yardstick of the domain maps (include/epievo_mi355x.h, epv_set_domain_maps): the rows of a sampled history
(1 where a node is in the state asked for), the run length at every site, the PART a stretch of sites contributes
(counts per node, size and site, and the first and last E = 2 (L_K - 1) bits of every row) and how adjacent parts
merge; and `walk`, the counts of one sample by a plain walk over the sites that shares no code with the rest.  No
shifted bit arithmetic here: memberships come from run lengths."""
import numpy as np

from corr_ref import pack_bits, unpack_bits
from domains_ref import node_states


def rows(fp, tree, state):
    """uint8 [N, n]: 1 where node v is in `state` (the node states of the domain size spectra)"""
    return (node_states(fp, tree) == state).astype(np.uint8)


def edge_bits(sizes):
    return 2 * (int(sizes[-1]) - 1)


def run_lengths(x):
    """x 0/1 [n] -> int64 [n]: at every site the length of the maximal run of equal values that holds it, clipped
    to the string"""
    x = np.asarray(x, np.uint8)
    n = len(x)
    if n == 0:
        return np.zeros(0, np.int64)
    starts = np.concatenate([[0], np.nonzero(x[1:] != x[:-1])[0] + 1])
    lengths = np.diff(np.concatenate([starts, [n]]))
    return np.repeat(lengths, lengths)


def members(x, L):
    """uint8 [n]: 1 where x is 1 and its run holds at least L sites"""
    x = np.asarray(x, np.uint8)
    return ((x == 1) & (run_lengths(x) >= L)).astype(np.uint8)


def part(x, sizes):
    """one sample over a stretch of sites, x 0/1 [N, cnt] with cnt >= E -> (cnt, counts uint32 [N, K, cnt],
    edges uint64 [1, N, 2, EW])"""
    x = np.asarray(x, np.uint8)
    N, cnt = x.shape
    E = edge_bits(sizes)
    assert cnt >= E
    counts = np.zeros((N, len(sizes), cnt), np.uint32)
    for v in range(N):
        for k, L in enumerate(sizes):
            counts[v, k] = members(x[v], L)
    edges = np.stack([pack_bits(x[:, :E], E), pack_bits(x[:, cnt - E:], E)], axis=1)[None]
    return cnt, counts, edges


def add_parts(a, b):
    """two samples of the same stretch: the counts add, the records of b's samples follow a's"""
    assert a[0] == b[0]
    return a[0], a[1] + b[1], np.concatenate([a[2], b[2]], axis=0)


def merge(sizes, parts):
    """adjacent parts (of the same samples), in genome order, each of at least E sites -> the part of their union"""
    E = edge_bits(sizes)
    cnt, counts, edges = parts[0][0], parts[0][1].copy(), parts[0][2].copy()
    assert cnt >= E
    for c2, n2, e2 in parts[1:]:
        assert c2 >= E
        counts = np.concatenate([counts, n2], axis=2)
        if E:
            tail, head = unpack_bits(edges[:, :, 1], E), unpack_bits(e2[:, :, 0], E)   # [samples, N, E]
            for s in range(tail.shape[0]):
                for v in range(tail.shape[1]):
                    joint = np.concatenate([tail[s, v], head[s, v]])
                    for k, L in enumerate(sizes):
                        hidden = members(joint, L).astype(np.int64)
                        hidden[:E] -= members(tail[s, v], L)
                        hidden[E:] -= members(head[s, v], L)
                        assert ((hidden == 0) | (hidden == 1)).all()
                        assert not hidden[:E - (L - 1)].any() and not hidden[E + L - 1:].any()
                        counts[v, k, cnt - E:cnt + E] += hidden.astype(np.uint32)
        edges = np.stack([edges[:, :, 0], e2[:, :, 1]], axis=2)
        cnt += c2
    return cnt, counts, edges


def walk(x, sizes):
    """counts [N][K][n] of one sample, in plain Python: at every site, step left and right while the value stays"""
    N, n = len(x), len(x[0])
    out = [[[0] * n for _ in sizes] for _ in range(N)]
    for v in range(N):
        for p in range(n):
            if not x[v][p]:
                continue
            a = p
            while a > 0 and x[v][a - 1]:
                a -= 1
            b = p
            while b + 1 < n and x[v][b + 1]:
                b += 1
            for k, L in enumerate(sizes):
                if b - a + 1 >= L:
                    out[v][k][p] = 1
    return np.array(out, np.uint32).reshape(N, len(sizes), n)
