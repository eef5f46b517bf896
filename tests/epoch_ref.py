"""Yardstick of the epoch statistics (epv_set_epoch_stats): J and D per branch, epoch and context by walking
the paths per triple in Python ints, straight from the definition.

Per branch b with scale 2^k_b: fixT = rint(T_b 2^k_b), edges E_p = p fixT // P (p = 0 .. P-1, E_P = +inf),
bin(c) = the largest p <= P-1 with E_p <= c.  A triple's events are walked as dense_cases.yardstick walks them
(ties right, middle, left) with an integer clock c from 0: the interval to the next event has the integer
F = rint((t - prev) 2^k_b) and occupies [c, c + F); D[b][p][ctx] receives the overlap of that range with
[E_p, E_p+1) -- computed here bin by bin, with no difference form --, then c += F and a jump of the middle site
adds 1 to J[b][bin(c)][ctx before the jump].  The last interval (to T_b) likewise.

A second, independent routine (raw_part) builds the accumulator's difference form from the same intervals; the
tests close it with the library and compare it with the direct walk."""
from bisect import bisect_right

import numpy as np


def fix_T(branches, scales):
    """fixT_b per non-root node as Python ints"""
    return [int(np.rint(float(branches[b]) * float(scales[b]))) for b in range(1, len(branches))]


def edges(fixT, P):
    return [p * fixT // P for p in range(P)]


def bin_of(E, c):
    return bisect_right(E, c) - 1


def intervals(fp, branches, scales, first=1, last=None):
    """per branch: the list of (ctx, c0, c1, mid) of the triples with a jump, the count of triples without one
    per context (each is the one interval [0, fixT)), and how many triples' clocks ended off fixT"""
    B, n = fp.n_nodes - 1, fp.n_sites
    last = n - 2 if last is None else last
    off = [int(x) for x in fp.offsets]
    jumps = fp.jumps
    init = [int(x) for x in fp.init]
    fixT = fix_T(branches, scales)
    out = []
    nj = np.diff(np.asarray(fp.offsets, np.int64)).reshape(B, n)
    st = np.asarray(fp.init, np.int64).reshape(B, n)
    sites = np.arange(first, last + 1)
    for b in range(B):
        T, sc = float(branches[b + 1]), float(scales[b + 1])
        ivs, off_T = [], 0
        # the triples without an event are only counted, per context (numpy: they are most of a genome)
        busy = (nj[b, sites - 1] + nj[b, sites] + nj[b, sites + 1]) > 0
        ctx0 = 4 * st[b, sites - 1] + 2 * st[b, sites] + st[b, sites + 1]
        quiet = [int(v) for v in np.bincount(ctx0[~busy], minlength=8)]
        for s in sites[busy].tolist():
            events = []
            for rank, bit, site in ((0, 1, s + 1), (1, 2, s), (2, 4, s - 1)):
                e = b * n + site
                events.extend((float(t), rank, bit) for t in jumps[off[e]:off[e + 1]])
            ctx = 4 * init[b * n + s - 1] + 2 * init[b * n + s] + init[b * n + s + 1]
            events.sort()
            prev, c = 0.0, 0
            for t, _, bit in events:
                F = int(np.rint((t - prev) * sc))
                ivs.append((ctx, c, c + F, bit == 2))
                c += F
                ctx ^= bit
                prev = t
            F = int(np.rint((T - prev) * sc))
            ivs.append((ctx, c, c + F, False))
            off_T += (c + F) != fixT[b]
        out.append((ivs, quiet, off_T))
    return out


def walk(ivs_per_branch, fixT, P):
    """the direct overlap walk -> (J, D) object arrays [B, P, 8] of Python ints, and what a test needs to know
    that it is not vacuous: dict(jump_epochs = the most epochs of one branch that hold a jump, span = the most
    epochs one interval meets, off_T = triples whose clock ended off fixT)"""
    B = len(ivs_per_branch)
    J = np.zeros((B, P, 8), object)
    D = np.zeros((B, P, 8), object)
    span, off_T = 0, 0
    for b, (ivs, quiet, o) in enumerate(ivs_per_branch):
        E = edges(fixT[b], P)
        off_T += o
        top = E[1:] + [None]
        for ctx, k in enumerate(quiet):       # k triples, each the interval [0, fixT)
            if k:
                for p in range(P):
                    hi = fixT[b] if top[p] is None else min(fixT[b], top[p])
                    if hi > E[p]:
                        D[b, p, ctx] += k * (hi - E[p])
        for ctx, c0, c1, mid in ivs:
            p0, p1 = bin_of(E, c0), bin_of(E, c1)
            if c1 > c0:
                span = max(span, bin_of(E, c1 - 1) - p0 + 1)
            for p in range(p0, p1 + 1):
                lo = max(c0, E[p])
                hi = c1 if top[p] is None else min(c1, top[p])
                if hi > lo:
                    D[b, p, ctx] += hi - lo
            if mid:
                J[b, p1, ctx] += 1
    jump_epochs = max(int((J[b].sum(axis=1) > 0).sum()) for b in range(B)) if B else 0
    return J, D, dict(jump_epochs=jump_epochs, span=span, off_T=off_T)


def raw_part(ivs_per_branch, fixT, P):
    """the difference form the accumulator keeps, built another way than walk(): object array [B, P, 32] of
    J[8], part (in the lo words), zeros (hi), cov[8] -- signed Python ints, see to_words"""
    B = len(ivs_per_branch)
    raw = np.zeros((B, P, 32), object)
    for b, (ivs, quiet, _) in enumerate(ivs_per_branch):
        E = edges(fixT[b], P)
        weighted = [(ctx, c0, c1, mid, 1) for ctx, c0, c1, mid in ivs]
        weighted += [(ctx, 0, fixT[b], False, k) for ctx, k in enumerate(quiet) if k]
        for ctx, c0, c1, mid, k in weighted:
            p0, p1 = bin_of(E, c0), bin_of(E, c1)
            if p0 == p1:
                raw[b, p0, 8 + ctx] += k * (c1 - c0)
            else:
                raw[b, p0, 8 + ctx] += k * (E[p0 + 1] - c0)
                raw[b, p1, 8 + ctx] += k * (c1 - E[p1])
                raw[b, p0 + 1, 24 + ctx] += k
                raw[b, p1, 24 + ctx] -= k
            if mid:
                raw[b, p1, ctx] += 1
    return raw


def to_words(raw):
    """signed Python ints [B, P, 32] -> the uint64 words of the device layout: part split into lo < 2^32 and
    hi, cov as two's complement"""
    out = np.zeros(raw.shape, np.uint64)
    for idx in np.ndindex(*raw.shape):
        v = int(raw[idx])
        c = idx[-1]
        if 8 <= c < 16:
            out[idx] = v & 0xffffffff
            out[idx[:-1] + (c + 8,)] = v >> 32
        elif c < 8 or c >= 24:
            out[idx] = v % (1 << 64)
    return out


def parts_of(raw_words):
    """uint64 [B, P, 32] -> (J, part, cov) as Python ints: what two raw parts must agree in (the split of part
    into lo and hi is not unique)"""
    r = np.asarray(raw_words, np.uint64).astype(object)
    cov = r[..., 24:32]
    cov = np.where(cov >= (1 << 63), cov - (1 << 64), cov)
    return r[..., :8], r[..., 8:16] + r[..., 16:24] * (1 << 32), cov


def sample(o, P_list, scales, branches):
    """the oracle's current paths as one sample -> {P: (J, D, info)}"""
    fp = o.paths()
    ivs = intervals(fp, branches, scales)
    fixT = fix_T(branches, scales)
    return dict((P, walk(ivs, fixT, P)) for P in P_list), ivs


def to_stats(J, D, scales, samples):
    """closed Python ints [B, P, 8] -> J, D float64 per sample: J = count / samples, D = integer 2^-k_b / samples
    (int -> double rounds to nearest even, as the library's conversion of a 128-bit integer does)"""
    Jf = np.array([[[float(int(v)) for v in row] for row in br] for br in J]) / float(samples)
    Df = np.array([[[float(int(v)) for v in row] for row in br] for br in D])
    Df = Df * (1.0 / np.asarray(scales)[1:, None, None]) / float(samples)
    return Jf, Df


class Yard:
    """the yardstick of a run: cumulative J, D per P after every batch sweep of a rung-B oracle"""

    def __init__(self, o, tree, Ps):
        self.o, self.tree, self.Ps = o, tree, Ps
        import wstat_ref
        self.sc = wstat_ref.scales(o)
        self.fixT = fix_T(tree.branches, self.sc)
        B = tree.n_nodes - 1
        self.J = dict((P, np.zeros((B, P, 8), object)) for P in Ps)
        self.D = dict((P, np.zeros((B, P, 8), object)) for P in Ps)
        self.span = dict((P, 0) for P in Ps)
        self.off_T = 0
        self.after = []          # per batch sweep: {P: (J, D)} so far

    def add(self):
        ivs = intervals(self.o.paths(), self.tree.branches, self.sc)
        for P in self.Ps:
            J, D, info = walk(ivs, self.fixT, P)
            self.J[P] = self.J[P] + J
            self.D[P] = self.D[P] + D
            self.span[P] = max(self.span[P], info["span"])
        self.off_T += info["off_T"]
        self.after.append(dict((P, (self.J[P].copy(), self.D[P].copy())) for P in self.Ps))

    def assert_not_vacuous(self):
        assert self.off_T >= 1
        for P in self.Ps:
            epochs_with_jump = max(int((self.J[P][b].sum(axis=1) > 0).sum()) for b in range(len(self.fixT)))
            if P >= 3:
                assert epochs_with_jump >= 2 and self.span[P] >= 3, P
            elif P == 2:
                assert self.span[P] == 2
