"""Yardstick of the regional sufficient statistics (epv_set_window_stats): the oracle's integer rows
(orc_suffstats_rows, oracle/epv_oracle.c) cut at the windows -- row w = global sites [w W, (w + 1) W) on one
context, where local site = global site -- and what a run adds to them."""
import ctypes as C

import numpy as np

import orc


def n_windows(n, W):
    W = min(int(W), n)
    return (n + W - 1) // W


def rows(o, W, n):
    """int64 [n_win, B, 16] of the oracle's current paths: J[8] then D[8] as integers per window of W sites
    (W clamped to n, as the device clamps it)"""
    W = min(int(W), n)
    nw = n_windows(n, W)
    out = np.zeros((nw, o.B, 16), np.int64)
    o.L.orc_suffstats_rows(o.h, 0, W, nw, 0, n - 1, orc._p(out, C.c_int64))
    return out


def total(o, n):
    """int64 [B, 16]: the whole genome as one row"""
    out = np.zeros((1, o.B, 16), np.int64)
    o.L.orc_suffstats_rows(o.h, 0, n + 5, 1, 0, n - 1, orc._p(out, C.c_int64))
    return out[0]


def scales(o):
    """2^k_b per node (index 0 unused)"""
    s = np.zeros(o.B + 1)
    o.L.orc_stat_scales(o.h, orc._p(s, C.c_double))
    return s


def run(o, n, Ws, burn_in, batch, base=0):
    """burn_in + batch sweeps of a reset oracle from sweep index `base`; -> {W: int64 [n_win, B, 16] added over
    the batch sweeps}, the per-sweep whole-genome totals int64 [batch, B, 16]"""
    for w in range(burn_in):
        o.sweep(base + w)
    acc = dict((W, np.zeros((n_windows(n, W), o.B, 16), np.int64)) for W in Ws)
    tot = np.zeros((batch, o.B, 16), np.int64)
    for w in range(batch):
        o.sweep(base + burn_in + w)
        for W in Ws:
            acc[W] += rows(o, W, n)
        tot[w] = total(o, n)
    return acc, tot


def to_stats(counts, sc, samples):
    """int64 [nw, B, 16] -> J, D [nw, B, 8] per sample: J = count / samples, D = integer * 2^-k_b / samples"""
    J = counts[:, :, :8].astype(np.float64) / float(samples)
    D = counts[:, :, 8:].astype(np.float64) * (1.0 / np.asarray(sc)[1:, None])[None] / float(samples)
    return J, D


def not_vacuous(counts):
    """at least two windows hold a jump and some window holds none"""
    j = counts[:, :, :8].sum(axis=(1, 2))
    return int((j > 0).sum()) >= 2 and bool((j == 0).any())
