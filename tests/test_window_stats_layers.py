"""Regional sufficient statistics, the layers above the device that need no GPU: the declared symbols, the
option errors of epievo_est_histories -r (raised before a device is opened), and ShardedSampler's read-out
(the ranks' integer contributions all-gathered and added, converted once) over a stand-in for the device and
the collective."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
import wstat_ref
from common import simulate
from epievo_amd import _build

EXE = os.path.join(_build.BIN_DIR, "epievo_est_histories")


def test_window_stats_symbols_declared():
    from epievo_amd.driver import DRIVER_SYMBOLS
    from epievo_amd.sampler import ABI_SYMBOLS
    abi = ("epv_set_window_stats", "epv_reset_window_stats", "epv_accumulate_window_stats", "epv_window_stats_samples",
           "epv_window_stats_set_samples", "epv_window_stats_scale_exps", "epv_window_stats_layout",
           "epv_get_window_stats", "epv_window_counts_to_stats")
    drv = ("epvd_set_window_stats", "epvd_window_stats_sizes", "epvd_download_window_stats")
    header = open(os.path.join(_build.INCLUDE, "epievo_mi355x.h")).read()
    dheader = open(os.path.join(_build.INCLUDE, "epievo_mi355x_driver.h")).read()
    for s in abi:
        assert s in ABI_SYMBOLS and ("int %s(" % s) in header
    for s in drv:
        assert s in DRIVER_SYMBOLS and ("int %s(" % s) in dheader


def _run(*args):
    return subprocess.run([EXE] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_regional_option_errors_come_before_any_device(tmp_path):
    """-w without -r or -c, and -w 0 with -r: refused on the options alone (the input files do not even exist)"""
    files = [tmp_path / "p.param", tmp_path / "t.nwk", tmp_path / "in.local_paths"]
    r = _run("-o", tmp_path / "o.paths", "-w", 5, *files)
    assert r.returncode != 0 and "-r/--regional" in r.stderr, r.stderr
    r = _run("-o", tmp_path / "o.paths", "-r", tmp_path / "r.txt", "-w", 0, *files)
    assert r.returncode != 0 and "at least one site" in r.stderr, r.stderr
    assert not (tmp_path / "r.txt").exists()
    r = _run("-o", tmp_path / "o.paths", "-r", tmp_path / "r.txt", "-w", 5, *files)
    assert r.returncode != 0 and "belongs to" not in r.stderr  # -w goes with -r: what fails now is the missing input


class _Buf:
    def __init__(self, nbytes):
        self.data = np.zeros(nbytes, np.uint8)

    def free(self):
        pass


class _FakeDev:
    """what ShardedSampler asks of its device: this rank's contribution to all windows, host-side buffers, and the
    conversion"""

    def __init__(self, ns, counts, sc):
        self.ns, self.counts, self.sc = ns, counts, sc

    def window_counts(self):
        return self.ns, self.counts

    def window_counts_to_stats(self, counts, samples):
        return wstat_ref.to_stats(counts, self.sc, samples)

    def alloc(self, nbytes):
        return _Buf(nbytes)

    def write(self, buf, offset, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf.data[offset:offset + raw.size] = raw

    def read(self, buf, offset, count, dtype=np.float64):
        return buf.data[offset:offset + count * np.dtype(dtype).itemsize].view(dtype).copy()


class _FakeComm:
    """an all-gather among ranks that run one after the other: pieces are remembered by rank"""

    def __init__(self, world, rank, pieces):
        self.world, self.rank, self.pieces = world, rank, pieces

    def all_gather(self, dev, piece, gathered):
        self.pieces[self.rank] = piece.data.copy()
        k = piece.data.size
        for r, p in self.pieces.items():
            if p.size == k:
                gathered.data[r * k:(r + 1) * k] = p


def test_engines_have_what_the_sharded_layer_asks_for():
    """ShardedSampler wraps a DeviceSampler or a LocalGroup: either has every method the stand-in above supplies,
    and every window-statistics method ShardedSampler itself offers"""
    from epievo_amd.parallel import LocalGroup, ShardedSampler
    from epievo_amd.sampler import DeviceSampler
    asked = [m for m in vars(_FakeDev) if not m.startswith("_")]
    asked += [m for m in vars(ShardedSampler) if "window_stats" in m]
    assert "window_counts_to_stats" in asked and "window_counts" in asked and "window_stats" in asked
    for engine in (DeviceSampler, LocalGroup):
        missing = [m for m in asked if not callable(getattr(engine, m, None))]
        assert not missing, (engine.__name__, missing)


def test_sharded_read_out_adds_the_ranks_integers():
    from epievo_amd.parallel import ShardedSampler
    n, W, ns = 3000, 100, 5
    model, tree, fp = simulate("tree", n, seed=9)
    o = orc.Oracle(tree, model, fp, "B", cap=32)
    sc = wstat_ref.scales(o)
    nw, B = n // W, tree.n_nodes - 1
    whole = wstat_ref.rows(o, W, n) * ns
    cuts = [0, 1024, 2304, n]                    # cut inside windows: two ranks contribute to one window

    def part(a, b):                              # rows of W sites over the owned sites a .. b - 1 only
        out = np.zeros((nw, B, 16), np.int64)
        o.L.orc_suffstats_rows(o.h, 0, W, nw, a, b - 1, orc._p(out, C.c_int64))
        return out * ns

    parts = [part(cuts[r], cuts[r + 1]) for r in range(3)]
    assert np.array_equal(sum(parts), whole) and all(p.any() for p in parts)
    assert parts[0][10].any() and parts[1][10].any()           # window 10 = sites 1000 .. 1099 straddles the cut
    pieces, ranks = {}, []
    for r in range(3):
        s = object.__new__(ShardedSampler)
        s.comm, s.cuts = _FakeComm(3, r, pieces), cuts
        s.dev = _FakeDev(ns, parts[r], sc)
        ranks.append(s)
    for s in ranks:                              # round 0 only fills `pieces`: the others' are still missing
        if s is ranks[-1]:
            s.window_stats(counts=True)
        else:
            with pytest.raises(RuntimeError, match="different numbers"):
                s.window_stats(counts=True)
    Jw, Dw = wstat_ref.to_stats(whole, sc, ns)
    for s in ranks:
        got_ns, got = s.window_stats(counts=True)
        assert got_ns == ns and got.dtype == np.int64 and np.array_equal(got, whole)
        got_ns, J, D = s.window_stats()
        assert got_ns == ns and np.array_equal(J, Jw) and np.array_equal(D, Dw)
    ranks[1].dev.ns = 4
    for s in (ranks[1], ranks[0]):
        with pytest.raises(RuntimeError, match="different numbers"):
            s.window_stats(counts=True)
