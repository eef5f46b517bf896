"""Epoch statistics, the layers above the device that need no GPU: the declared symbols, the option errors of
epievo_est_histories -E (raised before a device is opened), and ShardedSampler's read-out (the ranks' raw parts
all-gathered and added as integers, closed once) over a stand-in for the device and the collective."""
import os
import subprocess

import numpy as np
import pytest

import epoch_ref
import orc
import wstat_ref
from common import simulate
from epievo_amd import _build
from test_window_stats_layers import _Buf, _FakeComm

EXE = os.path.join(_build.BIN_DIR, "epievo_est_histories")


def test_epoch_stats_symbols_declared():
    from epievo_amd.driver import DRIVER_SYMBOLS
    from epievo_amd.sampler import ABI_SYMBOLS
    abi = ("epv_set_epoch_stats", "epv_reset_epoch_stats", "epv_accumulate_epoch_stats", "epv_epoch_stats_samples",
           "epv_epoch_stats_set_samples", "epv_epoch_stats_layout", "epv_get_epoch_stats")
    drv = ("epvd_set_epoch_stats", "epvd_epoch_stats_sizes", "epvd_download_epoch_stats")
    header = open(os.path.join(_build.INCLUDE, "epievo_mi355x.h")).read()
    dheader = open(os.path.join(_build.INCLUDE, "epievo_mi355x_driver.h")).read()
    for s in abi:
        assert s in ABI_SYMBOLS and ("int %s(" % s) in header
    for s in drv:
        assert s in DRIVER_SYMBOLS and ("int %s(" % s) in dheader


def _run(*args):
    return subprocess.run([EXE] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_epoch_option_errors_come_before_any_device(tmp_path):
    """-K without -E, and -K out of range with -E: refused on the options alone (the input files do not even exist)"""
    files = [tmp_path / "p.param", tmp_path / "t.nwk", tmp_path / "in.local_paths"]
    r = _run("-o", tmp_path / "o.paths", "-K", 5, *files)
    assert r.returncode != 0 and "-E/--epochs" in r.stderr, r.stderr
    for K in (0, 257):
        r = _run("-o", tmp_path / "o.paths", "-E", tmp_path / "e.txt", "-K", K, *files)
        assert r.returncode != 0 and "1 to 256 epochs" in r.stderr, r.stderr
        assert not (tmp_path / "e.txt").exists()
    r = _run("-o", tmp_path / "o.paths", "-E", tmp_path / "e.txt", "-K", 5, *files)
    assert r.returncode != 0 and "belongs to" not in r.stderr  # -K goes with -E: what fails now is the missing input


class _FakeDev:
    """what ShardedSampler asks of its device: this rank's raw part, the layout, and host-side buffers"""

    def __init__(self, ns, raw, k, fixT):
        self.ns, self.raw, self.k, self.fixT = ns, raw, k, fixT

    def epoch_raw(self):
        return self.ns, self.raw

    def epoch_stats_layout(self):
        return self.raw.shape[1], self.k, self.fixT

    def alloc(self, nbytes):
        return _Buf(nbytes)

    def write(self, buf, offset, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf.data[offset:offset + raw.size] = raw

    def read(self, buf, offset, count, dtype=np.float64):
        return buf.data[offset:offset + count * np.dtype(dtype).itemsize].view(dtype).copy()


def test_engines_have_what_the_sharded_layer_asks_for():
    from epievo_amd.parallel import LocalGroup, ShardedSampler
    from epievo_amd.sampler import DeviceSampler, SingleSiteSampler
    asked = [m for m in vars(_FakeDev) if not m.startswith("_")]
    asked += [m for m in vars(ShardedSampler) if "epoch_stats" in m]
    assert "epoch_raw" in asked and "epoch_stats" in asked and "enable_epoch_stats" in asked
    for engine in (DeviceSampler, LocalGroup):
        missing = [m for m in asked if not callable(getattr(engine, m, None))]
        assert not missing, (engine.__name__, missing)
    for m in ("enable_epoch_stats", "reset_epoch_stats", "accumulate_epoch_stats", "epoch_stats_samples", "epoch_stats"):
        assert callable(getattr(SingleSiteSampler, m, None)), m


def test_sharded_read_out_adds_the_ranks_integers():
    from epievo_amd.parallel import ShardedSampler
    n, P, ns = 900, 7, 5
    model, tree, fp = simulate("tree", n, seed=9)
    o = orc.Oracle(tree, model, fp, "B", cap=32)
    sc = wstat_ref.scales(o)
    fixT = epoch_ref.fix_T(tree.branches, sc)
    k = np.frexp(sc[1:])[1] - 1
    cuts = [0, 300, 650, n]

    def raw(a, b):                               # the triples centred at the owned sites a .. b - 1, ns equal samples
        ivs = epoch_ref.intervals(fp, tree.branches, sc, first=max(a, 1), last=min(b - 1, n - 2))
        return epoch_ref.to_words(epoch_ref.raw_part(ivs, fixT, P) * ns)

    J1, D1, _ = epoch_ref.walk(epoch_ref.intervals(fp, tree.branches, sc), fixT, P)
    J, D = J1 * ns, D1 * ns
    parts = [raw(cuts[r], cuts[r + 1]) for r in range(3)]
    assert all(p[..., 8:24].any() for p in parts)
    pieces, ranks = {}, []
    for r in range(3):
        s = object.__new__(ShardedSampler)
        s.comm, s.cuts = _FakeComm(3, r, pieces), cuts
        s.dev = _FakeDev(ns, parts[r], k, np.array(fixT, np.uint64))
        ranks.append(s)
    for s in ranks:                              # round 0 only fills `pieces`: the others' are still missing
        if s is ranks[-1]:
            s.epoch_stats(counts=True)
        else:
            with pytest.raises(RuntimeError, match="different numbers"):
                s.epoch_stats(counts=True)
    Jw, Dw = epoch_ref.to_stats(J, D, sc, ns)
    for s in ranks:
        got_ns, gJ, gD = s.epoch_stats(counts=True)
        assert got_ns == ns and gJ.dtype == np.int64 and np.array_equal(gJ, J.astype(np.int64)) and (gD == D).all()
        got_ns, Jf, Df = s.epoch_stats()
        assert got_ns == ns and np.array_equal(Jf, Jw) and np.array_equal(Df, Dw)
    ranks[1].dev.ns = 4
    for s in (ranks[1], ranks[0]):
        with pytest.raises(RuntimeError, match="different numbers"):
            s.epoch_stats(counts=True)
