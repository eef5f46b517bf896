"""Posterior branch-event maps, the parts that need no GPU: the numpy yardstick (tests/bevents_ref.py)
against a walk through every path's jumps, its window sums against np.add.reduceat, the option errors of
epievo_est_histories (raised before a device is opened), the declared symbols, and ShardedSampler's
read-out (ranks gathered in genome order, window contributions added) over a stand-in for the device and
the collective.  The device side is in test_branch_events_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import bevents_ref
from common import simulate
from epievo_amd import _build

EXE = os.path.join(_build.BIN_DIR, "epievo_est_histories")


@pytest.fixture(scope="module", params=[("pair", 4000), ("tree", 3001)], ids=["pair4000", "tree3001"])
def sample(request):
    cfg, n = request.param
    model, tree, fp = simulate(cfg, n, seed=6)
    return tree, fp, bevents_ref.counts(fp)


def test_yardstick_equals_walking_the_jumps(sample):
    tree, fp, cnt = sample
    assert cnt.dtype == np.uint32 and cnt.shape == (6, tree.n_nodes - 1, fp.n_sites)
    assert np.array_equal(cnt, bevents_ref.brute(fp))
    k = fp.counts().reshape(tree.n_nodes - 1, -1)
    a = fp.init.reshape(tree.n_nodes - 1, -1)
    # no plane is vacuous on these inputs: reverted changes from both start states, net gains and losses
    assert ((k >= 2) & (a == 0)).any() and ((k >= 2) & (a == 1)).any()
    assert cnt[1].any() and cnt[2].any()
    assert np.array_equal(cnt[4] + cnt[5], k) and np.array_equal(cnt[3], k >= 1)
    assert np.array_equal(bevents_ref.start1(cnt), a)


@pytest.mark.parametrize("W", [1, 7, 256, 10 ** 6])
def test_window_sums_equal_reduceat(sample, W):
    tree, fp, cnt = sample
    n = fp.n_sites
    got = bevents_ref.windows(cnt, W)
    want = np.add.reduceat(cnt.astype(np.uint64), np.arange(0, n, W), axis=2)
    assert got.dtype == np.uint64 and got.shape == (6, tree.n_nodes - 1, (n + W - 1) // W if W < n else 1)
    assert np.array_equal(got, want)
    if W == 1:
        assert np.array_equal(got, cnt)
    # pieces of the genome contribute to windows of GLOBAL sites: their contributions add up
    cut = [0, 1000, 1001, 2307, n]
    parts = [bevents_ref.windows(cnt[:, :, a:b], W, first_site=a, n_global=n) for a, b in zip(cut[:-1], cut[1:])]
    assert np.array_equal(sum(parts), want)


def _run(*args):
    return subprocess.run([EXE] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_window_option_errors_come_before_any_device(tmp_path):
    """-w without -c, and -w 0: refused on the options alone (the input files do not even exist)"""
    files = [tmp_path / "p.param", tmp_path / "t.nwk", tmp_path / "in.local_paths"]
    r = _run("-o", tmp_path / "o.paths", "-w", 5, *files)
    assert r.returncode != 0 and "-c/--changes" in r.stderr, r.stderr
    r = _run("-o", tmp_path / "o.paths", "-c", tmp_path / "c.txt", "-w", 0, *files)
    assert r.returncode != 0 and "at least one site" in r.stderr, r.stderr
    assert not (tmp_path / "c.txt").exists()


def test_changes_file_round_trip(tmp_path):
    """the writer's format, through the yardstick's parser (the program's writer is checked on the GPU)"""
    text = "#samples\t4\twindow\t100\nNODE:A\t0.25\n0\t1\t2\t3\t4\t5\t6\n100\t0\t0\t0\t1\t1\t1\nNODE:B\t1.5\n" \
           "0\t9\t8\t7\t6\t5\t4\n100\t1\t1\t1\t1\t1\t1\n"
    ns, W, names, blens, first, sums = bevents_ref.parse_changes(text)
    assert (ns, W, names, blens) == (4, 100, ["A", "B"], ["0.25", "1.5"])
    assert list(first) == [0, 100] and sums.shape == (6, 2, 2)
    assert list(sums[:, 0, 0]) == [1, 2, 3, 4, 5, 6] and list(sums[:, 1, 0]) == [9, 8, 7, 6, 5, 4]


def test_branch_event_symbols_declared():
    from epievo_amd.driver import DRIVER_SYMBOLS
    from epievo_amd.sampler import ABI_SYMBOLS, BRANCH_EVENT_PLANES
    for s in ("epv_set_branch_events", "epv_reset_branch_events", "epv_accumulate_branch_events",
              "epv_branch_events_samples", "epv_branch_events_layout", "epv_get_branch_events",
              "epv_get_branch_event_windows"):
        assert s in ABI_SYMBOLS
    for s in ("epvd_set_branch_events", "epvd_branch_events_sizes", "epvd_download_branch_events",
              "epvd_download_branch_event_windows"):
        assert s in DRIVER_SYMBOLS
    assert BRANCH_EVENT_PLANES == bevents_ref.PLANES


class _Buf:
    def __init__(self, nbytes):
        self.data = np.zeros(nbytes, np.uint8)

    def free(self):
        pass


class _FakeDev:
    """what ShardedSampler asks of its device for a read-out: this rank's result and host-side buffers"""

    def __init__(self, ns, planes, first_site, n_global):
        self.ns, self.planes, self.first_site, self.n_global = ns, planes, first_site, n_global

    def branch_events(self, counts=False):
        return self.ns, self.planes

    def branch_event_windows(self, W):
        return self.ns, bevents_ref.windows(self.planes, W, first_site=self.first_site, n_global=self.n_global)

    def alloc(self, nbytes):
        return _Buf(nbytes)

    def write(self, buf, offset, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf.data[offset:offset + raw.size] = raw

    def read(self, buf, offset, count, dtype=np.float64):
        return buf.data[offset:offset + count * np.dtype(dtype).itemsize].view(dtype).copy()


class _FakeComm:
    """an all-gather among ranks that run one after the other: pieces are remembered by rank, so the second
    round of calls sees every rank's piece"""

    def __init__(self, world, rank, pieces):
        self.world, self.rank, self.pieces = world, rank, pieces

    def all_gather(self, dev, piece, gathered):
        self.pieces[self.rank] = piece.data.copy()
        k = piece.data.size
        for r, p in self.pieces.items():
            if p.size == k:
                gathered.data[r * k:(r + 1) * k] = p


def test_sharded_read_out_gathers_in_genome_order_and_adds_windows(sample):
    from epievo_amd.parallel import ShardedSampler
    tree, fp, cnt = sample
    n = fp.n_sites
    cuts = [0, 1024, 2304, n]                    # unequal shards: the pieces are padded to the largest
    for what in ("planes", "windows"):
        pieces, ranks = {}, []
        for r in range(3):
            s = object.__new__(ShardedSampler)
            s.comm, s.cuts = _FakeComm(3, r, pieces), cuts
            s.dev = _FakeDev(5, cnt[:, :, cuts[r]:cuts[r + 1]], cuts[r], n)
            ranks.append(s)
        read = (lambda s: s.branch_events(counts=True)) if what == "planes" else (lambda s: s.branch_event_windows(1000))
        want = cnt if what == "planes" else bevents_ref.windows(cnt, 1000)
        for s in ranks:                          # round 0 only fills `pieces`: the others' are still missing
            if s is ranks[-1]:
                read(s)                          # ... until the last rank has given its own
            else:
                with pytest.raises(RuntimeError, match="different numbers"):
                    read(s)
        for s in ranks:
            ns, got = read(s)
            assert ns == 5 and got.dtype == want.dtype and np.array_equal(got, want)
    # ranks that disagree on the number of samples are an error, not a silent average
    ranks[1].dev.ns = 4
    for s in (ranks[1], ranks[0]):               # (rank 1 first: it gives its piece with the new count)
        with pytest.raises(RuntimeError, match="different numbers"):
            s.branch_event_windows(1000)
