"""Change patterns, the parts that need no GPU: the numpy yardstick (tests/patterns_ref.py) against a walk
through every path's jumps that finds subtrees by following parent_ids, on six topologies; no row is vacuous on
the forward-simulated inputs; its window sums against np.add.reduceat; the parser of the -P file; the summary
helper; the option errors of epievo_est_histories (raised before a device is opened); the declared symbols; and
ShardedSampler's read-out over a stand-in for the device and the collective.  The device side is in
test_change_patterns_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import patterns_ref
from common import simulate
from epievo_amd import _build, host

EXE = os.path.join(_build.BIN_DIR, "epievo_est_histories")
# (configuration, rows R = 12 + 2 B + I)
CASES = [("tree", 12 + 8 + 1), ("pair", 14), ("cat6", 12 + 20 + 4), ("multi", 12 + 16 + 2), ("star4", 12 + 8),
         ("bal16", 12 + 60 + 14)]


@pytest.fixture(scope="module", params=CASES, ids=[c for c, _ in CASES])
def sample(request):
    cfg, R = request.param
    model, tree, fp = simulate(cfg, 3000, seed=6)
    return cfg, R, tree, fp, patterns_ref.counts(fp, tree)


def test_yardstick_equals_walking_the_jumps(sample):
    cfg, R, tree, fp, cnt = sample
    assert cnt.dtype == np.uint32 and cnt.shape == (R, fp.n_sites) and R == patterns_ref.n_rows(tree)
    assert len(patterns_ref.row_names(tree)) == R
    assert np.array_equal(cnt, patterns_ref.brute(fp, tree))
    assert cnt.max() == 1


def test_no_row_is_vacuous_on_the_simulated_inputs(sample):
    cfg, R, tree, fp, cnt = sample
    tot = cnt.sum(axis=1, dtype=np.int64)
    B = tree.n_nodes - 1
    if cfg in ("cat6", "multi", "bal16"):
        assert (tot > 0).all(), [n for n, t in zip(patterns_ref.row_names(tree), tot) if not t]
        # every clade is seen both ways: changed, and untouched while the tree changed elsewhere
        changed = cnt[:7].sum(axis=0) > 0
        for row in cnt[12 + 2 * B:]:
            assert row.any() and (changed & (row == 0)).any()
    if cfg == "cat6":
        assert tot[6] == 10 and (tot[8], tot[9]) == (233, 220) and tot[10] == 154 and tot[11] == 131
        assert tot[12:12 + B].min() == 1 and tot[12 + B:12 + 2 * B].min() == 3
        assert list(tot[12 + 2 * B:]) == [981, 742, 510, 275]
    if cfg == "multi":
        assert tot[12:12 + B].min() == 4 and tot[12 + B:12 + 2 * B].min() == 3
    if cfg == "bal16":
        assert tot[12:12 + B].min() == 1 and tot[12 + B:12 + 2 * B].min() == 2
    if cfg == "pair":                                     # one branch: never two at once
        assert np.array_equal(cnt[7], cnt[:7].sum(axis=0)) and not cnt[8:11].any()
    if cfg == "star4":                                    # one root state for all branches: gains or losses, not both
        assert not cnt[10].any()


@pytest.mark.parametrize("W", [1, 7, 256, 10 ** 6])
def test_window_sums_equal_reduceat(sample, W):
    cfg, R, tree, fp, cnt = sample
    n = fp.n_sites
    got = patterns_ref.windows(cnt, W)
    want = np.add.reduceat(cnt.astype(np.uint64), np.arange(0, n, W), axis=1)
    assert got.dtype == np.uint64 and got.shape == (R, (n + W - 1) // W if W < n else 1)
    assert np.array_equal(got, want)
    if W == 1:
        assert np.array_equal(got, cnt)
    # pieces of the genome contribute to windows of GLOBAL sites: their contributions add up
    cut = [0, 1000, 1001, 2307, n]
    parts = [patterns_ref.windows(cnt[:, a:b], W, first_site=a, n_global=n) for a, b in zip(cut[:-1], cut[1:])]
    assert np.array_equal(sum(parts), want)


def test_summary_helper(sample):
    cfg, R, tree, fp, cnt = sample
    B = tree.n_nodes - 1
    rows = cnt * np.uint32(3)                             # three samples that all saw the same history
    rows[0, 0] = 0                                        # ... but for site 0: no single jump in any of them
    s = host.change_pattern_summary(3, rows, tree)
    K = fp.counts().reshape(B, -1).sum(axis=0)
    want0 = (K == 0).astype(np.float64)
    want0[0] = 1.0 if K[0] in (0, 1) else 0.0
    assert np.array_equal(s["conserved"], want0)
    assert s["jump_spectrum"].shape == (8, fp.n_sites) and np.array_equal(s["jump_spectrum"][0], s["conserved"])
    assert np.allclose(s["jump_spectrum"].sum(axis=0), 1.0)
    assert np.array_equal(s["jump_spectrum"][7], K >= 7)
    for i, name in enumerate(host.CHANGE_PATTERN_CLASSES):
        assert np.array_equal(s[name], cnt[7 + i])
    assert s["sole_gain"].shape == s["sole_loss"].shape == (B, fp.n_sites)
    assert np.array_equal(s["sole_gain"], cnt[12:12 + B]) and np.array_equal(s["sole_loss"], cnt[12 + B:12 + 2 * B])
    assert list(s["clade_nodes"]) == patterns_ref.clade_nodes(tree)
    assert np.array_equal(s["clade_identical_by_descent"], 1 - cnt[12 + 2 * B:].astype(np.float64))
    assert host.change_pattern_row_names(tree) == patterns_ref.row_names(tree)
    with pytest.raises(ValueError):
        host.change_pattern_summary(3, rows[:-1], tree)
    with pytest.raises(ValueError):
        host.change_pattern_summary(0, rows, tree)


def _run(*args):
    return subprocess.run([EXE] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_window_option_errors_come_before_any_device(tmp_path):
    """-P with -w 0: refused on the options alone (the input files do not even exist)"""
    files = [tmp_path / "p.param", tmp_path / "t.nwk", tmp_path / "in.local_paths"]
    r = _run("-o", tmp_path / "o.paths", "-P", tmp_path / "p.txt", "-w", 0, *files)
    assert r.returncode != 0 and "at least one site" in r.stderr, r.stderr
    r = _run("-o", tmp_path / "o.paths", "-P", tmp_path / "p.txt", "-w", 5, *files)     # -w goes with -P too
    assert r.returncode != 0 and "-c/--changes" not in r.stderr, r.stderr
    assert not (tmp_path / "p.txt").exists()


def test_patterns_file_round_trip():
    """the writer's format, through the yardstick's parser (the program's writer is checked on the GPU)"""
    text = "#samples\t4\twindow\t100\tsites\t150\n#rows\tjumps_1\tone_branch\tsole_gain:A\tclade_changed:X\n" \
           "0\t9\t8\t7\t6\n100\t1\t2\t3\t4\n"
    ns, W, n, names, first, sums = patterns_ref.parse_patterns(text)
    assert (ns, W, n, names) == (4, 100, 150, ["jumps_1", "one_branch", "sole_gain:A", "clade_changed:X"])
    assert list(first) == [0, 100] and sums.shape == (4, 2)
    assert list(sums[:, 0]) == [9, 8, 7, 6] and list(sums[:, 1]) == [1, 2, 3, 4]


def test_change_pattern_symbols_declared():
    from epievo_amd.driver import DRIVER_SYMBOLS
    from epievo_amd.sampler import ABI_SYMBOLS, CHANGE_PATTERN_ROWS
    for s in ("epv_set_change_patterns", "epv_reset_change_patterns", "epv_accumulate_change_patterns",
              "epv_change_patterns_samples", "epv_change_patterns_layout", "epv_get_change_patterns",
              "epv_get_change_pattern_windows"):
        assert s in ABI_SYMBOLS
    for s in ("epvd_set_change_patterns", "epvd_change_patterns_sizes", "epvd_download_change_patterns",
              "epvd_download_change_pattern_windows"):
        assert s in DRIVER_SYMBOLS
    assert CHANGE_PATTERN_ROWS == patterns_ref.FIXED


class _Buf:
    def __init__(self, nbytes):
        self.data = np.zeros(nbytes, np.uint8)

    def free(self):
        pass


class _FakeDev:
    """what ShardedSampler asks of its device for a read-out: this rank's result and host-side buffers"""

    def __init__(self, ns, rows, first_site, n_global):
        self.ns, self.rows, self.first_site, self.n_global = ns, rows, first_site, n_global

    def change_patterns(self, counts=False):
        return self.ns, self.rows

    def change_pattern_windows(self, W):
        return self.ns, patterns_ref.windows(self.rows, W, first_site=self.first_site, n_global=self.n_global)

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
    cfg, R, tree, fp, cnt = sample
    n = fp.n_sites
    cuts = [0, 1024, 2304, n]                    # unequal shards: the pieces are padded to the largest
    for what in ("rows", "windows"):
        pieces, ranks = {}, []
        for r in range(3):
            s = object.__new__(ShardedSampler)
            s.comm, s.cuts = _FakeComm(3, r, pieces), cuts
            s.dev = _FakeDev(5, cnt[:, cuts[r]:cuts[r + 1]], cuts[r], n)
            ranks.append(s)
        read = (lambda s: s.change_patterns(counts=True)) if what == "rows" else \
            (lambda s: s.change_pattern_windows(1000))
        want = cnt if what == "rows" else patterns_ref.windows(cnt, 1000)
        for s in ranks:                          # round 0 only fills `pieces`: the others' are still missing
            if s is ranks[-1]:
                read(s)                          # ... until the last rank has given its own
            else:
                with pytest.raises(RuntimeError, match="different numbers"):
                    read(s)
        for s in ranks:
            ns, got = read(s)
            assert ns == 5 and got.dtype == want.dtype and np.array_equal(got, want)
    ranks[1].dev.ns = 4                          # ranks that disagree on the number of samples are an error
    for s in (ranks[1], ranks[0]):
        with pytest.raises(RuntimeError, match="different numbers"):
            s.change_pattern_windows(1000)
