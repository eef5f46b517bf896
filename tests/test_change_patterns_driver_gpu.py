"""Change patterns through the C++ EM driver (epv::SingleSiteSampler, libepv_driver.so) and the
epievo_est_histories program: the same rows and window sums for one GPU slot and for EPV_DEVICES-style rehearsal
slots as DeviceSampler gives; the program's -P file parses back to them, and -P changes nothing in the paths
file the run writes."""
import os
import subprocess

import numpy as np
import pytest

import orc
import patterns_ref
from common import EXTRA_TREES, TEST_PARAM_TEXT, ref_test_model, simulate
from epievo_amd import _build, driver, host
from epievo_amd.sampler import DeviceSampler

pytestmark = pytest.mark.gpu


def _device_rows(tree, model, fp, seed, burn_in, batch):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, 16)
    d.enable_change_patterns()
    d.reset()
    d.run_mcmc(burn_in, batch, seed)
    ns, rows = d.change_patterns(counts=True)
    paths = d.paths()
    d.close()
    assert ns == batch
    return rows, paths


def test_driver_rows_equal_across_slots():
    n = 40000
    model, tree, fp = simulate("tree", n, seed=5)
    L, B = 1, 3
    want, wpaths = _device_rows(tree, model, fp, 31, L, B)
    assert want.shape == (21, n) and want[:3].any(axis=1).all() and want[12:].any(axis=1).sum() >= 6
    for devices in ([0], [0, 0, 0]):
        s = driver.CppSampler(L, B, devices=devices, capacity=16)
        s.enable_change_patterns()                # before the first reset: kept for its contexts
        s.reset(model, tree, fp)
        if len(devices) > 1:
            assert s.layout()["slots_here"] == 3
        s.run_mcmc(31, 0)
        ns, rows = s.change_patterns(counts=True)
        assert ns == B and rows.shape == (21, n)                          # sites 0 and n - 1 included
        assert orc.paths_equal(s.paths(), wpaths)
        assert np.array_equal(rows, want)
        for W in (1000, 10 ** 6):
            nsw, win = s.change_pattern_windows(W)
            assert nsw == B and np.array_equal(win, patterns_ref.windows(want, W))
        s.close()


def _write(d, name, text):
    p = os.path.join(str(d), name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_est_histories_patterns_file(tmp_path):
    model = ref_test_model()
    tree = host.Tree.read(_write(tmp_path, "cat6.nwk", EXTRA_TREES["cat6"]))
    param = _write(tmp_path, "test.param", TEST_PARAM_TEXT)
    n = 3001
    fp = host.simulate(model, tree, n, 12)
    inp = str(tmp_path / "in.local_paths")
    host.write_paths(inp, tree.node_names, tree.branches, fp)     # tot_time = branch length: no rescale
    exe = os.path.join(_build.BIN_DIR, "epievo_est_histories")
    seed, L, B = 17, 2, 4

    def run(out, *extra):
        r = subprocess.run([str(x) for x in [exe, "-L", L, "-B", B, "-s", seed, "-o", out, *extra, param,
                                          tmp_path / "cat6.nwk", inp]], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True)
        assert r.returncode == 0, r.stderr
        return open(str(out), "rb").read()

    plain = run(tmp_path / "plain.local_paths")
    want, wpaths = _device_rows(tree, model, fp, seed, L, B)
    outp, _, _ = host.read_paths(str(tmp_path / "plain.local_paths"))
    assert orc.paths_equal(outp, wpaths)
    for W in (1, 100):
        f = tmp_path / ("patterns_w%d.txt" % W)
        args = ("-P", f) if W == 1 else ("-P", f, "-w", W)       # the default window is one site
        assert run(tmp_path / ("with_P_w%d.local_paths" % W), *args) == plain
        ns, w, sites, names, first, sums = patterns_ref.parse_patterns(f.read_text())
        assert (ns, w, sites) == (B, W, n)
        assert names == patterns_ref.row_names(tree) == host.change_pattern_row_names(tree)
        assert np.array_equal(first, np.arange(0, n, W))
        assert np.array_equal(sums, patterns_ref.windows(want, W)) and sums.any(axis=1).sum() >= 30
    # together with the branch-event file: both written, the paths and the -c file still the same bytes
    c0 = tmp_path / "changes.txt"
    assert run(tmp_path / "c.local_paths", "-c", c0, "-w", 100) == plain
    f, c1 = tmp_path / "both.txt", tmp_path / "changes_both.txt"
    assert run(tmp_path / "both.local_paths", "-P", f, "-c", c1, "-w", 100) == plain
    assert f.read_text() == (tmp_path / "patterns_w100.txt").read_text() and c1.read_bytes() == c0.read_bytes()
