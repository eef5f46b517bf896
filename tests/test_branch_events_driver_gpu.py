"""Posterior branch-event maps through the C++ EM driver (epv::SingleSiteSampler, libepv_driver.so) and the
epievo_est_histories program: the same planes and window sums for one GPU slot and for EPV_DEVICES-style
rehearsal slots as DeviceSampler gives; the program's -c file parses back to them, and -c changes nothing
in the paths file the run writes."""
import os
import subprocess

import numpy as np
import pytest

import bevents_ref
import orc
from common import TEST_PARAM_TEXT, TREE_NWK_TEXT, ref_test_model, simulate
from epievo_amd import _build, driver, host
from epievo_amd.sampler import DeviceSampler

pytestmark = pytest.mark.gpu


def _device_planes(tree, model, fp, seed, burn_in, batch):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, 16)
    d.enable_branch_events()
    d.reset()
    d.run_mcmc(burn_in, batch, seed)
    ns, planes = d.branch_events(counts=True)
    paths = d.paths()
    d.close()
    assert ns == batch
    return planes, paths


def test_driver_planes_equal_across_slots():
    n = 70000
    model, tree, fp = simulate("tree", n, seed=5)
    L, B = 1, 3
    want, wpaths = _device_planes(tree, model, fp, 31, L, B)
    assert want[1].any() and want[2].any() and (want[4] + want[5] > want[3]).any()
    for devices in ([0], [0, 0, 0]):
        s = driver.CppSampler(L, B, devices=devices, capacity=16)
        s.enable_branch_events()                  # before the first reset: kept for its contexts
        s.reset(model, tree, fp)
        if len(devices) > 1:
            assert s.layout()["slots_here"] == 3
        s.run_mcmc(31, 0)
        ns, planes = s.branch_events(counts=True)
        assert ns == B and planes.shape == (6, tree.n_nodes - 1, n)      # sites 0 and n - 1 included
        assert orc.paths_equal(s.paths(), wpaths)
        assert np.array_equal(planes, want)
        for W in (1000, 10 ** 6):
            nsw, win = s.branch_event_windows(W)
            assert nsw == B and np.array_equal(win, bevents_ref.windows(want, W))
        s.close()


def _write(d, name, text):
    p = os.path.join(str(d), name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_est_histories_changes_file(tmp_path):
    model = ref_test_model()
    tree = host.Tree.read(_write(tmp_path, "tree.nwk", TREE_NWK_TEXT))
    param = _write(tmp_path, "test.param", TEST_PARAM_TEXT)
    n = 3001
    fp = host.simulate(model, tree, n, 12)
    inp = str(tmp_path / "in.local_paths")
    host.write_paths(inp, tree.node_names, tree.branches, fp)     # tot_time = branch length: no rescale
    exe = os.path.join(_build.BIN_DIR, "epievo_est_histories")
    seed, L, B = 17, 2, 4

    def run(out, *extra):
        r = subprocess.run([str(x) for x in [exe, "-L", L, "-B", B, "-s", seed, "-o", out, *extra, param,
                                          tmp_path / "tree.nwk", inp]], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True)
        assert r.returncode == 0, r.stderr
        return open(str(out), "rb").read()

    plain = run(tmp_path / "plain.local_paths")
    want, wpaths = _device_planes(tree, model, fp, seed, L, B)
    outp, _, _ = host.read_paths(str(tmp_path / "plain.local_paths"))
    assert orc.paths_equal(outp, wpaths)
    for W in (1, 100):
        f = tmp_path / ("changes_w%d.txt" % W)
        args = ("-c", f) if W == 1 else ("-c", f, "-w", W)       # the default window is one site
        assert run(tmp_path / ("with_c_w%d.local_paths" % W), *args) == plain
        ns, w, names, blens, first, sums = bevents_ref.parse_changes(f.read_text())
        assert (ns, w) == (B, W)
        assert names == list(tree.node_names[1:]) and blens == ["%g" % b for b in tree.branches[1:]]
        assert np.array_equal(first, np.arange(0, n, W))
        assert np.array_equal(sums, bevents_ref.windows(want, W))
    # together with the average file: both written, the paths file still the same bytes
    f, avg = tmp_path / "both.txt", tmp_path / "avg.txt"
    assert run(tmp_path / "both.local_paths", "-c", f, "-w", 100, "-a", avg, "-n", 5) == plain
    assert f.read_text() == (tmp_path / "changes_w100.txt").read_text() and avg.stat().st_size > 0
