"""Chain mixing diagnostics through the C++ driver (epv::SingleSiteSampler behind include/epievo_mi355x_driver.h)
and the epievo_est_histories program: the counts of two rehearsal slots on one GPU equal those of one DeviceSampler
(which tests/test_mixing_gpu.py pins to the oracle); the program's -x file holds the integer window sums of the moves
of its run and the pooled window summary, and -x leaves the paths the program writes byte-identical."""
import os
import subprocess

import numpy as np
import pytest

import mixing_ref
import orc
from common import TEST_PARAM_TEXT, TREE_NWK_TEXT, ref_test_model, simulate
from epievo_amd import _build, driver, host
from epievo_amd.sampler import DeviceSampler

pytestmark = pytest.mark.gpu

MAX_LAG = 3


def _device_counts(tree, model, fp, seed, burn_in, batch, calls, max_lag):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, 16)
    d.enable_mixing(max_lag)
    d.reset()
    for it in range(calls):
        d.run_mcmc(burn_in, batch, seed, sweep_base=it * (burn_in + batch))
    out, paths = d.mixing(counts=True), d.paths()
    d.close()
    return out, paths


def test_driver_of_two_slots_equals_one_context():
    n, L, B = 70000, 1, 5
    model, tree, fp = simulate("tree", n, seed=5)
    want, wpaths = _device_counts(tree, model, fp, 31, L, B, 2, MAX_LAG)
    s = driver.CppSampler(L, B, devices=[0, 0], capacity=16)
    s.enable_mixing(MAX_LAG)                       # before the first reset: kept for its contexts
    s.reset(model, tree, fp)
    assert s.layout()["slots_here"] == 2
    for it in range(2):
        s.run_mcmc(31, it)
    assert orc.paths_equal(s.paths(), wpaths)
    got = s.mixing(counts=True)
    assert got[:2] == want[:2] == (2 * B, 2 * B)
    for a, b in zip(got[2:], want[2:]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert got[3].shape == (n,) and ((got[3] > 0) & (got[3] < got[1])).any() and got[6][MAX_LAG - 1].any()
    summary = s.mixing()
    assert np.array_equal(summary["move_rate"], want[3] / float(want[1]))
    s.enable_mixing(0)
    with pytest.raises(driver.DriverError):
        s.mixing()
    with pytest.raises(driver.DriverError):
        s.enable_mixing(17)
    s.close()


def _write(d, name, text):
    p = os.path.join(str(d), name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_est_histories_mixing_file(tmp_path):
    model = ref_test_model()
    tree = host.Tree.read(_write(tmp_path, "tree.nwk", TREE_NWK_TEXT))
    param = _write(tmp_path, "test.param", TEST_PARAM_TEXT)
    n = 3001
    fp = host.simulate(model, tree, n, 12)
    inp = str(tmp_path / "in.local_paths")
    host.write_paths(inp, tree.node_names, tree.branches, fp)     # tot_time = branch length: no rescale
    exe = os.path.join(_build.BIN_DIR, "epievo_est_histories")
    seed, L, B, W = 17, 2, 6, 1000

    def run(out, *extra):
        r = subprocess.run([str(x) for x in [exe, "-L", L, "-B", B, "-s", seed, "-o", out, *extra, param,
                                          tmp_path / "tree.nwk", inp]], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True)
        assert r.returncode == 0, r.stderr
        return open(str(out), "rb").read()

    plain = run(tmp_path / "plain.local_paths")
    want, wpaths = _device_counts(tree, model, fp, seed, L, B, 1, 8)
    outp, _, _ = host.read_paths(str(tmp_path / "plain.local_paths"))
    assert orc.paths_equal(outp, wpaths)
    f = tmp_path / "mixing.txt"
    assert run(tmp_path / "with_x.local_paths", "-x", f, "-w", W) == plain        # -A defaults to 8
    got = host.read_mixing(str(f))
    assert (got["samples"], got["moved_pairs"], got["max_lag"], got["window"], got["first_window"]) == (B, B, 8, W, 0)
    assert np.array_equal(got["pairs"], want[2]) and got["sites"].tolist() == [1000, 1000, 1000, 1]
    assert got["moved"].dtype == np.uint64 and np.array_equal(got["moved"], mixing_ref.windows(want[3], W))
    assert got["moved"][:3].all()
    ws = host.mixing_window_summary(W, *want)
    for key in ("move_rate", "rho", "tau"):           # the program's floating point against numpy's: rounding apart
        assert np.allclose(got[key], ws[key], rtol=1e-9, atol=1e-12, equal_nan=True), key
    # another lag and window: the same integers where they overlap
    g = tmp_path / "mixing3.txt"
    assert run(tmp_path / "with_A.local_paths", "-x", g, "-A", 3) == plain         # -w defaults to 1
    got3 = host.read_mixing(str(g))
    assert got3["max_lag"] == 3 and got3["window"] == 1 and np.array_equal(got3["pairs"], want[2][:4])
    assert np.array_equal(got3["moved"], want[3])
    # -A without -x is refused
    r = subprocess.run([exe, "-A", "3", "-o", str(tmp_path / "no.local_paths"), param, str(tmp_path / "tree.nwk"), inp],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "-A/--acflags belongs to -x/--mixing" in r.stderr
