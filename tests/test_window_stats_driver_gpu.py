"""Regional sufficient statistics through the C++ EM driver (epv::SingleSiteSampler, libepv_driver.so) and the
epievo_est_histories program: one GPU slot and three rehearsal slots give the integers DeviceSampler gives; the
program's -r file parses (epv_io's reader) to the API's numbers, and -r changes nothing in the paths file."""
import os
import subprocess

import numpy as np
import pytest

import orc
from common import TEST_PARAM_TEXT, TREE_NWK_TEXT, ref_test_model, simulate
from epievo_amd import _build, driver, host
from epievo_amd.sampler import DeviceSampler

pytestmark = pytest.mark.gpu


def _device_windows(tree, model, fp, seed, burn_in, batch, W):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, 16)
    d.enable_window_stats(W)
    d.reset()
    d.run_mcmc(burn_in, batch, seed)
    ns, counts = d.window_stats(counts=True)
    _, J, D = d.window_stats()
    paths = d.paths()
    d.close()
    assert ns == batch
    return counts, J, D, paths


def test_driver_windows_equal_across_slots():
    n, W = 70000, 1000
    model, tree, fp = simulate("tree", n, seed=5)
    L, B = 1, 3
    want, J, D, wpaths = _device_windows(tree, model, fp, 31, L, B, W)
    assert want.shape == (70, tree.n_nodes - 1, 16) and want[:, :, :8].any() and want[:, :, 8:].all()
    for devices in ([0], [0, 0, 0]):
        s = driver.CppSampler(L, B, devices=devices, capacity=16)
        s.enable_window_stats(W)                  # before the first reset: kept for its contexts
        s.reset(model, tree, fp)
        if len(devices) > 1:
            assert s.layout()["slots_here"] == 3
        s.run_mcmc(31, 0)
        ns, counts = s.window_stats(counts=True)
        assert ns == B and orc.paths_equal(s.paths(), wpaths)
        assert np.array_equal(counts, want)
        ns, Js, Ds = s.window_stats()
        assert ns == B and np.array_equal(Js, J) and np.array_equal(Ds, D)
        s.close()


def _write(d, name, text):
    p = os.path.join(str(d), name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_est_histories_regional_file(tmp_path):
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
    for W in (1, 100):
        want, J, D, wpaths = _device_windows(tree, model, fp, seed, L, B, W)
        f = tmp_path / ("regional_w%d.txt" % W)
        args = ("-r", f) if W == 1 else ("-r", f, "-w", W)        # the default window is one site
        assert run(tmp_path / ("with_r_w%d.local_paths" % W), *args) == plain
        r = host.read_window_stats(str(f))
        assert (r["samples"], r["window"]) == (B, W)
        assert r["node_names"] == list(tree.node_names[1:]) and np.array_equal(r["branches"], tree.branches[1:])
        assert np.array_equal(r["counts"], want)
        # k_b as written turns the integers into the API's dwell times
        Dk = want[:, :, 8:].astype(np.float64) * np.ldexp(1.0, -r["scale_exp"])[None, :, None] / float(B)
        assert np.array_equal(Dk, D)
        assert np.array_equal(r["all_J"], want[:, :, :8].sum(axis=1))
        assert np.allclose(r["all_D"], D.sum(axis=1), rtol=1e-15, atol=0)
        rho = host.regional_rate_factors(J, D, model.rates)
        assert np.array_equal(np.isnan(r["factor"]), np.isnan(rho))
        ok = ~np.isnan(rho)
        assert ok.any() and np.array_equal(r["factor"][ok], rho[ok])
    outp, _, _ = host.read_paths(str(tmp_path / "plain.local_paths"))
    assert orc.paths_equal(outp, wpaths)
    # together with the changes file: both written, the paths file still the same bytes
    f, ch = tmp_path / "both.txt", tmp_path / "changes.txt"
    assert run(tmp_path / "both.local_paths", "-r", f, "-c", ch, "-w", 100) == plain
    assert f.read_text() == (tmp_path / "regional_w100.txt").read_text() and ch.stat().st_size > 0
