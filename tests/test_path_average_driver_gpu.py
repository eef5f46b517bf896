"""The average history through the C++ EM driver (epv::SingleSiteSampler, libepv_driver.so) and the
epievo_est_histories program: the same counts for one GPU slot and for EPV_DEVICES-style rehearsal
slots, equal to the counts numpy computes from the CPU oracle's batch-sweep paths; the program's
average file byte-equals the numpy-formatted average, and average_paths over its paths file gives
the bytes of its own -B 1 average."""
import os
import subprocess

import numpy as np
import pytest

import orc
import pavg_ref
from common import TEST_PARAM_TEXT, TREE_NWK_TEXT, ref_test_model, simulate
from epievo_amd import _build, driver, host

pytestmark = pytest.mark.gpu


def _oracle_counts(tree, model, fp, seed, burn_in, batch, P):
    o = orc.Oracle(tree, model, fp, "B", cap=16, seed=seed)
    o.reset()
    for w in range(burn_in):
        o.sweep(w)
    cnt = np.zeros((tree.n_nodes - 1, fp.n_sites, P), np.uint32)
    for w in range(batch):
        o.sweep(burn_in + w)
        cnt += pavg_ref.counts(o.paths(), tree.branches, P)
    return cnt, o.paths()


def test_driver_counts_equal_across_slots():
    model, tree, fp = simulate("tree", 70000, seed=5)
    P, L, B = 9, 1, 3
    got = []
    for devices in ([0], [0, 0, 0, 0]):
        s = driver.CppSampler(L, B, devices=devices, capacity=16)
        s.enable_path_average(P)                  # before the first reset: kept for its contexts
        s.reset(model, tree, fp)
        if len(devices) > 1:
            assert s.layout()["slots_here"] == 4
        s.run_mcmc(31, 0)
        ns, cnt = s.path_average(counts=True)
        assert ns == B and cnt.shape == (tree.n_nodes - 1, 70000, P)      # sites 0 and n - 1 included
        got.append((cnt, s.paths()))
        s.close()
    assert np.array_equal(got[0][0], got[1][0])
    assert orc.paths_equal(got[0][1], got[1][1])
    want, opaths = _oracle_counts(tree, model, fp, 31, L, B, P)
    assert orc.paths_equal(got[0][1], opaths)
    assert np.array_equal(got[0][0], want)


def _write(d, name, text):
    p = os.path.join(str(d), name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_est_histories_average_file(tmp_path):
    model = ref_test_model()
    tree = host.Tree.read(_write(tmp_path, "tree.nwk", TREE_NWK_TEXT))
    param = _write(tmp_path, "test.param", TEST_PARAM_TEXT)
    fp = host.simulate(model, tree, 3000, 12)
    inp = str(tmp_path / "in.local_paths")
    host.write_paths(inp, tree.node_names, tree.branches, fp)     # tot_time = branch length: no rescale
    exe = os.path.join(_build.BIN_DIR, "epievo_est_histories")
    seed, L, B, P = 17, 2, 4, 50
    avg, out = tmp_path / "avg.txt", tmp_path / "out" / "final.local_paths"
    out.parent.mkdir()
    r = subprocess.run([str(x) for x in [exe, "-L", L, "-B", B, "-s", seed, "-a", avg, "-n", P, "-o", out, param,
                                      tmp_path / "tree.nwk", inp]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    want, opaths = _oracle_counts(tree, model, fp, seed, L, B, P)
    assert avg.read_text() == pavg_ref.format_average(tree.node_names, tree.branches, want, B)
    s = driver.CppSampler(L, B, devices=[0], capacity=16)
    s.reset(model, tree, fp)
    s.run_mcmc(seed, 0)
    outp, _, _ = host.read_paths(str(out))
    assert orc.paths_equal(outp, s.paths()) and orc.paths_equal(outp, opaths)
    s.close()
    # average_paths over that one file == the program's own average of one batch sweep
    avg1, avg2 = tmp_path / "avg1.txt", tmp_path / "avg2.txt"
    r = subprocess.run([str(x) for x in [exe, "-L", L, "-B", 1, "-s", seed, "-a", avg1, "-n", P, "-o", tmp_path / "one.local_paths",
                                      param, tmp_path / "tree.nwk", inp]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    one = tmp_path / "one"
    one.mkdir()
    os.replace(str(tmp_path / "one.local_paths"), str(one / "x.local_paths"))
    r = subprocess.run([str(x) for x in [os.path.join(_build.BIN_DIR, "average_paths"), "-n", P, "-o", avg2, one]],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    assert avg1.read_text() == avg2.read_text()
