"""Epoch statistics through the C++ EM driver (epv::SingleSiteSampler, libepv_driver.so) and the
epievo_est_histories program: one GPU slot and three rehearsal slots give the closed integers DeviceSampler gives;
the program's -E file parses (epv_io's reader) to the API's numbers, and -E changes nothing in the other files."""
import os
import subprocess

import numpy as np
import pytest

import epoch_ref
import orc
from common import TEST_PARAM_TEXT, TREE_NWK_TEXT, ref_test_model, simulate
from epievo_amd import _build, driver, host
from epievo_amd.sampler import DeviceSampler

pytestmark = pytest.mark.gpu


def _device_epochs(tree, model, fp, seed, burn_in, batch, P):
    """a DeviceSampler's run next to a rung-B oracle of the same Philox sweeps: the closed integers equal the
    yardstick's, and the case is a real one on the oracle's own paths"""
    o = orc.Oracle(tree, model, fp, "B", cap=16, seed=seed)
    o.reset()
    y = epoch_ref.Yard(o, tree, (P,))
    for w in range(burn_in):
        o.sweep(w)
    for w in range(batch):
        o.sweep(burn_in + w)
        y.add()
    y.assert_not_vacuous()
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, 16)
    d.enable_epoch_stats(P)
    d.reset()
    c, _ = d.run_mcmc_counts(burn_in, batch, seed)
    ns, Jc, Dc = d.epoch_stats(counts=True)
    _, J, D = d.epoch_stats()
    _, k, fixT = d.epoch_stats_layout()
    paths = d.paths()
    d.close()
    assert ns == batch and orc.paths_equal(paths, o.paths())
    assert np.array_equal(Jc, y.J[P].astype(np.int64)) and (Dc == y.D[P]).all()          # identity B
    tot = c.reshape(batch, tree.n_nodes - 1, 16).sum(axis=0)                 # identity A
    assert np.array_equal(Jc.sum(axis=1), tot[:, :8]) and (Dc.sum(axis=1) == tot[:, 8:].astype(object)).all()
    return Jc, Dc, J, D, k, fixT, paths


def test_driver_epochs_equal_across_slots(monkeypatch):
    monkeypatch.setenv("EPV_ROW_BLOCKS", "4")     # slot cuts on 1024-site rows: three slots fit a short genome
    n, P = 12000, 100
    model, tree, fp = simulate("tree", n, seed=5)
    L, B = 1, 2
    Jc, Dc, J, D, k, fixT, wpaths = _device_epochs(tree, model, fp, 31, L, B, P)
    assert Jc.shape == (tree.n_nodes - 1, P, 8) and (Jc.sum(axis=2) > 0).sum(axis=1).min() >= 2 and Dc.any()
    for devices in ([0], [0, 0, 0]):
        s = driver.CppSampler(L, B, devices=devices, capacity=16)
        s.enable_epoch_stats(P)                   # before the first reset: kept for its contexts
        s.reset(model, tree, fp)
        if len(devices) > 1:
            assert s.layout()["slots_here"] == 3
        s.run_mcmc(31, 0)
        ns, Js, Ds = s.epoch_stats(counts=True)
        assert ns == B and orc.paths_equal(s.paths(), wpaths)
        assert np.array_equal(Js, Jc) and (Ds == Dc).all()
        ns, Jf, Df = s.epoch_stats()
        assert ns == B and np.array_equal(Jf, J) and np.array_equal(Df, D)
        s.close()


def _write(d, name, text):
    p = os.path.join(str(d), name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_est_histories_epochs_file(tmp_path):
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

    plain = run(tmp_path / "plain.local_paths", "-r", tmp_path / "plain_r.txt", "-w", 100, "-a", tmp_path / "plain_a.txt")
    for P in (10, 7):                             # (>= 3: a case can be a real one)
        Jc, Dc, J, D, k, fixT, wpaths = _device_epochs(tree, model, fp, seed, L, B, P)
        f = tmp_path / ("epochs_%d.txt" % P)
        args = ("-E", f) if P == 10 else ("-E", f, "-K", P)       # the default is ten epochs
        assert run(tmp_path / ("with_E_%d.local_paths" % P), *args) == plain
        r = host.read_epoch_stats(str(f))
        assert (r["samples"], r["epochs"]) == (B, P)
        assert r["node_names"] == list(tree.node_names[1:]) and np.array_equal(r["branches"], tree.branches[1:])
        assert np.array_equal(r["scale_exp"], k)
        assert np.array_equal(r["J"], Jc) and (r["D"] == Dc).all()
        for b in range(tree.n_nodes - 1):
            assert np.array_equal(r["start"][b], host.epoch_edges(fixT[b], P).astype(np.float64) / float(fixT[b]))
        rho = host.epoch_rate_factors(J, D, model.rates)
        ok = ~np.isnan(rho)
        assert ok.all() and np.allclose(r["factor"], rho, rtol=1e-14, atol=0)
    outp, _, _ = host.read_paths(str(tmp_path / "plain.local_paths"))
    assert orc.paths_equal(outp, wpaths)
    # together with the other outputs: all written, every other file still the same bytes
    f, rg, av = tmp_path / "both.txt", tmp_path / "both_r.txt", tmp_path / "both_a.txt"
    assert run(tmp_path / "both.local_paths", "-E", f, "-K", 7, "-r", rg, "-w", 100, "-a", av) == plain
    assert f.read_text() == (tmp_path / "epochs_7.txt").read_text()
    assert rg.read_bytes() == (tmp_path / "plain_r.txt").read_bytes()
    assert av.read_bytes() == (tmp_path / "plain_a.txt").read_bytes()
    # -K without -E, and too many epochs, are refused
    for extra in (("-K", 7), ("-E", f, "-K", 257)):
        r = subprocess.run([str(x) for x in [exe, "-L", 0, "-B", 1, "-s", 1, "-o", tmp_path / "x", *extra, param,
                                          tmp_path / "tree.nwk", inp]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode != 0
