"""Lineage origin maps through the C++ EM driver (epv::SingleSiteSampler, libepv_driver.so) and the
epievo_est_histories program: the same maps and window sums for one GPU slot and for EPV_DEVICES-style rehearsal
slots as DeviceSampler gives; the program's -O file holds the window sums of its run and reads back through the
reader; -O next to -c leaves the -c file (and the paths file) byte-identical."""
import os
import subprocess

import numpy as np
import pytest

import orc
import origin_ref
from common import TEST_PARAM_TEXT, TREE_NWK_TEXT, ref_test_model, simulate
from epievo_amd import _build, driver, host
from epievo_amd.sampler import DeviceSampler

pytestmark = pytest.mark.gpu


def _device_maps(tree, model, fp, seed, burn_in, batch):
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, 16)
    d.enable_lineage_origins()
    d.reset()
    d.run_mcmc(burn_in, batch, seed)
    ns, rows, origin, age = d.lineage_origins(counts=True)
    k, paths = d.lineage_origins_scale_exp(), d.paths()
    d.close()
    assert ns == batch
    return rows, origin, age, k, paths


def test_driver_maps_equal_across_slots():
    n = 70000
    model, tree, fp = simulate("tree", n, seed=5)
    L, B = 1, 3
    rows, origin, age, k, wpaths = _device_maps(tree, model, fp, 31, L, B)
    tab = origin_ref.tables(tree)
    assert np.array_equal(rows, tab["rows"]) and k == tab["k"]
    assert (origin[tab["rows"][:, 1] != 0].sum(axis=1) >= 1).all()
    for devices in ([0], [0, 0, 0]):
        s = driver.CppSampler(L, B, devices=devices, capacity=16)
        s.enable_lineage_origins()                # before the first reset: kept for its contexts
        s.reset(model, tree, fp)
        if len(devices) > 1:
            assert s.layout()["slots_here"] == 3
        s.run_mcmc(31, 0)
        assert np.array_equal(s.lineage_origin_rows(), rows)
        assert s.lineage_origins_scale_exp() == k
        ns, r2, o2, a2 = s.lineage_origins(counts=True)
        assert ns == B and o2.shape == (len(rows), n) and a2.shape == (len(tab["leaves"]), n)
        assert orc.paths_equal(s.paths(), wpaths)
        assert np.array_equal(r2, rows) and np.array_equal(o2, origin) and np.array_equal(a2, age)
        origin_ref.check_invariants(tree, o2, a2, ns, tab=tab)
        ns, _, p, mean_age = s.lineage_origins()
        assert np.array_equal(p, origin / float(B))
        assert np.array_equal(mean_age, np.ldexp(age.astype(np.float64), -k) / B)
        for W in (1000, 10 ** 6):
            nsw, ow, aw = s.lineage_origin_windows(W)
            assert nsw == B and np.array_equal(ow, origin_ref.windows(origin, W))
            assert np.array_equal(aw, origin_ref.windows(age, W))
        # one more sample of the resident paths, then from zero
        s.accumulate_lineage_origins()
        so, sa = origin_ref.sample(s.paths(), tree, tab)
        ns, _, o3, a3 = s.lineage_origins(counts=True)
        assert ns == B + 1 and np.array_equal(o3, origin + so) and np.array_equal(a3, age + sa)
        s.reset_lineage_origins()
        ns, _, o4, a4 = s.lineage_origins(counts=True)
        assert ns == 0 and not o4.any() and not a4.any()
        s.close()


def _write(d, name, text):
    p = os.path.join(str(d), name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_est_histories_origins_file(tmp_path):
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
    rows, origin, age, k, wpaths = _device_maps(tree, model, fp, seed, L, B)
    outp, _, _ = host.read_paths(str(tmp_path / "plain.local_paths"))
    assert orc.paths_equal(outp, wpaths)
    W = 100
    f = tmp_path / "origins.txt"
    assert run(tmp_path / "with_O.local_paths", "-O", f, "-w", W) == plain
    got = host.read_lineage_origins(str(f))
    assert (got["samples"], got["window"], got["scale_exp"]) == (B, W, k)
    assert got["row_leaf"] == [tree.node_names[a] for a, _ in rows]
    assert got["row_node"] == [tree.node_names[b] for _, b in rows]
    assert np.array_equal(got["origin"], origin_ref.windows(origin, W))
    assert np.array_equal(got["age"], origin_ref.windows(age, W))
    # the reader round-trips: written again from what was read, the same bytes
    again = tmp_path / "again.txt"
    host.write_lineage_origins(str(again), tree.node_names, rows, got["window"], got["samples"], got["scale_exp"],
                               got["origin"], got["age"])
    assert again.read_bytes() == f.read_bytes()
    # integers only below the row table
    body = [ln for ln in f.read_text().splitlines() if not ln.startswith(("#", "LEAF:"))]
    assert len(body) == int((rows[:, 1] == 0).sum()) * ((n + W - 1) // W)
    assert all(x.isdigit() for ln in body for x in ln.split("\t"))
    # the default window is one site
    f1 = tmp_path / "origins_w1.txt"
    assert run(tmp_path / "with_O_w1.local_paths", "-O", f1) == plain
    got1 = host.read_lineage_origins(str(f1))
    assert got1["window"] == 1 and np.array_equal(got1["origin"], origin) and np.array_equal(got1["age"], age)
    # -O together with -c: the -c file is the bytes of a run without -O, the paths file too
    c0, c1, f2 = tmp_path / "changes0.txt", tmp_path / "changes1.txt", tmp_path / "origins2.txt"
    assert run(tmp_path / "c0.local_paths", "-c", c0, "-w", W) == plain
    assert run(tmp_path / "c1.local_paths", "-c", c1, "-O", f2, "-w", W) == plain
    assert c1.read_bytes() == c0.read_bytes() and c0.stat().st_size > 0
    assert f2.read_bytes() == f.read_bytes()
