"""Spatial correlations through the C++ driver (epv::SingleSiteSampler behind include/epievo_mi355x_driver.h) and the
epievo_est_histories program: the merged part and the closed result of one GPU slot and of three rehearsal slots
equal the numpy yardstick on the resident paths of every batch sweep (tests/corr_ref.py, through a DeviceSampler
that the GPU tests pin to the oracle); the program's -C file holds the closed result of its run and reads back
through the reader; -C leaves every other file the program writes byte-identical, next to every other summary
option, with -g, and with missing leaf data (-m) and leaf evidence (-l)."""
import os
import subprocess

import numpy as np
import pytest

import corr_ref as cr
import orc
from common import TEST_PARAM_TEXT, TREE_NWK_TEXT, ref_test_model, simulate
from epievo_amd import _build, driver, host
from epievo_amd.sampler import DeviceSampler
from test_leaf_evidence import write_probs
from test_unobserved_leaves import leaf_ends, leaves, write_states

pytestmark = pytest.mark.gpu


def _yardstick(tree, model, fp, seed, burn_in, batch, max_lag):
    """the yardstick on a DeviceSampler's paths after every batch sweep -> (part, closed, final paths)"""
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, 16)
    d.reset()
    if burn_in:
        d.sweep(burn_in, seed, sweep_base=0)
    total = None
    for w in range(batch):
        d.sweep(1, seed, sweep_base=burn_in + w)
        p = cr.part(cr.rows(d.paths(), tree), max_lag)
        total = p if total is None else cr.add_parts(total, p)
    paths = d.paths()
    d.close()
    return total, cr.close(*total), paths


def test_driver_equals_yardstick_across_slots():
    n, M = 70000, 300
    model, tree, fp = simulate("tree", n, seed=5)
    L, B = 1, 3
    R, LW = 2 * tree.n_nodes - 1, (M + 63) // 64
    part, closed, wpaths = _yardstick(tree, model, fp, 31, L, B, M)
    for devices in ([0], [0, 0, 0]):
        s = driver.CppSampler(L, B, devices=devices, capacity=16)
        s.enable_spatial_correlation(M, B)        # before the first reset: kept for its contexts
        s.reset(model, tree, fp)
        if len(devices) > 1:
            assert s.layout()["slots_here"] == 3
        s.run_mcmc(31, 0)
        assert orc.paths_equal(s.paths(), wpaths)
        ns, cnt, n11, edges = s.spatial_correlation_part()
        assert ns == B and cnt == n and edges.shape == (B, R, 2, LW) and np.array_equal(edges, part[2])
        assert np.array_equal(n11, part[1])
        got = s.spatial_correlation()
        assert got[0] == B and all(np.array_equal(g, w) for g, w in zip(got[1:], closed))
        with pytest.raises(driver.DriverError):   # the cap: max_samples = B
            s.accumulate_spatial_correlation()
        s.reset_spatial_correlation()
        got = s.spatial_correlation()
        assert got[0] == 0 and not any(a.any() for a in got[1:])
        s.accumulate_spatial_correlation()        # one sample of the resident paths
        one = cr.part(cr.rows(s.paths(), tree), M)
        ns, cnt, n11, edges = s.spatial_correlation_part()
        assert ns == 1 and np.array_equal(edges, one[2]) and np.array_equal(n11, one[1])
        s.enable_spatial_correlation(0, 0)
        with pytest.raises(driver.DriverError):
            s.spatial_correlation()
        s.close()


def _write(d, name, text):
    p = os.path.join(str(d), name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_est_histories_correlation_file(tmp_path):
    model = ref_test_model()
    tree = host.Tree.read(_write(tmp_path, "tree.nwk", TREE_NWK_TEXT))
    param = _write(tmp_path, "test.param", TEST_PARAM_TEXT)
    n = 3001
    fp = host.simulate(model, tree, n, 12)
    inp = str(tmp_path / "in.local_paths")
    host.write_paths(inp, tree.node_names, tree.branches, fp)     # tot_time = branch length: no rescale
    exe = os.path.join(_build.BIN_DIR, "epievo_est_histories")
    seed, L, B = 17, 2, 4
    N = tree.n_nodes

    def run(out, *extra):
        r = subprocess.run([str(x) for x in [exe, "-L", L, "-B", B, "-s", seed, "-o", out, *extra, param,
                                          tmp_path / "tree.nwk", inp]], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True)
        assert r.returncode == 0, r.stderr
        return open(str(out), "rb").read()

    plain = run(tmp_path / "plain.local_paths")
    part, closed, wpaths = _yardstick(tree, model, fp, seed, L, B, 64)
    outp, _, _ = host.read_paths(str(tmp_path / "plain.local_paths"))
    assert orc.paths_equal(outp, wpaths)
    f = tmp_path / "corr.txt"
    assert run(tmp_path / "with_C.local_paths", "-C", f) == plain             # -M defaults to 64
    got = host.read_spatial_correlation(str(f))
    names = list(tree.node_names)
    assert got["samples"] == B and got["sites"] == n and got["max_lag"] == 64
    assert got["row_names"] == ["NODE:" + s for s in names] + ["BRANCH:" + s for s in names[1:]]
    assert all(np.array_equal(got[k], w) for k, w in zip(("n11", "left1", "right1"), closed))
    lines = f.read_text().splitlines()
    assert lines[0] == "#samples\t%d\tsites\t%d\tmax_lag\t64" % (B, n) and lines[1] == "NODE:" + names[0]
    assert lines[2] == "ones\t%d" % closed[0][0, 0]
    assert lines[3] == "1\t%d\t%d\t%d" % (closed[0][0, 1], closed[1][0, 1], closed[2][0, 1])
    assert len(lines) == 1 + (2 * N - 1) * 66
    body = [ln for ln in lines[1:] if not ln.startswith(("NODE:", "BRANCH:", "ones"))]
    assert all(x.isdigit() for ln in body for x in ln.split("\t"))
    s = host.spatial_correlation_summary(got["samples"], got["sites"], got["n11"], got["left1"], got["right1"], tree)
    assert (s["corr"][:N, 1] > 0.2).all()                                     # neighbouring sites agree
    # another max_lag: the shared lags are the same integers
    g = tmp_path / "corr130.txt"
    assert run(tmp_path / "with_M.local_paths", "-C", g, "-M", 130) == plain
    got130 = host.read_spatial_correlation(str(g))
    assert got130["max_lag"] == 130 and all(np.array_equal(got130[k][:, :65], got[k]) for k in ("n11", "left1", "right1"))
    # the reader round-trips: written again from what was read, the same bytes
    again = tmp_path / "again.txt"
    host.write_spatial_correlation(str(again), names, got["samples"], got["sites"], got["n11"], got["left1"],
                                   got["right1"])
    assert again.read_bytes() == f.read_bytes()
    # -C next to every other summary, with -g: each of their files is the bytes of a run without -C
    others = ["a", "c", "r", "O", "d", "E", "P", "R"]
    opts0 = sum((["-" + o, tmp_path / ("%s0.txt" % o)] for o in others), []) + ["-g", "0"]
    opts1 = sum((["-" + o, tmp_path / ("%s1.txt" % o)] for o in others), []) + ["-g", "0", "-C", tmp_path / "C1.txt"]
    assert run(tmp_path / "all0.local_paths", *opts0) == plain
    assert run(tmp_path / "all1.local_paths", *opts1) == plain
    for o in others:
        a, b = tmp_path / ("%s0.txt" % o), tmp_path / ("%s1.txt" % o)
        assert a.stat().st_size > 0 and a.read_bytes() == b.read_bytes(), o
    assert (tmp_path / "C1.txt").read_bytes() == f.read_bytes()
    # missing leaf data and leaf evidence: the paths are those of the run without -C, the file differs from the
    # observed run's (the leaf's row moves)
    ends = leaf_ends(tree, fp)
    lv = leaves(tree)
    miss = [(lv[0], s) for s in range(100, 160)]
    write_states(str(tmp_path / "m.states"), tree, lv, ends, missing=miss)
    m0 = run(tmp_path / "m0.local_paths", "-m", tmp_path / "m.states")
    assert run(tmp_path / "m1.local_paths", "-m", tmp_path / "m.states", "-C", tmp_path / "Cm.txt") == m0
    assert host.read_spatial_correlation(str(tmp_path / "Cm.txt"))["samples"] == B
    assert (tmp_path / "Cm.txt").read_bytes() != f.read_bytes()
    write_probs(str(tmp_path / "l.probs"), tree, lv, ends, {cell: "0.4" for cell in miss})
    l0 = run(tmp_path / "l0.local_paths", "-l", tmp_path / "l.probs")
    assert run(tmp_path / "l1.local_paths", "-l", tmp_path / "l.probs", "-C", tmp_path / "Cl.txt") == l0
    assert host.read_spatial_correlation(str(tmp_path / "Cl.txt"))["samples"] == B
