"""Change tracts through the C++ driver (epv::SingleSiteSampler behind include/epievo_mi355x_driver.h) and the
epievo_est_histories program: the merged part and the closed result of one GPU slot and of three rehearsal slots
equal the numpy yardstick on the resident paths of every batch sweep (tests/tracts_ref.py, through a DeviceSampler
that the GPU tests pin to the oracle); the program's -X file holds the closed result of its run and reads back
through the reader; -X leaves every other file the program writes byte-identical, next to every other summary
option, with -g, and with missing leaf data (-m) and leaf evidence (-l)."""
import os
import subprocess

import numpy as np
import pytest

import orc
import tracts_ref as xr
from common import TEST_PARAM_TEXT, TREE_NWK_TEXT, ref_test_model, simulate
from epievo_amd import _build, driver, host
from epievo_amd.sampler import DeviceSampler
from test_leaf_evidence import write_probs
from test_unobserved_leaves import leaf_ends, leaves, write_states

pytestmark = pytest.mark.gpu


def _yardstick(tree, model, fp, seed, burn_in, batch):
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
        p = xr.part(xr.rows(d.paths()))
        total = p if total is None else xr.add_parts(total, p)
    paths = d.paths()
    d.close()
    return total, xr.close(*total), paths


def test_driver_equals_yardstick_across_slots():
    n = 70000
    model, tree, fp = simulate("tree", n, seed=5)
    L, B = 1, 3
    nb = tree.n_nodes - 1
    part, closed, wpaths = _yardstick(tree, model, fp, 31, L, B)
    for devices in ([0], [0, 0, 0]):
        s = driver.CppSampler(L, B, devices=devices, capacity=16)
        s.enable_change_tracts(B)                 # before the first reset: kept for its contexts
        s.reset(model, tree, fp)
        if len(devices) > 1:
            assert s.layout()["slots_here"] == 3
        s.run_mcmc(31, 0)
        assert orc.paths_equal(s.paths(), wpaths)
        ns, hist, len_sum, edges = s.change_tracts_part()
        assert ns == B and edges.shape == (B, nb, 2) and np.array_equal(edges, part[2])
        assert np.array_equal(hist, part[0]) and np.array_equal(len_sum, part[1])
        ns, hist, len_sum = s.change_tracts()
        assert ns == B and np.array_equal(hist, closed[0]) and np.array_equal(len_sum, closed[1])
        with pytest.raises(driver.DriverError):   # the cap: max_samples = B
            s.accumulate_change_tracts()
        s.reset_change_tracts()
        ns, hist, len_sum = s.change_tracts()
        assert ns == 0 and not hist.any() and not len_sum.any()
        s.accumulate_change_tracts()              # one sample of the resident paths
        one = xr.part(xr.rows(s.paths()))
        ns, hist, len_sum, edges = s.change_tracts_part()
        assert ns == 1 and np.array_equal(edges, one[2]) and np.array_equal(hist, one[0])
        s.enable_change_tracts(0)
        with pytest.raises(driver.DriverError):
            s.change_tracts()
        s.close()


def _write(d, name, text):
    p = os.path.join(str(d), name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_est_histories_tracts_file(tmp_path):
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
    part, closed, wpaths = _yardstick(tree, model, fp, seed, L, B)
    outp, _, _ = host.read_paths(str(tmp_path / "plain.local_paths"))
    assert orc.paths_equal(outp, wpaths)
    f = tmp_path / "tracts.txt"
    assert run(tmp_path / "with_X.local_paths", "--tracts", f) == plain
    got = host.read_change_tracts(str(f))
    assert got["samples"] == B and got["branch_names"] == list(tree.node_names)[1:]
    assert np.array_equal(got["hist"], closed[0]) and np.array_equal(got["len_sum"], closed[1])
    lines = f.read_text().splitlines()
    assert lines[0] == "#samples\t%d\tbins\t128" % B and lines[1] == "BRANCH:" + tree.node_names[1]
    assert closed[0][0, 0].any()
    assert lines[2] == "gain\tleft\t0\tright\t0\ttracts\t%d\tsites\t%d" % (closed[0][0, 0].sum(), closed[1][0, 0])
    body = [ln for ln in lines[1:] if not ln.startswith(("BRANCH:", "gain", "loss", "mixed"))]
    assert len(body) == int((closed[0] != 0).sum()) and all(x.isdigit() for ln in body for x in ln.split("\t"))
    s = host.change_tract_summary(got["samples"], got["hist"], got["len_sum"], tree)
    assert all(s[k].sum() > 0 for k in host.TRACT_EVENTS)
    # the reader round-trips: written again from what was read, the same bytes
    again = tmp_path / "again.txt"
    host.write_change_tracts(str(again), got["branch_names"], got["samples"], got["hist"], got["len_sum"])
    assert again.read_bytes() == f.read_bytes()
    # -X next to every other summary, with -g: each of their files is the bytes of a run without -X
    others = ["a", "c", "r", "O", "d", "E", "P", "R", "C", "x", "D"]
    opts0 = sum((["-" + o, tmp_path / ("%s0.txt" % o)] for o in others), []) + ["-g", "0"]
    opts1 = sum((["-" + o, tmp_path / ("%s1.txt" % o)] for o in others), []) + ["-g", "0", "-X", tmp_path / "X1.txt"]
    assert run(tmp_path / "all0.local_paths", *opts0) == plain
    assert run(tmp_path / "all1.local_paths", *opts1) == plain
    for o in others:
        a, b = tmp_path / ("%s0.txt" % o), tmp_path / ("%s1.txt" % o)
        assert a.stat().st_size > 0 and a.read_bytes() == b.read_bytes(), o
    assert (tmp_path / "X1.txt").read_bytes() == f.read_bytes()
    # missing leaf data and leaf evidence: the paths are those of the run without -X, the file differs from the
    # observed run's (the leaf's changes move)
    ends = leaf_ends(tree, fp)
    lv = leaves(tree)
    miss = [(lv[0], s) for s in range(100, 160)]
    write_states(str(tmp_path / "m.states"), tree, lv, ends, missing=miss)
    m0 = run(tmp_path / "m0.local_paths", "-m", tmp_path / "m.states")
    assert run(tmp_path / "m1.local_paths", "-m", tmp_path / "m.states", "-X", tmp_path / "Xm.txt") == m0
    assert host.read_change_tracts(str(tmp_path / "Xm.txt"))["samples"] == B
    assert (tmp_path / "Xm.txt").read_bytes() != f.read_bytes()
    write_probs(str(tmp_path / "l.probs"), tree, lv, ends, {cell: "0.4" for cell in miss})
    l0 = run(tmp_path / "l0.local_paths", "-l", tmp_path / "l.probs")
    assert run(tmp_path / "l1.local_paths", "-l", tmp_path / "l.probs", "-X", tmp_path / "Xl.txt") == l0
    assert host.read_change_tracts(str(tmp_path / "Xl.txt"))["samples"] == B
