"""Domain maps through the C++ driver (epv::SingleSiteSampler behind include/epievo_mi355x_driver.h) and the
epievo_est_histories program: the merged part of one GPU slot and of three rehearsal slots equals the numpy yardstick
on the resident paths of every batch sweep (tests/domain_maps_ref.py, through a DeviceSampler that the GPU tests pin to
the oracle); the program's -D file holds the window sums of its run and reads back through host.read_domain_maps; -D
leaves every other file the program writes byte-identical, next to every other summary option and with -g."""
import os
import subprocess

import numpy as np
import pytest

import domain_maps_ref as mr
import orc
from common import TEST_PARAM_TEXT, TREE_NWK_TEXT, ref_test_model, simulate
from epievo_amd import _build, driver, host
from epievo_amd.sampler import DeviceSampler

pytestmark = pytest.mark.gpu


def _yardstick(tree, model, fp, seed, burn_in, batch, sizes, state):
    """the yardstick on a DeviceSampler's paths after every batch sweep -> (part, final paths)"""
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
        p = mr.part(mr.rows(d.paths(), tree, state), sizes)
        total = p if total is None else mr.add_parts(total, p)
    paths = d.paths()
    d.close()
    return total, paths


def test_driver_equals_yardstick_across_slots():
    n, sizes, state = 70000, (1, 5, 20), 0
    model, tree, fp = simulate("tree", n, seed=5)
    L, B = 1, 3
    N = tree.n_nodes
    part, wpaths = _yardstick(tree, model, fp, 31, L, B, sizes, state)
    for devices in ([0], [0, 0, 0]):
        s = driver.CppSampler(L, B, devices=devices, capacity=16)
        s.enable_domain_maps(sizes, state, B)         # before the first reset: kept for its contexts
        s.reset(model, tree, fp)
        if len(devices) > 1:
            assert s.layout()["slots_here"] == 3
        s.run_mcmc(31, 0)
        assert orc.paths_equal(s.paths(), wpaths)
        ns, cnt, counts, edges = s.domain_maps_part()
        assert ns == B and cnt == n and edges.shape == (B, N, 2, 1) and np.array_equal(edges, part[2])
        assert counts.dtype == np.uint32 and np.array_equal(counts, part[1])
        ns, maps = s.domain_maps()
        assert ns == B and np.array_equal(maps, part[1] / float(B))
        with pytest.raises(driver.DriverError):   # the cap: max_samples = B
            s.accumulate_domain_maps()
        s.reset_domain_maps()
        got = s.domain_maps_part()
        assert got[0] == 0 and not got[2].any()
        s.accumulate_domain_maps()                # one sample of the resident paths
        one = mr.part(mr.rows(s.paths(), tree, state), sizes)
        ns, cnt, counts, edges = s.domain_maps_part()
        assert ns == 1 and np.array_equal(edges, one[2]) and np.array_equal(counts, one[1])
        s.enable_domain_maps(())
        with pytest.raises(driver.DriverError):
            s.domain_maps()
        s.close()


def _write(d, name, text):
    p = os.path.join(str(d), name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_est_histories_maps_file(tmp_path):
    model = ref_test_model()
    tree = host.Tree.read(_write(tmp_path, "tree.nwk", TREE_NWK_TEXT))
    param = _write(tmp_path, "test.param", TEST_PARAM_TEXT)
    n = 3001
    fp = host.simulate(model, tree, n, 12)
    inp = str(tmp_path / "in.local_paths")
    host.write_paths(inp, tree.node_names, tree.branches, fp)     # tot_time = branch length: no rescale
    exe = os.path.join(_build.BIN_DIR, "epievo_est_histories")
    seed, L, B = 17, 2, 4

    def run(out, *extra, ok=True):
        r = subprocess.run([str(x) for x in [exe, "-L", L, "-B", B, "-s", seed, "-o", out, *extra, param,
                                          tmp_path / "tree.nwk", inp]], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True)
        assert (r.returncode == 0) == ok, r.stderr
        return open(str(out), "rb").read() if ok else r.stderr

    plain = run(tmp_path / "plain.local_paths")
    part, wpaths = _yardstick(tree, model, fp, seed, L, B, (5, 20), 1)
    outp, _, _ = host.read_paths(str(tmp_path / "plain.local_paths"))
    assert orc.paths_equal(outp, wpaths)
    f = tmp_path / "maps.txt"
    assert run(tmp_path / "with_D.local_paths", "-D", f) == plain             # -z defaults to 5,20, -S to 1, -w to 1
    got = host.read_domain_maps(str(f))
    assert (got["samples"], got["sites"], got["window"], got["state"]) == (B, n, 1, 1)
    assert got["sizes"].tolist() == [5, 20] and got["node_names"] == list(tree.node_names)
    assert np.array_equal(got["sums"], part[1])                                # windows of one site: the maps themselves
    lines = f.read_text().splitlines()
    assert lines[0] == "#samples\t%d\tstate\t1\tsizes\t5\t20" % B and lines[1] == "#window\t1\tsites\t%d" % n
    assert lines[2] == "NODE:" + tree.node_names[0] and len(lines) == 2 + tree.n_nodes * (n + 1)
    body = [ln for ln in lines[2:] if not ln.startswith("NODE:")]
    assert all(x.isdigit() for ln in body for x in ln.split("\t"))
    # the options of the issue's command line: state 0, three sizes, windows of 1000 sites
    g = tmp_path / "maps0.txt"
    assert run(tmp_path / "with_z.local_paths", "-D", g, "-z", "1,5,20", "-S", 0, "-w", 1000) == plain
    part0, _ = _yardstick(tree, model, fp, seed, L, B, (1, 5, 20), 0)
    got0 = host.read_domain_maps(str(g))
    assert (got0["window"], got0["state"], got0["sizes"].tolist()) == (1000, 0, [1, 5, 20])
    assert np.array_equal(got0["sums"], host.domain_map_windows(part0[1], 1000))
    # the reader round-trips: written again from what was read, the same bytes
    again = tmp_path / "again.txt"
    host.write_domain_maps(str(again), got0["node_names"], got0["samples"], got0["state"], got0["sizes"], got0["sites"],
                           got0["window"], got0["sums"])
    assert again.read_bytes() == g.read_bytes()
    # -D next to every other summary, with -g: each of their files is the bytes of a run without -D
    others = ["a", "c", "r", "O", "d", "E", "P", "R", "C", "x"]
    opts0 = sum((["-" + o, tmp_path / ("%s0.txt" % o)] for o in others), []) + ["-g", "0"]
    opts1 = sum((["-" + o, tmp_path / ("%s1.txt" % o)] for o in others), []) + ["-g", "0", "-D", tmp_path / "D1.txt"]
    assert run(tmp_path / "all0.local_paths", *opts0) == plain
    assert run(tmp_path / "all1.local_paths", *opts1) == plain
    for o in others:
        a, b = tmp_path / ("%s0.txt" % o), tmp_path / ("%s1.txt" % o)
        assert a.stat().st_size > 0 and a.read_bytes() == b.read_bytes(), o
    assert (tmp_path / "D1.txt").read_bytes() == f.read_bytes()
    # refusals of the command line
    for bad in (["-z", "5,5"], ["-z", "0"], ["-z", "1025"], ["-z", "1,2,3,4,5"], ["-z", "5,x"], ["-S", 2]):
        assert run(tmp_path / "bad.local_paths", "-D", tmp_path / "bad.txt", *bad, ok=False)
    assert "-D/--maps" in run(tmp_path / "bad.local_paths", "-z", "5", ok=False)
