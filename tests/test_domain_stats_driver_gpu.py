"""Domain size spectra through the C++ driver (epv::SingleSiteSampler behind include/epievo_mi355x_driver.h) and the
epievo_est_histories program: the merged part and the closed result of one GPU slot and of three rehearsal slots
equal the numpy yardstick on the resident paths of every batch sweep (tests/domains_ref.py, through a
DeviceSampler that the GPU tests pin to the oracle); the program's -d file holds the closed result of its run and
reads back through the reader; -d leaves the paths file byte-identical, alone and next to -c."""
import os
import subprocess

import numpy as np
import pytest

import domains_ref as dr
import orc
from common import TEST_PARAM_TEXT, TREE_NWK_TEXT, ref_test_model, simulate
from epievo_amd import _build, driver, host
from epievo_amd.sampler import DeviceSampler

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
        p = dr.part(dr.node_states(d.paths(), tree))
        total = p if total is None else dr.add_parts(total, p)
    paths = d.paths()
    d.close()
    return total, dr.close(*total), paths


def test_driver_equals_yardstick_across_slots():
    n = 70000
    model, tree, fp = simulate("tree", n, seed=5)
    L, B = 1, 3
    part, closed, wpaths = _yardstick(tree, model, fp, 31, L, B)
    for devices in ([0], [0, 0, 0]):
        s = driver.CppSampler(L, B, devices=devices, capacity=16)
        s.enable_domain_stats(B)                  # before the first reset: kept for its contexts
        s.reset(model, tree, fp)
        if len(devices) > 1:
            assert s.layout()["slots_here"] == 3
        s.run_mcmc(31, 0)
        assert orc.paths_equal(s.paths(), wpaths)
        ns, hist, len_sum, edges = s.domain_stats_part()
        assert ns == B and np.array_equal(edges, part[2])
        assert np.array_equal(hist, part[0]) and np.array_equal(len_sum, part[1])
        ns, hist, len_sum = s.domain_stats()
        assert ns == B and np.array_equal(hist, closed[0]) and np.array_equal(len_sum, closed[1])
        assert (len_sum.sum(axis=1) == B * n).all()
        with pytest.raises(driver.DriverError):   # the cap: max_samples = B
            s.accumulate_domain_stats()
        s.reset_domain_stats()
        ns, hist, len_sum = s.domain_stats()
        assert ns == 0 and not hist.any() and not len_sum.any()
        s.accumulate_domain_stats()               # one sample of the resident paths
        one = dr.part(dr.node_states(s.paths(), tree))
        ns, hist, len_sum, edges = s.domain_stats_part()
        assert ns == 1 and np.array_equal(edges, one[2]) and np.array_equal(hist, one[0])
        s.close()


def _write(d, name, text):
    p = os.path.join(str(d), name)
    with open(p, "w") as f:
        f.write(text)
    return p


def test_est_histories_domains_file(tmp_path):
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
    f = tmp_path / "domains.txt"
    assert run(tmp_path / "with_d.local_paths", "-d", f) == plain
    got = host.read_domain_stats(str(f))
    assert got["samples"] == B and got["node_names"] == list(tree.node_names)
    assert np.array_equal(got["hist"], closed[0]) and np.array_equal(got["len_sum"], closed[1])
    lines = f.read_text().splitlines()
    assert lines[0] == "#samples\t%d\tbins\t128" % B and lines[1] == "NODE:" + tree.node_names[0]
    body = [ln for ln in lines[1:] if not ln.startswith(("NODE:", "state"))]
    assert len(body) == int((closed[0] != 0).sum()) and all(x.isdigit() for ln in body for x in ln.split("\t"))
    # the reader round-trips: written again from what was read, the same bytes
    again = tmp_path / "again.txt"
    host.write_domain_stats(str(again), got["node_names"], got["samples"], got["hist"], got["len_sum"])
    assert again.read_bytes() == f.read_bytes()
    # -d together with -c: the -c file is the bytes of a run without -d, the paths file too
    c0, c1, f2 = tmp_path / "changes0.txt", tmp_path / "changes1.txt", tmp_path / "domains2.txt"
    assert run(tmp_path / "c0.local_paths", "-c", c0) == plain
    assert run(tmp_path / "c1.local_paths", "-c", c1, "-d", f2) == plain
    assert c1.read_bytes() == c0.read_bytes() and c0.stat().st_size > 0
    assert f2.read_bytes() == f.read_bytes()
