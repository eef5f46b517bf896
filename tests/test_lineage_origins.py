"""Lineage origin maps, the parts that need no GPU: the numpy yardstick (tests/origin_ref.py) against a plain
per-site walk up every leaf's lineage, the invariants of a sample (a leaf's rows sum to one, the leaf-branch row
is the branch events' `changed` plane, the root row counts the jump-free lineages, the age bound), the
fixed-point scale k and fixT on trees of very different heights, window sums, the file of epievo_est_histories
-O through its writer and reader, and the option errors of the program (raised before a device is opened).
The device side is in test_lineage_origins_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import bevents_ref
import origin_ref
from common import config, simulate
from epievo_amd import _build, host

EXE = os.path.join(_build.BIN_DIR, "epievo_est_histories")


@pytest.fixture(scope="module", params=[("tree", 257), ("cat6", 300)], ids=["tree257", "cat6x300"])
def one(request):
    cfg, n = request.param
    model, tree, fp = simulate(cfg, n, seed=6)
    return tree, fp, origin_ref.tables(tree), origin_ref.sample(fp, tree)


def test_yardstick_equals_walking_the_lineages(one):
    tree, fp, tab, (origin, age) = one
    L, R = len(tab["leaves"]), len(tab["rows"])
    assert origin.dtype == np.uint32 and origin.shape == (R, fp.n_sites)
    assert age.dtype == np.uint64 and age.shape == (L, fp.n_sites)
    bo, ba = origin_ref.brute(fp, tree)
    assert np.array_equal(origin, bo) and np.array_equal(age, ba)
    # not vacuous: every non-root row of every leaf holds a site (tree.nwk at n = 257: at least 6), and so does
    # every root row
    non_root = tab["rows"][:, 1] != 0
    assert (origin[non_root].sum(axis=1) >= 1).all() and (origin[~non_root].sum(axis=1) >= 1).all()


def test_row_table(one):
    tree, fp, tab, _ = one
    parent, sub = tree.parent_ids, tree.subtree_sizes
    rows = tab["rows"]
    assert tab["leaves"] == [v for v in range(1, tree.n_nodes) if sub[v] == 1]
    assert len(rows) == sum(1 + _depth(parent, v) for v in tab["leaves"])
    for li, leaf in enumerate(tab["leaves"]):
        r0, r1 = tab["first"][li], tab["first"][li + 1]
        assert r1 - r0 == _depth(parent, leaf) + 1 and (rows[r0:r1, 0] == leaf).all()
        assert rows[r0, 1] == leaf and rows[r1 - 1, 1] == 0 and parent[rows[r1 - 2, 1]] == 0
        assert all(rows[r + 1, 1] == parent[rows[r, 1]] for r in range(r0, r1 - 1))


def _depth(parent, v):
    d = 0
    while v != 0:
        v, d = int(parent[v]), d + 1
    return d


def test_invariants_of_one_sample(one):
    tree, fp, tab, (origin, age) = one
    changed = bevents_ref.counts(fp)[3]
    origin_ref.check_invariants(tree, origin, age, 1, changed=changed, tab=tab)
    cnt = fp.counts().reshape(tree.n_nodes - 1, -1)
    for li in range(len(tab["leaves"])):
        r0, r1 = tab["first"][li], tab["first"][li + 1]
        lineage = tab["rows"][r0:r1 - 1, 1].astype(np.int64) - 1
        any_jump = (cnt[lineage] >= 1).any(axis=0)
        assert np.array_equal(origin[r1 - 1], 1 - any_jump.astype(np.uint32))      # the root row
    # the invariants add up over samples: two samples of the same paths
    origin_ref.check_invariants(tree, origin * np.uint32(2), age * np.uint64(2), 2, changed=changed * np.uint32(2),
                                tab=tab)


def _scaled(tree, f):
    return host.Tree(tree.subtree_sizes, tree.parent_ids, tree.branches * f, tree.node_names)


def test_scale_and_fixed_branch_lengths():
    # tree.nwk: the longest lineage is C or D through E, 0.06 + 0.02, or F alone, 0.1 = 0.8 * 2^-3: e = -3
    tree = config("tree")
    tab = origin_ref.tables(tree)
    assert tab["H"] == 0.1 and tab["k"] == 43
    assert np.array_equal(tab["fixT"][1:], np.rint(tree.branches[1:] * 2.0 ** 43).astype(np.int64))
    assert tab["fixT"][0] == 0 and int(tab["fixT"].max()) < 2 ** 40
    # pair, T = 1 = 0.5 * 2^1: e = 1, k = 39, fixT = 2^39 exactly
    tab = origin_ref.tables(config("pair"))
    assert tab["H"] == 1.0 and tab["k"] == 39 and tab["fixT"].tolist() == [0, 2 ** 39]
    assert tab["rows"].tolist() == [[1, 1], [1, 0]] and tab["first"] == [0, 2]
    # scaled by 1e-6 and 1e6: k follows the height, the integers keep 40 bits of the longest lineage
    for f in (1e-6, 1e6):
        t = _scaled(tree, f)
        tab = origin_ref.tables(t)
        e = int(np.frexp(tab["H"])[1])
        assert tab["k"] == 40 - e
        assert 2 ** 39 <= tab["H"] * 2.0 ** tab["k"] < 2 ** 40
        assert np.array_equal(tab["fixT"][1:], np.rint(np.ldexp(t.branches[1:], tab["k"])).astype(np.int64))
        for li in range(len(tab["leaves"])):
            nodes = tab["rows"][tab["first"][li]:tab["first"][li + 1] - 1, 1]
            assert int(tab["fixT"][nodes].sum()) < 2 ** 40 + len(nodes)      # MAX_SAMPLES of them stay below 2^63
    assert tab["k"] == 40 - 17 and origin_ref.tables(_scaled(tree, 1e-6))["k"] == 40 + 23
    assert origin_ref.MAX_SAMPLES * (2 ** 40 + 4096) < 2 ** 63


@pytest.mark.parametrize("W", [1, 7, 256, 10 ** 6])
def test_window_sums_equal_reduceat(one, W):
    tree, fp, tab, (origin, age) = one
    n = fp.n_sites
    for cells in (origin, age):
        got = origin_ref.windows(cells, W)
        want = np.add.reduceat(cells.astype(np.uint64), np.arange(0, n, W), axis=1)
        assert got.dtype == np.uint64 and np.array_equal(got, want)
        cut = [0, 100, 101, 230, n]
        parts = [origin_ref.windows(cells[:, a:b], W, first_site=a, n_global=n) for a, b in zip(cut[:-1], cut[1:])]
        assert np.array_equal(sum(parts), want)


def test_file_round_trip(one, tmp_path):
    tree, fp, tab, (origin, age) = one
    W, ns = 100, 3
    ow, aw = origin_ref.windows(origin, W) * np.uint64(ns), origin_ref.windows(age, W) * np.uint64(ns)
    path = str(tmp_path / "origins.txt")
    host.write_lineage_origins(path, tree.node_names, tab["rows"], W, ns, tab["k"], ow, aw)
    text = open(path).read()
    lines = text.splitlines()
    assert lines[0] == "#samples\t%d\twindow\t%d\tscale_exp\t%d" % (ns, W, tab["k"])
    for r, (leaf, node) in enumerate(tab["rows"]):
        assert lines[1 + r] == "#row\t%d\t%s\t%s" % (r, tree.node_names[leaf], tree.node_names[node])
    # integers only below the header: every field of every window line
    body = [ln for ln in lines[1 + len(tab["rows"]):] if not ln.startswith("LEAF:")]
    assert len(body) == len(tab["leaves"]) * ow.shape[1] and all(f.isdigit() for ln in body for f in ln.split("\t"))
    first = tab["first"]
    for li, leaf in enumerate(tab["leaves"]):
        at = 1 + len(tab["rows"]) + li * (ow.shape[1] + 1)
        assert lines[at] == "LEAF:%s\t%d" % (tree.node_names[leaf], first[li + 1] - first[li])
        for w in range(ow.shape[1]):
            want = [w * W] + [int(v) for v in ow[first[li]:first[li + 1], w]] + [int(aw[li, w])]
            assert [int(v) for v in lines[at + 1 + w].split("\t")] == want
    back = host.read_lineage_origins(path)
    assert (back["samples"], back["window"], back["scale_exp"]) == (ns, W, tab["k"])
    assert back["row_leaf"] == [tree.node_names[a] for a, _ in tab["rows"]]
    assert back["row_node"] == [tree.node_names[b] for _, b in tab["rows"]]
    assert back["origin"].dtype == np.uint64 and np.array_equal(back["origin"], ow) and np.array_equal(back["age"], aw)
    # written again from what was read: the same bytes
    again = str(tmp_path / "again.txt")
    host.write_lineage_origins(again, tree.node_names, tab["rows"], back["window"], back["samples"], back["scale_exp"],
                               back["origin"], back["age"])
    assert open(again).read() == text
    with pytest.raises(RuntimeError):
        host.read_lineage_origins(str(tmp_path / "missing.txt"))
    with pytest.raises(ValueError):
        host.write_lineage_origins(path, tree.node_names, tab["rows"], W, ns, tab["k"], ow, aw[:-1])


def test_symbols_declared():
    from epievo_amd.driver import DRIVER_SYMBOLS
    from epievo_amd.sampler import ABI_SYMBOLS
    abi = ("epv_set_lineage_origins", "epv_reset_lineage_origins", "epv_accumulate_lineage_origins",
           "epv_lineage_origins_samples", "epv_lineage_origins_set_samples", "epv_lineage_origins_layout",
           "epv_lineage_origin_rows", "epv_lineage_origins_scale_exp", "epv_get_lineage_origins",
           "epv_get_lineage_origin_windows")
    drv = ("epvd_set_lineage_origins", "epvd_reset_lineage_origins", "epvd_accumulate_lineage_origins",
           "epvd_lineage_origin_rows", "epvd_lineage_origins_scale_exp", "epvd_lineage_origins_sizes", "epvd_download_lineage_origins",
           "epvd_download_lineage_origin_windows")
    header = open(os.path.join(_build.INCLUDE, "epievo_mi355x.h")).read()
    dheader = open(os.path.join(_build.INCLUDE, "epievo_mi355x_driver.h")).read()
    for s in abi:
        assert s in ABI_SYMBOLS and ("int %s(" % s) in header
    for s in drv:
        assert s in DRIVER_SYMBOLS and ("int %s(" % s) in dheader


def _run(*args):
    return subprocess.run([EXE] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_origins_option_errors_come_before_any_device(tmp_path):
    """-w without an output that takes windows, and -w 0 with -O: refused on the options alone (the input files
    do not even exist)"""
    files = [tmp_path / "p.param", tmp_path / "t.nwk", tmp_path / "in.local_paths"]
    r = _run("-o", tmp_path / "o.paths", "-w", 5, *files)
    assert r.returncode != 0 and "-O/--origins" in r.stderr, r.stderr
    r = _run("-o", tmp_path / "o.paths", "-O", tmp_path / "g.txt", "-w", 0, *files)
    assert r.returncode != 0 and "at least one site" in r.stderr, r.stderr
    assert not (tmp_path / "g.txt").exists()
    r = _run("-o", tmp_path / "o.paths", "-O", tmp_path / "g.txt", "-w", 5, *files)
    assert r.returncode != 0 and "belongs to" not in r.stderr   # -w goes with -O: what fails now is the missing input
