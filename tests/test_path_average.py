"""average_paths (host CLI, the reference's program of the same name): its output equals, byte for
byte, a numpy restatement of average_paths.cpp:31-63 with the per-branch fix (tests/pavg_ref.py);
grid-edge cases and input errors.  The device-side averaging is in test_path_average_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import pavg_ref
from common import simulate
from epievo_amd import _build, host

AVG = os.path.join(_build.BIN_DIR, "average_paths")


def _run(*args):
    return subprocess.run([AVG] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _write_samples(d, tree, fps, names=None):
    names = names or tree.node_names
    for k, fp in enumerate(fps):
        host.write_paths(os.path.join(str(d), "s%02d.local_paths" % k), names, tree.branches, fp)


def _expected(tree, fps, P):
    cnt = sum(pavg_ref.counts(fp, tree.branches, P) for fp in fps)
    return pavg_ref.format_average(tree.node_names, tree.branches, cnt, len(fps))


@pytest.mark.parametrize("cfg,n,P", [("tree", 300, 100), ("tree", 257, 7), ("bal16", 120, 2), ("pair", 200, 50)])
def test_average_paths_matches_restatement(tmp_path, cfg, n, P):
    fps = []
    for seed in (3, 4, 5):
        model, tree, fp = simulate(cfg, n, seed=seed)
        fps.append(fp)
    _write_samples(tmp_path, tree, fps)
    (tmp_path / "notes.txt").write_text("not a paths file\n")      # ignored: wrong suffix
    out = tmp_path / "avg.txt"
    r = _run("-n", P, "-o", out, tmp_path)
    assert r.returncode == 0, r.stderr
    assert out.read_text() == _expected(tree, fps, P)


def test_average_paths_default_points_and_single_file(tmp_path):
    model, tree, fp = simulate("tree", 64, seed=9)
    _write_samples(tmp_path, tree, [fp])
    out = tmp_path / "avg.txt"
    assert _run("-o", out, tmp_path).returncode == 0
    text = out.read_text()
    assert text == _expected(tree, [fp], 100)
    assert len(text.splitlines()[1 + 1].split("\t")) == 100


def _edge_case_grid():
    """a branch length and point count whose repeated-addition grid ends below the branch length"""
    for P in range(3, 40):
        for T in (0.1, 0.3, 0.7, 0.9, 1.1, 0.03):
            t = pavg_ref.grid(T, P)
            if t[-1] < T and np.nextafter(t[-1], np.inf) < T:
                return T, P, t
    raise AssertionError("no such grid")


def test_average_paths_grid_edges(tmp_path):
    T, P, t = _edge_case_grid()
    tree = host.Tree.single_branch(T)
    # site 0: a jump exactly on t_2 (lower_bound: not before it) and one in (t_{P-1}, T);
    # site 1: two jumps inside one cell; site 2: none; site 3: a jump just below t_1
    jumps = [[t[2], np.nextafter(t[-1], np.inf)], [0.5 * (t[1] + t[2]), np.nextafter(t[2], 0.0)], [],
             [np.nextafter(t[1], 0.0)]]
    init = np.array([0, 1, 1, 0], np.uint8)
    off = np.zeros(5, np.uint64)
    off[1:] = np.cumsum([len(j) for j in jumps])
    fp = host.FlatPaths(4, 2, init, off, np.array([x for j in jumps for x in j]))
    _write_samples(tmp_path, tree, [fp])
    cnt = pavg_ref.counts(fp, tree.branches, P)
    assert cnt[0, 0, 2] == 0 and cnt[0, 0, 3] == 1 and cnt[0, 0, -1] == 1    # the jump beyond t_{P-1} counts nowhere
    assert list(cnt[0, 1]) == [1] * P                                        # two jumps in one cell cancel
    assert cnt[0, 3, 0] == 0 and cnt[0, 3, 1] == 1
    out = tmp_path / "avg.txt"
    r = _run("-n", P, "-o", out, tmp_path)
    assert r.returncode == 0, r.stderr
    assert out.read_text() == pavg_ref.format_average(tree.node_names, tree.branches, cnt, 1)


def test_average_paths_per_branch_fix(tmp_path):
    """node b's own path at every point: the reference's average_paths reads node 1's (:39)"""
    model, tree, fp = simulate("tree", 50, seed=2)
    _write_samples(tmp_path, tree, [fp])
    out = tmp_path / "avg.txt"
    assert _run("-n", 5, "-o", out, tmp_path).returncode == 0
    blocks = out.read_text().split("NODE:")[2:]
    rows = [np.array([[float(v) for v in ln.split("\t")] for ln in blk.splitlines()[1:]]) for blk in blocks]
    B, n = tree.n_nodes - 1, 50
    init = fp.init.reshape(B, n)
    for b in range(B):
        assert np.array_equal(rows[b][:, 0], init[b])
    ends = [np.array([np.searchsorted(fp.jumps[int(fp.offsets[b * n + s]):int(fp.offsets[b * n + s + 1])],
                                      pavg_ref.grid(tree.branches[b + 1], 5)[2]) & 1 ^ init[b, s] for s in range(n)])
            for b in range(B)]
    for b in range(B):
        assert np.array_equal(rows[b][:, 2], ends[b])


def test_average_paths_errors(tmp_path):
    out = tmp_path / "avg.txt"
    empty = tmp_path / "empty"
    empty.mkdir()
    r = _run("-o", out, empty)
    assert r.returncode != 0 and "no *local_paths files" in r.stderr
    r = _run("-o", out, tmp_path / "missing")
    assert r.returncode != 0 and "cannot read directory" in r.stderr

    model, tree, fp = simulate("tree", 40, seed=1)
    ok = tmp_path / "ok"
    ok.mkdir()
    _write_samples(ok, tree, [fp])
    r = _run("-n", 1, "-o", out, ok)
    assert r.returncode != 0 and "at least 2" in r.stderr

    sites = tmp_path / "sites"
    sites.mkdir()
    _write_samples(sites, tree, [fp, simulate("tree", 41, seed=1)[2]])
    r = _run("-o", out, sites)
    assert r.returncode != 0 and "41 sites" in r.stderr

    nodes = tmp_path / "nodes"
    nodes.mkdir()
    _write_samples(nodes, tree, [fp])
    m2, t2, fp2 = simulate("pair", 40, seed=1)
    host.write_paths(str(nodes / "z.local_paths"), t2.node_names, t2.branches, fp2)
    r = _run("-o", out, nodes)
    assert r.returncode != 0 and "nodes" in r.stderr

    names = tmp_path / "names"
    names.mkdir()
    _write_samples(names, tree, [fp])
    host.write_paths(str(names / "z.local_paths"), ["X%d" % i for i in range(tree.n_nodes)], tree.branches, fp)
    r = _run("-o", out, names)
    assert r.returncode != 0 and "node names differ" in r.stderr


def test_path_average_symbols_declared():
    from epievo_amd.sampler import ABI_SYMBOLS
    for s in ("epv_set_path_average", "epv_reset_path_average", "epv_accumulate_path_average",
              "epv_path_average_samples", "epv_get_path_average"):
        assert s in ABI_SYMBOLS
