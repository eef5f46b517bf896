"""epievo_initialization -m / -l on the GPU: hard tokens are the plain run byte for byte, N is N in either file,
a soft run equals the same pipeline driven through DeviceSampler, and its output feeds
epievo_est_params_histories -l with the same file."""
import os
import subprocess

import numpy as np
import pytest

from common import simulate, TREE_NWK_TEXT
from epievo_amd import _build, host

pytestmark = pytest.mark.gpu
BIN = _build.BIN_DIR
N_SITES, ITERS, BATCH, SEED = 600, 3, 2, 5


def _case():
    # (data seed 33: on seed 31's 600 sites the last host M-step, the reference's optimiser without -b, needs
    # 12 s to converge, with or without the flags of this file; the tests here are not about that)
    model, tree, fp = simulate("tree", N_SITES, seed=33)
    B, n = tree.n_nodes - 1, fp.n_sites
    es = fp.init.reshape(B, n) ^ (fp.counts().reshape(B, n) & 1).astype(np.uint8)
    leaves = [i for i in range(tree.n_nodes) if tree.subtree_sizes[i] == 1]
    return tree, es, leaves


def _write(path, tree, leaves, tokens):
    """tokens[leaf index][site] -> a states-shaped file"""
    with open(path, "w") as f:
        f.write("#" + "\t".join(tree.node_names[i] for i in leaves) + "\n")
        for s in range(len(tokens[0])):
            f.write("%d\t%s\n" % (s, "\t".join(t[s] for t in tokens)))


def _run(d, tag, args, optimize, expect=0):
    cmd = [os.path.join(BIN, "epievo_initialization"), "-i", str(ITERS), "-B", str(BATCH), "-s", str(SEED), "-v",
           "-p", "%s/%s.param" % (d, tag), "-o", "%s/%s.paths" % (d, tag), "-t", "%s/%s.nwk" % (d, tag)]
    if optimize:
        cmd.append("-b")
    r = subprocess.run(cmd + args, capture_output=True, text=True)
    assert r.returncode == expect, r.stderr
    if expect:
        return r.stderr
    out = [open("%s/%s.param" % (d, tag), "rb").read(), open("%s/%s.paths" % (d, tag), "rb").read()]
    if optimize:
        out.append(open("%s/%s.nwk" % (d, tag), "rb").read())
    return out, r.stderr


def _tokens(es, leaves, holes=None, soft=None):
    """the data as tokens; holes / soft: {(leaf index, site): token}"""
    t = [[str(int(x)) for x in es[i - 1]] for i in leaves]
    for cells in (holes or {}), (soft or {}):
        for (k, s), tok in cells.items():
            t[k][s] = tok
    return t


def _cells(n, leaves, every=7):
    return [(k, s) for k in range(len(leaves)) for s in range(k, n, every)]


@pytest.mark.parametrize("optimize", [False, True])
def test_hard_tokens_are_the_plain_run_and_n_is_n(tmp_path, optimize):
    tree, es, leaves = _case()
    d = str(tmp_path)
    open(d + "/t.nwk", "w").write(TREE_NWK_TEXT)
    _write(d + "/obs.states", tree, leaves, _tokens(es, leaves))
    plain, _ = _run(d, "plain", [d + "/t.nwk", d + "/obs.states"], optimize)
    hard, err = _run(d, "hard", ["-l", d + "/obs.states", d + "/t.nwk"], optimize)
    assert hard == plain
    assert "[LEAF CELLS WITH EVIDENCE: 0 of %d]" % (len(leaves) * N_SITES) in err
    holes = {c: "N" for c in _cells(N_SITES, leaves)}
    _write(d + "/holes.states", tree, leaves, _tokens(es, leaves, holes))
    lp, err_l = _run(d, "lp", ["-l", d + "/holes.states", d + "/t.nwk"], optimize)
    ms, err_m = _run(d, "ms", ["-m", d + "/holes.states", d + "/t.nwk"], optimize)
    assert lp == ms and lp != plain
    assert "[LEAF CELLS WITH EVIDENCE: %d of %d]" % (len(holes), len(leaves) * N_SITES) in err_l
    assert "[UNOBSERVED LEAF CELLS: %d of %d]" % (len(holes), len(leaves) * N_SITES) in err_m
    # a states file with N given positionally still fails as it does today
    err = _run(d, "bad", [d + "/t.nwk", d + "/holes.states"], optimize, expect=1)
    assert "inconsistent number of states" in err


@pytest.mark.parametrize("optimize", [False, True])
def test_soft_run_matches_the_python_pipeline_and_feeds_the_em_driver(tmp_path, optimize):
    from epievo_amd.sampler import DeviceSampler
    tree, es, leaves = _case()
    d = str(tmp_path)
    open(d + "/t.nwk", "w").write(TREE_NWK_TEXT)
    values = ["0.8", "0.02", "N", "0.35", "0.5", "0.999", "1e-3"]
    soft = {c: values[i % len(values)] for i, c in enumerate(_cells(N_SITES, leaves, every=5))}
    tok = _tokens(es, leaves, soft=soft)
    _write(d + "/soft.probs", tree, leaves, tok)
    out, err = _run(d, "soft", ["-l", d + "/soft.probs", d + "/t.nwk"], optimize)
    assert "[LEAF CELLS WITH EVIDENCE: %d of %d]" % (len(soft), len(leaves) * N_SITES) in err

    # the recipe of test_cli.py::test_initialization_matches_oracle_pipeline with the device in the oracle's place
    N, n, B = tree.n_nodes, N_SITES, tree.n_nodes - 1
    r = np.array([[0.5 if t in ("N", "n") else float(t) for t in row] for row in tok], np.float32)
    st = np.zeros((N, n), np.uint8)
    st[leaves] = r > 0.5
    p0 = host.initialize_paths_heuristic(SEED, tree, st)
    table = np.full((B, n), np.nan, np.float32)
    table[[i - 1 for i in leaves]] = np.where((r == 0) | (r == 1), np.float32(np.nan), r)
    dev = DeviceSampler(0)
    dev.auto_grow = True
    dev.set_tree(tree)
    dev.set_model(host.Model(np.ones(8), np.full(4, 0.5), np.zeros(4)))
    dev.upload_paths(p0, 32)
    dev.set_leaf_evidence(table)
    rates, br = np.zeros(2), tree.branches.copy()
    J, D = dev.indep_suffstats()
    for it in range(ITERS):
        rates, br_new = host.indep_m_step(rates, br, J, D, optimize_branches=optimize)
        if optimize:
            dev.scale_jump_times(br_new)
            br = br_new
        J, D = dev.indep_expectation(rates)
    Jt, Dt = np.zeros(B * 8), np.zeros(B * 8)
    for i in range(BATCH):
        dev.indep_update_paths(rates, SEED, 0xF0000000 + i)
        J1, D1 = dev.suffstats()
        Jt += J1
        Dt += D1
    Jt /= BATCH
    Dt /= BATCH
    m2, br2, llh, text = host.m_step(host.model_from_indep_rates(rates), br, Jt, Dt, optimize_branches=optimize)
    dev.scale_jump_times(br2)
    assert out[0].decode() == text + "\n"
    host.write_paths(d + "/exp.paths", tree.node_names, br2, dev.paths())
    assert out[1] == open(d + "/exp.paths", "rb").read()

    # hard leaf cells in the output equal the input; some soft cell left its start state
    got, names, tt = host.read_paths(d + "/soft.paths")
    es2 = got.init.reshape(B, n) ^ (got.counts().reshape(B, n) & 1).astype(np.uint8)
    lv = [i - 1 for i in leaves]
    hard = (r == 0) | (r == 1)
    assert np.array_equal(es2[lv][hard], es[lv][hard])
    assert not np.array_equal(es2[lv], st[leaves])

    # the same FILE passes the agreement check of the E-step program, which runs one iteration
    open(d + "/p.param", "w").write(out[0].decode())
    tree_in = d + "/soft.nwk" if optimize else d + "/t.nwk"
    e = subprocess.run([os.path.join(BIN, "epievo_est_params_histories"), "-i", "1", "-B", "2", "-L", "1", "-s", "7", "-v",
                        "-l", d + "/soft.probs", "-o", d + "/em.paths", "-p", d + "/em.param", d + "/p.param", tree_in,
                        d + "/soft.paths"], capture_output=True, text=True)
    assert e.returncode == 0, e.stderr
    assert "[LEAF CELLS WITH EVIDENCE: %d of %d]" % (len(soft), len(leaves) * N_SITES) in e.stderr
