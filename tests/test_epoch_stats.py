"""Epoch statistics, the parts that need no GPU: the yardstick (tests/epoch_ref.py, a plain-Python walk of the
oracle's paths) adds up over the epochs to the oracle's whole-genome integers for every P; the library closes a
difference form built by a second Python routine to the direct overlap walk; raw parts of a genome cut at random
points add up to the raw part of the whole; the edges tile the branch, also where bins have no width; the rate
factor per branch and epoch is the maximiser of the likelihood along rho * rates; the file of
epievo_est_histories -E round-trips through the epv_io writer and reader."""
import decimal
import math
import random

import numpy as np
import pytest

import epoch_ref
import orc
import wstat_ref
from common import simulate
from epievo_amd import host
from epievo_amd.sampler import EPOCH_MAX_P
from test_window_stats import _argmax_by_bracketing

PS = (1, 2, 7, 64, EPOCH_MAX_P)
SHAPES = [("tree", 300), ("bal16", 120)]
_cache = {}


def _oracle(cfg, n):
    """a reset rung-B oracle after two sweeps (the sampler's paths, not the input's), with the intervals of its
    triples; shared and only read"""
    if (cfg, n) not in _cache:
        model, tree, fp = simulate(cfg, n, seed=6)
        o = orc.Oracle(tree, model, fp, "B", cap=int(max(16, 2 * fp.counts().max() + 8)), seed=77)
        o.reset()
        o.sweep(0)
        o.sweep(1)
        sc = wstat_ref.scales(o)
        _cache[(cfg, n)] = (model, tree, o, sc, epoch_ref.intervals(o.paths(), tree.branches, sc),
                            epoch_ref.fix_T(tree.branches, sc))
    return _cache[(cfg, n)]


def test_max_p_is_the_headers():
    text = open(host._build.INCLUDE + "/epievo_mi355x.h").read()
    assert "#define EPV_EPOCH_MAX_P %du" % EPOCH_MAX_P in text


@pytest.mark.parametrize("cfg,n", SHAPES)
def test_epochs_add_up_to_the_genome(cfg, n):
    """identity A of the yardstick: summed over the epochs it gives, per branch and context, the oracle's integers"""
    model, tree, o, sc, ivs, fixT = _oracle(cfg, n)
    whole = wstat_ref.total(o, n)
    assert whole[:, :8].any()
    for P in PS:
        J, D, info = epoch_ref.walk(ivs, fixT, P)
        assert np.array_equal(J.sum(axis=1).astype(np.int64), whole[:, :8]), P
        assert np.array_equal(D.sum(axis=1).astype(np.int64), whole[:, 8:]), P
        if P >= 3:       # the case is a real one: jumps in two epochs of a branch, an interval over three, a clock off T
            assert info["jump_epochs"] >= 2 and info["span"] >= 3 and info["off_T"] >= 1
        if P == 1:       # identity C
            assert np.array_equal(J[:, 0].astype(np.int64), whole[:, :8])
            assert np.array_equal(D[:, 0].astype(np.int64), whole[:, 8:])


@pytest.mark.parametrize("cfg,n", SHAPES)
def test_library_closes_the_difference_form(cfg, n):
    model, tree, o, sc, ivs, fixT = _oracle(cfg, n)
    for P in PS:
        J, D, _ = epoch_ref.walk(ivs, fixT, P)
        raw = epoch_ref.to_words(epoch_ref.raw_part(ivs, fixT, P))
        Jc, Dc = host.epoch_close(raw, fixT)
        assert Jc.dtype == np.int64 and np.array_equal(Jc, J.astype(np.int64)), P
        assert all(int(a) == int(b) for a, b in zip(Dc.reshape(-1), D.reshape(-1))), P
        # per sample: the doubles of the integers
        ns, Jf, Df = host.epoch_finish(raw, fixT, np.frexp(sc[1:])[1] - 1, 3)
        Jw, Dw = epoch_ref.to_stats(J, D, sc, 3)
        assert ns == 3 and np.array_equal(Jf, Jw) and np.array_equal(Df, Dw)
    with pytest.raises(RuntimeError):
        host.epoch_finish(raw, fixT, np.frexp(sc[1:])[1] - 1, 0)
    # a raw part no walk can have made is refused: cover that never ends
    bad = raw.copy()
    bad[0, 0, 24] += np.uint64(1)
    with pytest.raises(RuntimeError):
        host.epoch_close(bad, fixT)
    with pytest.raises(ValueError):
        host.epoch_close(raw[0], fixT)


def test_close_takes_sums_beyond_64_bits():
    """many samples: part sums pass 2^64 (the hi words hold them), the closed D is a 128-bit integer"""
    fixT, P = [(1 << 50) - 3], 4
    E = epoch_ref.edges(fixT[0], P)
    k = (1 << 31) * 6000                       # intervals [0, fixT), as samples x sites of no-jump triples
    raw = np.zeros((1, P, 32), object)
    raw[0, 0, 8] = k * E[1]
    raw[0, P - 1, 8] = k * (fixT[0] - E[P - 1])
    raw[0, 1, 24] = k
    raw[0, P - 1, 24] = -k
    J, D = host.epoch_close(epoch_ref.to_words(raw), fixT)
    want = [k * (E[1] - E[0]), k * (E[2] - E[1]), k * (E[3] - E[2]), k * (fixT[0] - E[3])]
    assert [int(D[0, p, 0]) for p in range(P)] == want and max(want) > 1 << 64
    assert sum(want) == k * fixT[0] and not J.any()


@pytest.mark.parametrize("cfg,n", SHAPES)
def test_raw_parts_of_a_cut_genome_add_up(cfg, n):
    model, tree, o, sc, ivs, fixT = _oracle(cfg, n)
    fp = o.paths()
    rng = random.Random(5)
    for P in (2, 7, EPOCH_MAX_P):
        whole = epoch_ref.to_words(epoch_ref.raw_part(ivs, fixT, P))
        cuts = [1] + sorted(rng.sample(range(2, n - 1), 3)) + [n - 1]
        pieces = [epoch_ref.to_words(epoch_ref.raw_part(
            epoch_ref.intervals(fp, tree.branches, sc, first=a, last=b - 1), fixT, P)) for a, b in zip(cuts[:-1], cuts[1:])]
        # another split of part into lo and hi, as another launch shape makes it
        x = np.minimum(pieces[1][..., 16:24], np.uint64(5))
        assert x.any()
        pieces[1][..., 16:24] -= x
        pieces[1][..., 8:16] += x << np.uint64(32)
        tot = host.epoch_raw_add(pieces)
        for a, b in zip(epoch_ref.parts_of(tot), epoch_ref.parts_of(whole)):
            assert (a == b).all(), P
        assert (tot[..., 8:16] < np.uint64(1 << 32)).all()
        Jc, Dc = host.epoch_close(tot, fixT)
        J, D, _ = epoch_ref.walk(ivs, fixT, P)
        assert np.array_equal(Jc, J.astype(np.int64)) and (Dc == D).all()


def test_edges_tile_the_branch():
    for fixT in (0, 1, 5, 255, 256, 1000, (1 << 50) - 1):
        for P in PS:
            E = host.epoch_edges(fixT, P)
            assert E.dtype == np.uint64 and [int(e) for e in E] == epoch_ref.edges(fixT, P)
            assert E[0] == 0 and (np.diff(E.astype(np.int64)) >= 0).all() and int(E[-1]) <= fixT
            widths = [int(b) - int(a) for a, b in zip(E, list(E[1:]) + [fixT])]
            assert sum(widths) == fixT and max(widths) - min(widths) <= 1
            if fixT < P:
                assert widths.count(0) == P - fixT            # bins without width
            # every clock value lies in exactly one bin, and bin() finds it; the last bin is open-ended
            for c in sorted(set([0, 1, fixT // 2, max(fixT - 1, 0), fixT, fixT + 3072])):
                p = epoch_ref.bin_of([int(e) for e in E], c)
                assert 0 <= p <= P - 1 and E[p] <= c and (p == P - 1 or c < E[p + 1])
    # a walk on a branch shorter than P quanta: zero-width bins take nothing, the sums hold
    ivs = [([(3, 0, 2, True), (1, 2, 5, False)], [0, 2, 0, 0, 0, 0, 0, 0], 0)]
    J, D, _ = epoch_ref.walk(ivs, [5], 7)
    raw = epoch_ref.to_words(epoch_ref.raw_part(ivs, [5], 7))
    Jc, Dc = host.epoch_close(raw, [5])
    assert np.array_equal(Jc, J.astype(np.int64)) and (Dc == D).all()
    assert int(D[0, :, 1].sum()) == 2 * 5 + 3 and int(D[0, :, 3].sum()) == 2 and int(J.sum()) == 1
    widths = np.diff(epoch_ref.edges(5, 7) + [5])
    assert all(not D[0, p].any() for p in range(6) if widths[p] == 0)


def test_rate_factor_is_the_argmax():
    model, tree, o, sc, ivs, fixT = _oracle("tree", 300)
    P = 7
    J, D, _ = epoch_ref.walk(ivs, fixT, P)
    Jf, Df = epoch_ref.to_stats(J, D, sc, 1)
    rho = host.epoch_rate_factors(Jf, Df, model.rates)
    assert rho.shape == (tree.n_nodes - 1, P)
    seen = 0
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        for b in range(rho.shape[0]):
            for p in range(P):
                if Jf[b, p].sum() == 0:
                    assert rho[b, p] == 0.0
                    continue
                seen += 1
                want = _argmax_by_bracketing(Jf[b, p][None], Df[b, p][None], model.rates)
                assert abs(rho[b, p] - want) <= 1e-9 * want, (b, p, rho[b, p], want)
    assert seen >= 2
    want = Jf.sum(axis=2) / (Df * model.rates[None, None, :]).sum(axis=2)
    assert np.allclose(rho, want, rtol=1e-14, atol=0)
    assert math.isnan(host.epoch_rate_factors(np.zeros((1, 2, 8)), np.zeros((1, 2, 8)), model.rates)[0, 0])
    with pytest.raises(ValueError):
        host.epoch_rate_factors(Jf[0], Df[0], model.rates)


@pytest.mark.parametrize("cfg,n,P", [("tree", 300, 7), ("bal16", 120, 64)])
def test_file_round_trip(tmp_path, cfg, n, P):
    model, tree, o, sc, ivs, fixT = _oracle(cfg, n)
    samples = 3
    J, D, _ = epoch_ref.walk(ivs, fixT, P)
    J, D = J.astype(np.int64) * samples, D * (samples << 40)           # D beyond 64 bits
    assert max(int(v) for v in D.reshape(-1)) > 1 << 64
    k = np.concatenate([[0], np.frexp(sc[1:])[1] - 1])
    assert np.array_equal(np.ldexp(1.0, k[1:]), sc[1:])
    f1, f2 = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    host.write_epoch_stats(f1, tree.node_names, tree.branches, k, [0] + fixT, samples, J, D, model.rates)
    r = host.read_epoch_stats(f1)
    assert r["samples"] == samples and r["epochs"] == P
    assert r["node_names"] == list(tree.node_names[1:])
    assert np.array_equal(r["branches"], tree.branches[1:]) and np.array_equal(r["scale_exp"], k[1:])
    assert np.array_equal(r["J"], J) and (r["D"] == D).all()
    for b in range(tree.n_nodes - 1):
        assert np.array_equal(r["start"][b], np.array(epoch_ref.edges(fixT[b], P), np.float64) / float(fixT[b]))
    Df = np.array([float(int(v)) for v in D.reshape(-1)]).reshape(D.shape) / sc[1:, None, None]
    rho = host.epoch_rate_factors(J.astype(np.float64), Df, model.rates)
    ok = ~np.isnan(rho)
    assert np.array_equal(np.isnan(r["factor"]), np.isnan(rho)) and np.array_equal(r["factor"][ok], rho[ok])
    host.write_epoch_stats(f2, ["root"] + r["node_names"], np.concatenate([[0.0], r["branches"]]),
                           np.concatenate([[0], r["scale_exp"]]), [0] + fixT, r["samples"], r["J"], r["D"], model.rates)
    assert open(f1, "rb").read() == open(f2, "rb").read()
    lines = open(f1).read().split("\n")
    assert lines[0].split("\t") == ["#samples", str(samples), "epochs", str(P)]
    assert lines[1].split("\t") == ["NODE:" + tree.node_names[1], "%.17g" % tree.branches[1], str(k[1])]
    assert len(lines[2].split("\t")) == 18 and len(lines) == 1 + (tree.n_nodes - 1) * (P + 1) + 1
    with open(str(tmp_path / "bad.txt"), "w") as fh:
        fh.write("#samples\t1\tepochs\t2\nNODE:x\t0.5\t40\n0\t" + "\t".join(["0"] * 17) + "\n")
    with pytest.raises(RuntimeError):
        host.read_epoch_stats(str(tmp_path / "bad.txt"))
