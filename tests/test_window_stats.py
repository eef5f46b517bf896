"""Regional sufficient statistics, the parts that need no GPU: the yardstick (the oracle's integer rows cut at
the windows) adds up to the whole genome for every window size and agrees per site with the plain-Python walk
of dense_cases.yardstick; the regional rate factor is the maximiser of the M-step's log-likelihood along
rho * rates; the file of epievo_est_histories -r round-trips through the epv_io writer and reader."""
import decimal
import math

import numpy as np
import pytest

import dense_cases as dc
import orc
import wstat_ref
from common import simulate
from epievo_amd import host

SHAPES = [("tree", 700), ("bal16", 300)]
_cache = {}


def _oracle(cfg, n):
    """a reset rung-B oracle after two sweeps (so that the paths are the sampler's, not the input's), shared and
    only read"""
    if (cfg, n) not in _cache:
        model, tree, fp = simulate(cfg, n, seed=6)
        o = orc.Oracle(tree, model, fp, "B", cap=int(max(16, 2 * fp.counts().max() + 8)), seed=77)
        o.reset()
        o.sweep(0)
        o.sweep(1)
        _cache[(cfg, n)] = (model, tree, o)
    return _cache[(cfg, n)]


@pytest.mark.parametrize("cfg,n", SHAPES)
def test_rows_add_up_to_the_genome(cfg, n):
    model, tree, o = _oracle(cfg, n)
    whole = wstat_ref.total(o, n)
    assert whole[:, :8].any() and whole[:, 8:].any()
    for W in (1, 3, 64, 100, 256, n + 5):
        r = wstat_ref.rows(o, W, n)
        assert r.shape == (wstat_ref.n_windows(n, W), tree.n_nodes - 1, 16)
        assert np.array_equal(r.sum(axis=0), whole), W
        assert (r >= 0).all()
    assert wstat_ref.rows(o, n + 5, n).shape[0] == 1                      # clamped: one window
    # the genome's two end sites centre no triple: at W = 1 their windows are empty
    r1 = wstat_ref.rows(o, 1, n)
    assert not r1[0].any() and not r1[n - 1].any() and r1[1, :, 8:].any()
    # total time per interior site and branch, to the quantum: sum_ctx D = T_b
    sc = wstat_ref.scales(o)
    per_site = r1[1:n - 1, :, 8:].sum(axis=2) / sc[None, 1:]
    assert np.allclose(per_site, np.asarray(tree.branches)[None, 1:], rtol=1e-9, atol=0)
    assert wstat_ref.not_vacuous(wstat_ref.rows(o, 3, n))


@pytest.mark.parametrize("cfg,n", SHAPES)
def test_rows_at_one_site_match_the_walk(cfg, n):
    model, tree, o = _oracle(cfg, n)
    fp, sc = o.paths(), wstat_ref.scales(o)
    r1 = wstat_ref.rows(o, 1, n)
    for s in range(1, n - 1):
        J, D, n_int = dc.yardstick(fp, tree.branches, first=s, last=s)
        assert np.array_equal(r1[s, :, :8], J), s
        got = r1[s, :, 8:].astype(np.float64) / sc[1:, None]
        assert (np.abs(got - D) <= dc.dwell_bound(n_int, D, sc)).all(), s


def _ll_exact(J, D, rates, rho):
    """log_likelihood(sum_b J, sum_b D, rho * rates) in 60-digit decimal arithmetic from the doubles' exact values.
    A maximiser found by comparing function values is only as sharp as the square root of the arithmetic's
    precision (the function is flat to second order there): fp64 would give 1e-8, short of the 1e-9 asked."""
    Dm = decimal.Decimal
    Jc, Dc = J.sum(axis=0), D.sum(axis=0)
    tot = Dm(0)
    for c in range(8):
        r = rho * Dm(float(rates[c]))
        tot += Dm(float(Jc[c])) * r.ln() - Dm(float(Dc[c])) * r
    return tot


def _argmax_by_bracketing(J, D, rates):
    """ternary search on (0, hi]: the function is strictly concave in rho when sum J > 0"""
    Dm = decimal.Decimal
    lo, hi = Dm("1e-6"), Dm("1e6")
    f = lambda x: _ll_exact(J, D, rates, x)    # noqa: E731
    for _ in range(400):
        a, b = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        if f(a) < f(b):
            lo = a
        else:
            hi = b
        if (hi - lo) / hi < Dm("1e-13"):
            break
    return float((lo + hi) / 2)


def test_rate_factor_is_the_argmax():
    model, tree, o = _oracle("tree", 700)
    n, W = 700, 100
    counts = wstat_ref.rows(o, W, n)
    J, D = wstat_ref.to_stats(counts, wstat_ref.scales(o), 1)
    rho = host.regional_rate_factors(J, D, model.rates)
    assert rho.shape == (7,)
    seen = 0
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        for w in range(len(rho)):
            if J[w].sum() == 0:
                assert rho[w] == 0.0          # no jump: the likelihood falls with rho, the maximum is at 0
                continue
            seen += 1
            want = _argmax_by_bracketing(J[w], D[w], model.rates)
            assert abs(rho[w] - want) <= 1e-9 * want, (w, rho[w], want)
            # and the library's own log-likelihood is no larger a little to either side
            here = host.collapsed_log_likelihood(J[w], D[w], rho[w] * model.rates)
            for f in (1.0 - 1e-5, 1.0 + 1e-5):
                assert host.collapsed_log_likelihood(J[w], D[w], f * rho[w] * model.rates) < here
    assert seen >= 2
    # the closed form
    want = J.sum(axis=(1, 2)) / (D * model.rates[None, None, :]).sum(axis=(1, 2))
    assert np.allclose(rho, want, rtol=1e-14, atol=0)
    # doubling every rate halves the factor: it is relative to the rates it is given
    assert np.allclose(host.regional_rate_factors(J, D, 2.0 * model.rates), rho / 2.0, rtol=1e-14, atol=0)


def test_rate_factor_of_an_empty_window_is_nan():
    model, tree, o = _oracle("tree", 700)
    counts = wstat_ref.rows(o, 1, 700)[:3]            # window 0 = site 0, which centres no triple
    J, D = wstat_ref.to_stats(counts, wstat_ref.scales(o), 1)
    rho = host.regional_rate_factors(J, D, model.rates)
    assert math.isnan(rho[0]) and not math.isnan(rho[1]) and not math.isnan(rho[2])
    with pytest.raises(ValueError):
        host.regional_rate_factors(J[0], D[0], model.rates)


@pytest.mark.parametrize("cfg,n,W", [("tree", 700, 100), ("bal16", 300, 1)])
def test_file_round_trip(tmp_path, cfg, n, W):
    model, tree, o = _oracle(cfg, n)
    samples = 3
    counts = wstat_ref.rows(o, W, n) * samples        # as if three equal samples had been added
    sc = wstat_ref.scales(o)
    k = np.concatenate([[0], np.frexp(sc[1:])[1] - 1])                    # the oracle's k_b
    assert np.array_equal(np.ldexp(1.0, k[1:]), sc[1:])
    J, D = wstat_ref.to_stats(counts, sc, samples)
    f1, f2 = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    host.write_window_stats(f1, tree.node_names, tree.branches, k, W, samples, counts, J, D, model.rates)
    r = host.read_window_stats(f1)
    assert r["samples"] == samples and r["window"] == W
    assert r["node_names"] == list(tree.node_names[1:])
    assert np.array_equal(r["branches"], tree.branches[1:]) and np.array_equal(r["scale_exp"], k[1:])
    assert np.array_equal(r["counts"], counts)
    assert np.array_equal(r["all_J"], counts[:, :, :8].sum(axis=1))
    assert np.allclose(r["all_D"], D.sum(axis=1), rtol=1e-15, atol=0)
    rho = host.regional_rate_factors(J, D, model.rates)
    assert np.array_equal(np.isnan(r["factor"]), np.isnan(rho))
    ok = ~np.isnan(rho)
    assert np.array_equal(r["factor"][ok], rho[ok])                       # %.17g: the doubles themselves
    if W == 1:
        assert np.isnan(r["factor"][0]) and np.isnan(r["factor"][-1])
    # what was read writes the same bytes
    J2, D2 = wstat_ref.to_stats(r["counts"], np.concatenate([[1.0], np.ldexp(1.0, r["scale_exp"])]), r["samples"])
    host.write_window_stats(f2, ["root"] + r["node_names"], np.concatenate([[0.0], r["branches"]]),
                            np.concatenate([[0], r["scale_exp"]]), r["window"], r["samples"], r["counts"], J2, D2,
                            model.rates)
    assert open(f1, "rb").read() == open(f2, "rb").read()
    head = open(f1).readline().rstrip("\n").split("\t")
    assert head == ["#samples", str(samples), "window", str(W)]
    with open(str(tmp_path / "bad.txt"), "w") as fh:
        fh.write("#samples\t1\twindow\t1\nNODE:x\t0.5\t40\n")
    with pytest.raises(RuntimeError):
        host.read_window_stats(str(tmp_path / "bad.txt"))


def test_file_round_trip_keeps_long_node_names(tmp_path):
    """names of any length come back whole and aligned with their nodes"""
    model, tree, o = _oracle("bal16", 300)
    names = [("node%d_" % i) + "x" * (40 + 7 * i) for i in range(tree.n_nodes)]       # 40 .. 250 characters
    assert np.mean([len(s) for s in names[1:]]) > 63
    sc = wstat_ref.scales(o)
    k = np.concatenate([[0], np.frexp(sc[1:])[1] - 1])
    counts = wstat_ref.rows(o, 100, 300)
    J, D = wstat_ref.to_stats(counts, sc, 1)
    f = str(tmp_path / "long.txt")
    host.write_window_stats(f, names, tree.branches, k, 100, 1, counts, J, D, model.rates)
    r = host.read_window_stats(f)
    assert r["node_names"] == names[1:] and np.array_equal(r["counts"], counts)
