"""Randomised parity: random tree topologies (2..12 leaves, multifurcations, branch lengths
over two orders of magnitude), random models and seeds -- the HIP path must reproduce the
parallel rung of the oracle bit for bit on every one (paths, accept counts, cached
log-likelihoods, J, D).

Cases 12 .. 23 widen the model box (stationary 0.02 .. 0.999, baseline -6 .. 2, branches over four orders of
magnitude).  A model from that box can make the rejection search for a kept segment arbitrarily long
(model_cases.py), so each of them must meet the work bound of model_cases.py on the oracle before its GPU twin
creates a device context."""
import numpy as np
import pytest

import orc
import refvec
from common import _tmp
from epievo_amd import host



def _random_newick(rng, n_leaves):
    """random rooted tree as Newick; inner nodes get 2 or 3 children"""
    names = iter("n%d" % i for i in range(1000))
    nodes = ["%s:%.4g" % (next(names), 10 ** rng.uniform(-2.0, 0.0)) for _ in range(n_leaves)]
    while len(nodes) > 1:
        k = min(len(nodes), int(rng.choice([2, 2, 3])))
        idx = sorted(rng.choice(len(nodes), size=k, replace=False), reverse=True)
        kids = [nodes.pop(i) for i in idx]
        if nodes:
            nodes.append("(%s)%s:%.4g" % (",".join(kids), next(names), 10 ** rng.uniform(-2.0, 0.0)))
        else:
            nodes.append("(%s)%s:0.0" % (",".join(kids), next(names)))
    return nodes[0] + ";\n"


def _random_case(case):
    rng = np.random.RandomState(1000 + case)
    n_leaves = int(rng.randint(2, 13))
    tree = host.Tree.read(_tmp("fuzz%d.nwk" % case, _random_newick(rng, n_leaves)))
    st0, st1 = rng.uniform(0.6, 0.95, size=2)
    b0, b1 = -rng.uniform(0.2, 1.5), -rng.uniform(0.5, 2.5)
    model = host.Model.read(_tmp("fuzz%d.param" % case,
                                 "stationary\t%.6f\t%.6f\nbaseline\t%.6f\t%.6f\n" % (st0, st1, b0, b1)), scale=True)
    n = int(rng.choice([3, 17, 500, 2001]))
    fp = host.simulate(model, tree, n, int(rng.randint(1, 1 << 30)))
    cap = int(max(16, 2 * fp.counts().max() + 8))
    seed = int(rng.randint(1, 1 << 62))
    return tree, model, fp, cap, seed


def _wide_case(case):
    """cases 12 .. 23: the wide model box, branches 1e-4 .. 1, 17 .. 400 sites"""
    rng = np.random.RandomState(3000 + case)
    n_leaves = int(rng.randint(2, 13))
    text = _random_newick(rng, n_leaves)
    # the branch lengths of _random_newick span two orders: square them for four (1e-4 .. 1)
    tree = host.Tree.read(_tmp("fuzz%d.nwk" % case, text))
    tree = host.Tree(tree.subtree_sizes, tree.parent_ids, tree.branches ** 2, tree.node_names)
    st0, st1 = rng.uniform(0.02, 0.999, size=2)
    b0, b1 = rng.uniform(-6.0, 2.0, size=2)
    model = host.Model.read(_tmp("fuzz%d.param" % case,
                                 "stationary\t%.6f\t%.6f\nbaseline\t%.6f\t%.6f\n" % (st0, st1, b0, b1)), scale=True)
    n = int(rng.choice([17, 150, 400]))
    fp = host.simulate(model, tree, n, int(rng.randint(1, 1 << 30)))
    cap = int(max(16, 2 * fp.counts().max() + 8))
    seed = int(rng.randint(1, 1 << 62))
    return tree, model, fp, cap, seed


WIDE = range(12, 24)


def _case(case):
    return _wide_case(case) if case in WIDE else _random_case(case)


def _oracle_run(case):
    """rung B through everything the GPU twin runs -> (the states it compares with, the counters)"""
    tree, model, fp, cap, seed = _case(case)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    o.reset()
    out = [o.tri_llh()]
    for w in range(2):
        out.append((o.sweep(w), o.paths(), o.tri_llh()))
    out.append(o.run_mcmc(1, 2, sweep_base=5))
    return out, o.counters()


@pytest.mark.parametrize("case", WIDE)
def test_wide_case_meets_the_work_bound(case):
    """a condition, not a measurement (model_cases.py): trials / segments <= 64 on the oracle, finite likelihoods
    and rates inside the box's reach"""
    import model_cases as mc
    tree, model, fp, cap, seed = _case(case)
    out, c = _oracle_run(case)
    print(case, "rates %.3g .. %.3g, branches %.3g .. %.3g, n %d, trials / segment %.2f, overflow %d"
          % (model.rates.min(), model.rates.max(), tree.branches[1:].min(), tree.branches[1:].max(), fp.n_sites,
             mc.work(c), c["overflow"]))
    assert mc.work(c) <= mc.WORK_BOUND, c
    assert np.all(np.isfinite(out[0][1:-1])) and np.all(np.isfinite(out[2][2][1:-1]))


def test_wide_cases_are_wide():
    rates = np.array([_case(c)[1].rates for c in WIDE])
    br = np.concatenate([_case(c)[0].branches[1:] for c in WIDE])
    # (scale=True normalises a model to one substitution per unit time, which keeps the rates of this box within
    # 2e-3 .. 23; the extreme rates are the named models of model_cases.py)
    assert rates.max() / rates.min() > 5e3 and br.max() / br.min() > 5e3
    assert (rates.max(1) / rates.min(1)).max() > 1e3


@pytest.mark.parametrize("case", range(24))
def test_random_case_rung_a_vs_linked_reference(case):
    """the same random inputs, reference-schedule rung against the LINKED reference, live
    (against its stored outputs, tests/golden/ref/, where oracle/_ref is absent)"""
    tree, model, fp, cap, seed = _case(case)

    def reference():
        R = orc.Reference(tree, model, fp, seed=seed & 0xffffffff)
        R.reset(1, 2)
        llh0 = R.tri_llh()
        Jr, Dr, accr = R.run_mcmc()
        return dict(llh0=llh0, J=Jr, D=Dr, acc=np.float64(accr), **refvec.pack_paths("paths", R.paths()))

    r = refvec.reference_outputs("fuzz_case%d" % case, reference)
    o = orc.Oracle(tree, model, fp, "A", seed=seed & 0xffffffff)
    o.reset()
    assert np.array_equal(o.tri_llh(), r["llh0"])
    Jo, Do, nacc, acc = o.run_mcmc(1, 2)
    assert np.array_equal(Jo, r["J"]) and np.array_equal(Do, r["D"]) and acc == float(r["acc"])
    assert orc.paths_equal(o.paths(), refvec.unpack_paths("paths", r))


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(24))
def test_random_tree_model_seed(case):
    tree, model, fp, cap, seed = _case(case)
    if case in WIDE:
        # the oracle first: no device context unless its run of the same calls meets the work bound
        import model_cases as mc
        assert mc.work(_oracle_run(case)[1]) <= mc.WORK_BOUND
    from epievo_amd.sampler import DeviceSampler
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    d.upload_paths(fp, cap)
    d.reset()
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    o.reset()
    assert np.array_equal(d.tri_llh(), o.tri_llh())
    for w in range(2):
        assert d.sweep(1, seed, sweep_base=w) == o.sweep(w)
        assert orc.paths_equal(d.paths(), o.paths())
        assert np.array_equal(d.tri_llh(), o.tri_llh())
    Jd, Dd, nd = d.run_mcmc(1, 2, seed, sweep_base=5)
    Jo, Do, no, _ = o.run_mcmc(1, 2, sweep_base=5)
    assert nd == no and np.array_equal(Jd, Jo) and np.array_equal(Dd, Do)
    assert d.counters()["overflow"] == o.counters()["overflow"]
