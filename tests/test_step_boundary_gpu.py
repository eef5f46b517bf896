"""The host side of an EM step's boundary: epv::SingleSiteSampler's persistent part threads and the stream-ordered
epv_set_model with its two pinned staging slots.

One sampler of three contexts goes through twenty reset(model) / run_mcmc iterations, every one under another
model; before each, two resets with decoy models are queued straight in front of the real one, so that three
copies of the constants wait on every stream while the host writes the slots again.  Each iteration's J, D,
acceptance rate and paths must equal, bit for bit, those of a fresh sampler that starts from the paths the long-lived
one held before that iteration.  In the middle run_mcmc is called without reset until the halos are used up: the
error of the contexts, raised on the part threads' side of the call, must reach the caller as it always did, and
the sampler must go on unharmed."""
import types

import numpy as np
import pytest

import orc
from common import config, ref_test_model
from epievo_amd import host

BURN_IN, BATCH, SEED = 2, 3, 17
N_SITES = 3300      # three parts: each owns more than its two 256-column halos plus two blocks
ITERATIONS = 20


def variant(model, i):
    """the model of iteration i: every triplet rate moved by its own factor"""
    f = 1.0 + 0.02 * ((np.arange(8) * 3 + i * 5) % 11 - 5) / 5.0 + 0.001 * i
    return types.SimpleNamespace(rates=np.asarray(model.rates, np.float64) * f, T=np.asarray(model.T, np.float64))


def test_models_differ():
    m = ref_test_model()
    seen = set(tuple(variant(m, i).rates) for i in range(-2, ITERATIONS))
    assert len(seen) == ITERATIONS + 2 and all(min(r) > 0 for r in seen)


@pytest.mark.gpu
def test_twenty_iterations_equal_twenty_fresh_samplers():
    from epievo_amd import driver
    model, tree = ref_test_model(), config("tree")
    fp = host.simulate(model, tree, N_SITES, 6)
    cap = int(max(16, 2 * fp.counts().max() + 8))
    s = driver.CppSampler(BURN_IN, BATCH, devices=[0], capacity=cap)
    s.reset(model, tree, fp)
    assert s.layout()["parts_here"] == 3
    raised = False
    for i in range(ITERATIONS):
        m = variant(model, i)
        before = s.paths()
        s.reset(variant(model, -1))
        s.reset(variant(model, -2))
        s.reset(m)
        J, D, acc = s.run_mcmc(SEED, i)
        f = driver.CppSampler(BURN_IN, BATCH, devices=[0], capacity=cap)
        f.reset(m, tree, before)
        Jf, Df, accf = f.run_mcmc(SEED, i)
        assert np.array_equal(J.view(np.uint64), Jf.view(np.uint64)), i
        assert np.array_equal(D.view(np.uint64), Df.view(np.uint64)), i
        assert acc == accf and acc > 0, i
        assert orc.paths_equal(s.paths(), f.paths()), i
        f.close()
        if i == 9:
            # 256 halo columns last 128 colour phases, a run_mcmc takes 15: the ninth call since the reset fails
            with pytest.raises(driver.DriverError, match="halo"):
                for k in range(12):
                    s.run_mcmc(SEED, 100 + k)
            raised = True
    assert raised
    s.close()
