"""bm.ess and bm.rhat (NumPy on the host; include/bmm_mcmc.h "log joint trace" says what they are applied to).  The
bands were checked on the CPU over 20 seeds with a plain NumPy implementation: ess / (S (1 - phi) / (1 + phi)) of an
AR(1) series of S = 20000 measured 0.87 - 1.17; split-R-hat of four iid chains of 2000 below 1.01, and 1.09 - 1.12 with
one chain shifted by one standard deviation."""
import numpy as np
import pytest

import bmm_mcmc_amd as bm


def _ar1(rng, S, phi):
    e = rng.standard_normal(S)
    x = np.empty(S)
    x[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, S):
        x[t] = phi * x[t - 1] + e[t]
    return x


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("phi", [0.0, 0.9])
def test_ess_of_iid_and_ar1_series(seed, phi):
    S = 20000
    x = _ar1(np.random.default_rng(seed), S, phi)
    ratio = bm.ess(x) / (S * (1.0 - phi) / (1.0 + phi))
    print("ess ratio", phi, seed, ratio)
    assert 0.8 <= ratio <= 1.25


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rhat_of_iid_chains_and_of_a_shifted_chain(seed):
    rng = np.random.default_rng(seed)
    chains = [rng.standard_normal(2000) for _ in range(4)]
    r0 = bm.rhat(chains)
    chains[2] = chains[2] + 1.0
    r1 = bm.rhat(chains)
    print("rhat", seed, r0, r1)
    assert r0 < 1.01
    assert r1 > 1.05


def test_constant_and_short_series_give_nan():
    assert np.isnan(bm.ess(np.full(100, 3.25)))
    assert np.isnan(bm.rhat([np.full(100, 3.25), np.full(100, 3.25)]))
    assert np.isnan(bm.ess(np.arange(7.0)))           # fewer than 4 values per half
    assert np.isnan(bm.rhat([np.arange(7.0), np.arange(7.0)]))
    assert np.isfinite(bm.ess(np.random.default_rng(0).standard_normal(8)))
    assert np.isfinite(bm.rhat([np.random.default_rng(0).standard_normal(8)]))
    assert np.isnan(bm.ess([1.0, 2.0, np.nan, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]))
