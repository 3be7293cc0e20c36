"""The oracle's gamma, beta and update_alpha variates against their distributions over the whole shape plane the
samplers accept (any beta, gamma > 0; shapes from 1e-3 to 3e8), scipy.stats as the reference.  The device is held to
the oracle bit for bit over the same grid (test_gpu_variates.py), so what is shown here for the oracle holds for the
kernels.  The band is a binomial bound (variates_cases.py), not a measured figure.

What these tests found (profiles/variates/README.md): with X / (X + Y) alone, Beta(1e-3, 1e-3) was NaN in a quarter of
its draws and Beta(3e-3, 3e-3) in 1.4 %; with the NaN alone repaired, Beta(1e-3, 1e-3) was still 15 sigma off at its
0.3 quantile, because a draw with ONE flushed gamma returned exactly 0 or 1 whatever the flushed variate's share.
rbeta_ decides from the logarithms whenever either gamma flushed."""
import numpy as np
import pytest

import variates_cases as vc


@pytest.mark.parametrize("shape", vc.GAMMA_SHAPES, ids=["%.17g" % s for s in vc.GAMMA_SHAPES])
def test_gamma_follows_its_law(oracle, shape):
    g = oracle.rgamma_array(np.full(vc.N_DRAWS, shape), 20241 + vc.GAMMA_SHAPES.index(shape), 1)
    assert not np.isnan(g).any()
    assert (g >= 0.0).all() and np.isfinite(g).all()
    q, usable = vc.usable_gamma(shape)
    dev, j = vc.law_deviations(g, q, usable)
    print("gamma(%g): worst %.2f sigma at p = %d/20, %d usable points, %d draws exactly 0" % (shape, dev, j, usable.sum(), (g == 0).sum()))
    assert dev <= vc.SIGMAS, (shape, dev, j)


@pytest.mark.parametrize("p,q", vc.BETA_PAIRS, ids=["%g-%g" % pq for pq in vc.BETA_PAIRS])
def test_beta_follows_its_law(oracle, p, q):
    b = oracle.rbeta_array(np.full(vc.N_DRAWS, p), np.full(vc.N_DRAWS, q), 777 + vc.BETA_PAIRS.index((p, q)), 2)
    n_nan = int(np.isnan(b).sum())
    print("beta(%g, %g): %d NaN, %d exactly 0, %d exactly 1" % (p, q, n_nan, (b == 0).sum(), (b == 1).sum()))
    assert n_nan == 0, "%d of %d draws are NaN" % (n_nan, b.size)
    assert ((b >= 0.0) & (b <= 1.0)).all()
    x, usable = vc.usable_beta(p, q)
    dev, j = vc.law_deviations(b, x, usable)
    print("beta(%g, %g): worst %.2f sigma at p = %d/20, %d usable points" % (p, q, dev, j, usable.sum()))
    assert dev <= vc.SIGMAS, (p, q, dev, j)


def test_beta_is_a_number_in_the_unit_interval_for_every_positive_pair(oracle):
    """shapes down to the smallest positive doubles, where log(u) / p overflows: never NaN, always in [0, 1]"""
    tiny = np.array([5e-324, 1e-310, 2.4e-307, 1e-300, 1e-100, 1e-20, 1e-6, 1e-3, 1.0, 1e8])
    p, q = (m.reshape(-1) for m in np.meshgrid(tiny, tiny, indexing="ij"))
    p, q = np.tile(p, 50), np.tile(q, 50)
    b = oracle.rbeta_array(p, q, 5, 3)
    assert not np.isnan(b).any() and ((b >= 0.0) & (b <= 1.0)).all()


def test_update_alpha_is_finite_and_positive_over_the_plane(oracle):
    triples, old, K = vc.alpha_grid()
    reps = 40
    for t, (a, b, N) in enumerate(triples):
        got = oracle.update_alpha_array(np.tile(old, reps), np.tile(K, reps), a, b, N, 1000 * t, 4)
        assert np.isfinite(got).all() and (got > 0.0).all(), (a, b, N, got.min())
