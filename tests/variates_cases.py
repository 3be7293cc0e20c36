"""The shape plane the variate tests share (test_variates_law.py on the CPU, test_gpu_variates.py on the device): the
grids, the quantile check against scipy's distributions, and array helpers.

The law check: n draws, the empirical fraction <= q_j against p_j = j/20, j = 1..19, where q_j is the reference
quantile at p_j.  The count of draws <= q_j is Binomial(n, p_j), so the fraction lies within
5 sqrt(p_j (1 - p_j) / n) of p_j except with probability 5.7e-7 (two-sided normal tail at 5 sigma; n p_j >= 2000, so
the normal tail describes the binomial one): over the 29 grid points' 551 comparisons below 4e-4 in all, and the
seeds are fixed.  A quantile point is usable where the reference quantile is a number the variate can be compared
with: above 1e-300 (gamma, beta) and below 1 - 1e-15 (beta); a variate that rounded to exactly 0 or 1 then falls on the
right side of every usable point.  Every grid point has at least MIN_USABLE usable points (asserted)."""
import numpy as np
from scipy import stats

N_DRAWS = 40_000
PROBS = np.arange(1, 20) / 20.0
SIGMAS = 5.0
MIN_USABLE = 5

GAMMA_SHAPES = [1e-3, 3e-3, 1e-2, 0.05, 0.3, 0.5, 1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, 4.0 / 3.0, 3.7, 250.5, 1e3, 1e5,
                1e7, 3e8]
BETA_PAIRS = [(1e-3, 1e-3), (3e-3, 3e-3), (1e-2, 1e-2), (0.05, 0.05), (0.5, 0.5), (1.0, 1.0), (2.0, 5.0), (0.3, 1.7),
              (0.5, 120.5), (1e-3, 1e6), (1.0, 1e7), (3e6, 1.5), (1e7, 1e7)]

# update_alpha over a, b, N, K, alpha_old
ALPHA_A = [0.1, 1.0, 5.0]
ALPHA_B = [0.1, 1.0, 10.0]
ALPHA_N = [10.0, 1e3, 1e7]
ALPHA_K = [1, 2, 50]
ALPHA_OLD = [1e-3, 1.0, 50.0]


# Chains at small hyperparameters: N = 300, P = 40, three generating components, 60 sweeps.  (beta, gamma) and the
# kernel form by maxK: one lane per observation (12 accumulators), the resident kernel at 30, two lanes per
# observation above 32 accumulators, the generic kernels above 64 categories.
CHAIN_N, CHAIN_P, CHAIN_SWEEPS = 300, 40, 60
CHAIN_HYPER = [(0.3, 1.7), (0.05, 0.05), (0.01, 0.01), (0.003, 0.003)]
CHAIN_FORMS = {"one-lane": 10, "resident": 30, "two-lanes": 40, "generic": 70}


def chain_data():
    """X (N x P, column-major int32) from three components with rates 0.1 + 0.8 U, weights 3 : 2 : 1"""
    rng = np.random.Generator(np.random.PCG64(1234))
    theta = 0.1 + 0.8 * rng.random((3, CHAIN_P))
    lab = rng.choice(3, size=CHAIN_N, p=[0.5, 1.0 / 3.0, 1.0 / 6.0])
    return np.asfortranarray((rng.random((CHAIN_N, CHAIN_P)) < theta[lab]).astype(np.int32))


def chain_start(maxK):
    rng = np.random.default_rng(maxK)
    pi0 = np.exp(rng.random(maxK))
    return pi0 / pi0.sum(), rng.random((maxK, CHAIN_P))


def oracle_chain(oracle, sampler, X, maxK, beta, gamma, seed=17, **kw):
    """the oracle's chain of a case: alpha sampled under a = b = 1, every sweep kept"""
    pi0, th0 = chain_start(maxK)
    fn = oracle.stickbreaking if sampler == "stickbreaking" else oracle.full
    return fn(X, pi0, th0, CHAIN_SWEEPS, maxK, 0.0, beta, gamma, 1, 1, 0, seed=seed, **kw)


def alpha_grid():
    """[(a, b, N)], and per such triple the arrays alpha_old[i], K[i] over ALPHA_OLD x ALPHA_K"""
    old, K = np.meshgrid(ALPHA_OLD, np.asarray(ALPHA_K, dtype=np.float64), indexing="ij")
    return [(a, b, N) for a in ALPHA_A for b in ALPHA_B for N in ALPHA_N], old.reshape(-1).copy(), K.reshape(-1).copy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def usable_gamma(shape):
    q = stats.gamma.ppf(PROBS, shape)
    return q, q > 1e-300


def usable_beta(p, q):
    x = stats.beta.ppf(PROBS, p, q)
    return x, (x > 1e-300) & (x < 1.0 - 1e-15)


def law_deviations(draws, quantiles, usable):
    """(worst deviation in sigmas, its j) of the empirical fraction <= q_j from p_j over the usable points"""
    draws = np.asarray(draws)
    assert usable.sum() >= MIN_USABLE, "the grid point has only %d usable quantile points" % usable.sum()
    frac = (draws[:, None] <= quantiles[None, usable]).mean(axis=0)
    p = PROBS[usable]
    dev = np.abs(frac - p) / np.sqrt(p * (1.0 - p) / draws.size)
    j = int(np.argmax(dev))
    return float(dev[j]), int(np.flatnonzero(usable)[j]) + 1
