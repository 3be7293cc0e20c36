"""tests/logpost_ref.py -- the SciPy restatement of the log joint (include/bmm_mcmc.h "log joint trace") -- against
things that do not depend on it: its priors and its likelihood are normalised, its differences are the log ratios of
the samplers' own allocation conditionals as the oracle computes them, and the allocation model's value is
alloc_ref.log_target.  The host program and the device are then held to the restatement
(tests/test_logpost_host_cpu.py, tests/test_gpu_logpost.py)."""
import itertools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_ref  # noqa: E402
import logpost_ref as ref  # noqa: E402

N7 = 7


def _sum_exp(vals):
    vals = np.asarray(vals)
    m = vals.max()
    return math.exp(m) * float(np.sum(np.exp(vals - m)))


# ---------------------------------------------------------------- 1. the priors are normalised
@pytest.mark.parametrize("alpha", [0.7, 2.5])
def test_the_finite_prior_sums_to_one_over_the_labelled_states(alpha):
    vals = [ref.log_prior_counts("collapsed", np.bincount(z, minlength=3), N7, alpha)
            for z in itertools.product(range(3), repeat=N7)]
    assert abs(_sum_exp(vals) - 1.0) < 1e-12


@pytest.mark.parametrize("alpha", [0.7, 2.5])
def test_the_stick_breaking_prior_sums_to_one_and_depends_on_the_label_order(alpha):
    vals = [ref.log_prior_counts("stickbreaking", np.bincount(z, minlength=3), N7, alpha)
            for z in itertools.product(range(3), repeat=N7)]
    assert abs(_sum_exp(vals) - 1.0) < 1e-12
    a = ref.log_prior_counts("stickbreaking", [5, 1, 1], N7, alpha)
    b = ref.log_prior_counts("stickbreaking", [1, 1, 5], N7, alpha)
    assert abs(a - b) > 0.1  # the same partition under two numberings


@pytest.mark.parametrize("alpha", [0.7, 2.5])
def test_the_dp_prior_sums_to_one_over_the_877_partitions(alpha):
    """log_prior of the DP model is the probability of the PARTITION (the exchangeable partition probability function
    alpha^K+ prod Gamma(n_k) Gamma(alpha) / Gamma(alpha + N)): every numbering of its blocks within the maxK labels has
    this same value, and the labelled multiplicity it is summed with is 1 per partition."""
    parts = list(ref.partitions(N7))
    assert len(parts) == 877  # the Bell number B_7
    vals = [ref.log_prior_counts("dp", np.bincount(z, minlength=N7), N7, alpha) for z in parts]
    assert abs(_sum_exp(vals) - 1.0) < 1e-12
    # ... and the value does not depend on which of the maxK labels carry the blocks
    z = np.array(parts[400])
    assert ref.log_prior_counts("dp", np.bincount(z, minlength=9), N7, alpha) == pytest.approx(
        ref.log_prior_counts("dp", np.bincount(8 - z, minlength=9), N7, alpha), rel=1e-14)


@pytest.mark.parametrize("a", [0.6, 1.0])
def test_the_allocation_prior_sums_to_one_over_k_and_z(a):
    lpk = alloc_ref.poisson_prior(3)
    vals = []
    for K in (1, 2, 3):
        for z in itertools.product(range(K), repeat=N7):
            vals.append(ref.log_prior_counts("allocation", np.bincount(z, minlength=3), N7, a, k_open=K, log_prior_k=lpk))
    assert abs(_sum_exp(vals) - 1.0) < 1e-12


# ---------------------------------------------------------------- 2. the likelihood is normalised
@pytest.mark.parametrize("z,mask", [([0, 0, 0], None), ([0, 1, 0], None), ([2, 0, 1], None), ([0, 1, 0], [1, 0])])
def test_the_likelihood_sums_to_one_over_all_64_data_sets(z, mask):
    beta, gamma = 0.5, 1.25
    vals = []
    for bits in itertools.product((0, 1), repeat=6):
        X = np.array(bits).reshape(3, 2)
        Nk, S = ref.counts(X, z, 3)
        vals.append(ref.log_lik_counts(Nk, S, 3, beta, gamma, mask))
    assert abs(_sum_exp(vals) - 1.0) < 1e-12


# ---------------------------------------------------------------- 3. differences are the samplers' conditionals
def _data(N=12, P=5, seed=11):
    rng = np.random.default_rng(seed)
    theta = np.where(rng.random((3, P)) < 0.5, 0.2, 0.8)
    return np.asfortranarray((rng.random((N, P)) < theta[rng.integers(3, size=N)]).astype(np.int32))


# four states of 12 rows; every label that holds a row holds at least two, so that moving one row empties none (an
# emptied finite label is where the model and the finite sampler part)
STATES = [
    [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2],
    [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2],
    [2, 2, 2, 2, 2, 2, 0, 0, 1, 1, 1, 0],
    [1, 1, 0, 0, 0, 0, 0, 2, 2, 0, 0, 0],
]


def _assert_ratios(lj, prob, cats):
    """lj[c], prob[c] over the categories `cats`: every pairwise difference of lj is the log ratio of prob"""
    for c1, c2 in itertools.combinations(cats, 2):
        want = math.log(prob[c1]) - math.log(prob[c2])
        got = lj[c1] - lj[c2]
        assert abs(got - want) <= 1e-11 * abs(want), (c1, c2, got, want)


@pytest.mark.parametrize("state", range(4))
def test_differences_are_the_finite_samplers_conditional(oracle, state):
    X, K, alpha, beta, gamma = _data(), 3, 1.7, 0.5, 0.8
    z = np.array(STATES[state])
    for i in range(len(z)):
        _, prob = oracle.collapsed_cond(X, z + 1, i, K, alpha, beta, gamma)
        lj = {}
        for k in range(K):
            zz = z.copy(); zz[i] = k
            lj[k] = ref.log_joint("collapsed", X, zz, K, alpha, beta, gamma)[3]
        _assert_ratios(lj, prob, range(K))


@pytest.mark.parametrize("state", range(4))
def test_differences_are_the_dp_samplers_conditional(oracle, state):
    X, K, alpha, beta = _data(), 6, 1.7, 0.5  # beta == gamma: where the sampler's new-cluster term is the model's
    z = np.array(STATES[state])
    for i in range(len(z)):
        _, prob = oracle.dp_cond(X, z + 1, i, K, alpha, beta, beta)
        lj = {}
        for k in range(3):
            zz = z.copy(); zz[i] = k
            lj[k] = ref.log_joint("dp", X, zz, K, alpha, beta, beta)[3]
        zz = z.copy(); zz[i] = 3  # the new cluster: the first unused label; category K of the conditional
        lj[K] = ref.log_joint("dp", X, zz, K, alpha, beta, beta)[3]
        _assert_ratios(lj, prob, [0, 1, 2, K])


@pytest.mark.parametrize("state", range(4))
def test_differences_are_the_allocation_samplers_conditional(oracle, state):
    X, maxK, k_open, a, beta, gamma = _data(), 5, 4, 0.9, 0.5, 0.8  # label 3 open and empty, label 4 closed
    lpk = alloc_ref.poisson_prior(maxK)
    z = np.array(STATES[state])
    for i in range(len(z)):
        _, prob = oracle.alloc_cond(X, z + 1, i, maxK, k_open, a, beta, gamma)
        assert prob[4] == 0.0
        lj = {}
        for k in range(k_open):
            zz = z.copy(); zz[i] = k
            lj[k] = ref.log_joint("allocation", X, zz, maxK, a, beta, gamma, k_open=k_open, log_prior_k=lpk)[3]
        _assert_ratios(lj, prob, range(k_open))


# ---------------------------------------------------------------- 4. the allocation model's value
@pytest.mark.parametrize("state", range(4))
def test_the_allocation_value_is_alloc_refs_log_target(state):
    X, maxK, a, beta, gamma = _data(), 5, 0.9, 0.5, 0.8
    lpk = alloc_ref.poisson_prior(maxK)
    z = np.array(STATES[state])
    for k_open in (3, 4, 5):
        r = ref.log_joint("allocation", X, z, maxK, a, beta, gamma, k_open=k_open, log_prior_k=lpk)
        want = alloc_ref.log_target(k_open, z, X, a, beta, gamma, lpk)
        assert abs((r[0] + r[1]) - want) <= 1e-12 * abs(want)
        assert r[2] == 0.0
