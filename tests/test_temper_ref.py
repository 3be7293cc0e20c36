"""The restatement of parallel tempering (tests/temper_ref.py) held to what it must satisfy on its own, without a GPU:
the tempered scan leaves the tempered posterior invariant, the exchange leaves the product of two rungs' posteriors
invariant, at b = 1 the conditional is the oracle's, and the shapes and powers the device's exchange test uses make
every pair both accept and reject."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_merge_ref as smr  # noqa: E402
import temper_ref as tr  # noqa: E402

BETA = GAMMA = 0.5
ALPHA = 1.3


def five_rows():
    return np.array([[1, 1, 0], [1, 0, 0], [0, 1, 1], [0, 0, 1], [1, 1, 1]], dtype=np.int32)


@pytest.fixture(scope="module")
def enumerated():
    X = five_rows()
    parts = smr.partitions(len(X))
    assert len(parts) == 52
    return X, parts


@pytest.mark.parametrize("b", [1.0, 0.5, 0.1])
def test_tempered_scan_leaves_the_tempered_posterior_invariant(enumerated, b):
    X, parts = enumerated
    pi, _ = tr.tempered_posterior(X, parts, ALPHA, BETA, GAMMA, b)
    T = tr.scan_matrix(X, parts, ALPHA, BETA, GAMMA, b, K=6)
    np.testing.assert_allclose(T.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    err = np.abs(pi @ T - pi).max()
    print("b = %g: worst |pi T - pi| = %.2e" % (b, err))
    assert err <= 1e-12
    if b != 1.0:  # and the check can tell: the untempered posterior is not invariant under the tempered scan
        pi1, _ = tr.tempered_posterior(X, parts, ALPHA, BETA, GAMMA, 1.0)
        assert np.abs(pi1 @ T - pi1).max() > 1e-4


@pytest.mark.parametrize("b", [0.5, 0.1])
def test_exchange_leaves_the_product_of_the_two_posteriors_invariant(enumerated, b):
    X, parts = enumerated
    pi1, L = tr.tempered_posterior(X, parts, ALPHA, BETA, GAMMA, 1.0)
    pib, _ = tr.tempered_posterior(X, parts, ALPHA, BETA, GAMMA, b)
    joint = np.outer(pi1, pib).reshape(-1)
    T = tr.exchange_matrix(L, 1.0, b)
    np.testing.assert_allclose(T.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    err = np.abs(joint @ T - joint).max()
    print("b = %g: worst |(pi_1 x pi_b) T - (pi_1 x pi_b)| = %.2e" % (b, err))
    assert err <= 1e-12
    other = np.outer(pib, pi1).reshape(-1)  # the rungs the wrong way round
    assert np.abs(other @ T - other).max() > 1e-6


@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
def test_at_power_one_the_conditional_is_the_oracles(oracle, sampler):
    N, P, K = 60, 7, 5
    X, _ = tr.mixture(N, P, [0.2, 0.5, 0.8], 5)
    rng = np.random.default_rng(1)
    z = rng.integers(0, K - 2, N)  # the last label unused: the DP's new cluster has a label to open
    z[3] = K - 2                   # ... and label K - 2 holds one row: emptied when that row is scored
    got = tr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, 1.0, sampler)
    worst = 0.0
    for i in range(N):
        fn = oracle.collapsed_cond if sampler == "collapsed" else oracle.dp_cond
        _, want = fn(X, (z + 1).astype(np.int32), i, K, ALPHA, BETA, GAMMA, spec=True)
        mine = got[i]
        if sampler == "dp":  # the oracle lists the K labels, then the new-cluster option; here it sits under the label it opens
            n = np.bincount(np.delete(z, i), minlength=K)
            free = np.flatnonzero(n == 0)[0]
            folded = np.array(want[:K])
            assert folded[free] == 0.0
            folded[free] = want[K]
            want = folded
        big = want > 1e-300
        worst = max(worst, float(np.max(np.abs(mine[big] - want[big]) / want[big])))
        assert np.all(mine[~big] <= 1e-300)
    print("%s: worst relative difference at b = 1: %.2e" % (sampler, worst))
    assert worst <= 1e-12


def test_a_power_below_one_flattens_the_conditional():
    X, _ = tr.mixture(60, 7, [0.2, 0.5, 0.8], 5)
    z = np.random.default_rng(1).integers(0, 4, 60)
    for sampler in ("collapsed", "dp"):
        cold = tr.z_conditional(X, z, 5, ALPHA, BETA, GAMMA, 1.0, sampler)
        warm = tr.z_conditional(X, z, 5, ALPHA, BETA, GAMMA, 0.3, sampler)
        assert np.abs(cold - warm).max() > 1e-3
        # at b -> 0 the prior weights alone are left
        flat = tr.z_conditional(X, z, 5, ALPHA, BETA, GAMMA, 1e-300, sampler)
        n = np.bincount(z, minlength=5).astype(np.float64)
        for i in (0, 7, 31):
            m = n.copy()
            m[z[i]] -= 1
            w = np.where(m > 0, m + (ALPHA / 5 if sampler == "collapsed" else 0.0), 0.0)
            if sampler == "dp":
                w[np.flatnonzero(m == 0)[0]] = ALPHA
            np.testing.assert_allclose(flat[i], w / w.sum(), rtol=1e-12, atol=0)


def test_exchange_rule_and_uniform(oracle):
    assert tr.accepts(0.0, 0.999) and tr.accepts(3.0, 0.999)
    assert not tr.accepts(float("nan"), 0.0)
    assert not tr.accepts(-np.inf, 0.0)
    assert tr.accepts(-1.0, 0.3) and not tr.accepts(-1.0, 0.4)  # exp(-1) = 0.3679
    us = np.array([[tr.exchange_uniform(77, r, t) for r in range(7)] for t in range(40)])
    assert np.all((us >= 0.0) & (us < 1.0)) and len(np.unique(us)) == us.size
    assert 0.35 < us.mean() < 0.65
    assert tr.exchange_uniform(77, 1, 2) != tr.exchange_uniform(77, 2, 1) != tr.exchange_uniform(78, 2, 1)
    assert tr.proposed_pairs(5, 0) == [0, 2] and tr.proposed_pairs(5, 1) == [1, 3] and tr.proposed_pairs(2, 1) == []


@pytest.mark.parametrize("R", sorted(tr.EXCHANGE_POWERS))
def test_the_device_tests_ladders_both_accept_and_reject(oracle, R):
    """The data and the powers of the device's exchange-decision test: the restated ladder, with the device's uniforms
    and its own sweeps, both accepts and rejects at least 10 proposals of every pair in the test's 60 steps."""
    N, P, K = tr.EXCHANGE_SHAPE
    X, _ = tr.mixture(N, P, tr.EXCHANGE_THETAS, tr.EXCHANGE_DATA_SEED)
    z0 = np.random.default_rng(11).integers(0, K, N)
    out = tr.restated_ladder(X, z0, K, ALPHA, BETA, GAMMA, tr.EXCHANGE_POWERS[R], tr.EXCHANGE_STEPS, seed=5)
    rejected = out["proposed"] - out["accepted"]
    print("R = %d: proposed %s accepted %s" % (R, out["proposed"], out["accepted"]))
    assert np.all(out["accepted"] >= 10) and np.all(rejected >= 10)
    assert sorted(out["walker"]) == list(range(R))
