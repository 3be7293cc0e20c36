"""Pins of tests/predictive_ref.py, the NumPy restatement of the posterior predictive density
that the GPU tests hold the device kernels to:

  1. it is a density: over all 2^P rows the per-state predictive sums to 1, with an empty label and beta != gamma;
  2. it is the oracle's own allocation conditional for an (N+1)-th observation (oracle.collapsed_cond / dp_cond /
     sb_cond, unchanged) wherever the two are meant to agree, and differs from it by exactly the stated term in
     the two places they are not (an emptied label of the finite collapsed sampler; the DP's new-cluster term
     when beta != gamma);
  3. it estimates what it should: exp(lppd) from a batch-1 oracle chain's states against the exact p(x* | X) by
     enumeration on data small enough to enumerate, within four standard errors of the chain's own estimate.
"""
import itertools

import numpy as np
import pytest
from scipy.special import betaln, gammaln, logsumexp

import predictive_ref as pref

RTOL = 1e-12  # the project's known-answer tolerance (tests/test_oracle_kats.py)


def _state(rng, N, P, K, empty=()):
    """data, 1-based labels that leave the labels in `empty` unused, and the counts"""
    X = np.asfortranarray((rng.random((N, P)) < 0.2 + 0.6 * rng.random(P)).astype(np.int32))
    live = [k for k in range(K) if k not in empty]
    z = np.array([live[i % len(live)] for i in range(N)], dtype=np.int32)
    rng.shuffle(z)
    z += 1
    Nk, S = pref.counts_from_labels(X, z, K)
    return X, z, Nk, S


# ---------------------------------------------------------------- 1. sums to one
@pytest.mark.parametrize("P", [1, 4, 10])
def test_collapsed_predictive_sums_to_one_with_an_empty_label(P):
    rng = np.random.default_rng(100 + P)
    X, z, Nk, S = _state(rng, 60, P, 5, empty=(2,))
    assert Nk[2] == 0
    t = pref.collapsed_terms(pref.all_rows(P), Nk, S, 1.7, 60, 0.7, 0.4)
    assert abs(np.exp(pref.logdens(t)).sum() - 1.0) < 1e-12
    assert np.abs(pref.resp(t).sum(axis=1) - 1.0).max() < 1e-14


@pytest.mark.parametrize("P", [1, 4, 10])
def test_dp_predictive_sums_to_one_with_unused_labels_and_asymmetric_prior(P):
    rng = np.random.default_rng(200 + P)
    X, z, Nk, S = _state(rng, 60, P, 6, empty=(1, 4))
    t = pref.dp_terms(pref.all_rows(P), Nk, S, 0.9, 60, 0.3, 1.1)
    assert t.shape[1] == 7 and np.all(np.isneginf(t[:, [1, 4]]))
    assert abs(np.exp(pref.logdens(t)).sum() - 1.0) < 1e-12
    assert np.abs(pref.resp(t).sum(axis=1) - 1.0).max() < 1e-14


@pytest.mark.parametrize("P", [1, 4, 10])
def test_explicit_predictive_sums_to_one(P):
    rng = np.random.default_rng(300 + P)
    pi = rng.dirichlet(np.ones(4))
    theta = rng.random((4, P))
    t = pref.explicit_terms(pref.all_rows(P), pi, theta)
    assert abs(np.exp(pref.logdens(t)).sum() - 1.0) < 1e-12


# ---------------------------------------------------------------- 2. the oracle's own conditionals
def _appended(X, z, x, label):
    return (np.asfortranarray(np.vstack([X, x[None, :]]).astype(np.int32)),
            np.append(z, label).astype(np.int32))


@pytest.mark.parametrize("spec", [False, True])
def test_collapsed_predictive_is_the_oracle_conditional_of_an_appended_row(oracle, spec):
    N, P, K, alpha, beta, gamma = 400, 7, 4, 1.3, 0.7, 0.4
    rng = np.random.default_rng(1)
    X, z, Nk, S = _state(rng, N, P, K)
    Xnew = (rng.random((50, P)) < 0.5).astype(np.int32)
    want = pref.logdens(pref.collapsed_terms(Xnew, Nk, S, alpha, N, beta, gamma))
    worst = 0.0
    for m in range(50):
        X1, z1 = _appended(X, z, Xnew[m], 1 + m % K)  # any valid label: observation N itself is left out
        raw, _ = oracle.collapsed_cond(X1, z1, N, K, alpha, beta, gamma, spec=spec)
        got = logsumexp(raw) if spec else np.log(raw.sum())
        worst = max(worst, abs(got - want[m]) / abs(want[m]))
        assert got == pytest.approx(want[m], rel=RTOL)
    print("largest relative difference", worst)


@pytest.mark.parametrize("spec", [False, True])
def test_dp_predictive_is_the_oracle_conditional_of_an_appended_row(oracle, spec):
    N, P, K, alpha, beta = 300, 6, 5, 0.8, 0.5  # beta == gamma: the only case the reference's new-cluster term is the model's
    rng = np.random.default_rng(2)
    X, z, Nk, S = _state(rng, N, P, K)
    Xnew = (rng.random((40, P)) < 0.5).astype(np.int32)
    want = pref.logdens(pref.dp_terms(Xnew, Nk, S, alpha, N, beta, beta))
    for m in range(40):
        X1, z1 = _appended(X, z, Xnew[m], 1 + m % K)
        logw, _ = oracle.dp_cond(X1, z1, N, K, alpha, beta, beta, spec=spec)
        assert logsumexp(logw) == pytest.approx(want[m], rel=RTOL)


@pytest.mark.parametrize("spec", [False, True])
def test_explicit_predictive_is_the_oracle_stickbreaking_conditional(oracle, spec):
    P, K = 9, 4
    rng = np.random.default_rng(3)
    pi = rng.dirichlet(np.ones(K))
    theta = np.asfortranarray(0.05 + 0.9 * rng.random((K, P)))
    Xnew = np.asfortranarray((rng.random((40, P)) < 0.5).astype(np.int32))
    want = pref.logdens(pref.explicit_terms(Xnew, pi, theta))
    for m in range(40):
        raw, _ = oracle.sb_cond(Xnew, m, pi, theta, spec=spec)
        got = logsumexp(raw) if spec else np.log(raw.sum())
        assert got == pytest.approx(want[m], rel=RTOL)


def test_an_emptied_label_is_the_whole_difference_from_the_collapsed_conditional(oracle):
    """The finite collapsed sampler gives an emptied label probability 0 for ever; the predictive keeps its prior
    weight (alpha/K)/(N + alpha) and the prior Bernoulli terms.  Every other category is the oracle's."""
    N, P, K, alpha, beta, gamma = 200, 6, 4, 1.3, 0.7, 0.4
    rng = np.random.default_rng(4)
    X, z, Nk, S = _state(rng, N, P, K, empty=(2,))
    Xnew = (rng.random((30, P)) < 0.5).astype(np.int32)
    t = pref.collapsed_terms(Xnew, Nk, S, alpha, N, beta, gamma)
    prior = np.log(alpha / K) - np.log(N + alpha) + (Xnew * np.log(beta) + (1 - Xnew) * np.log(gamma) - np.log(beta + gamma)).sum(axis=1)
    np.testing.assert_allclose(t[:, 2], prior, rtol=RTOL)
    for m in range(30):
        X1, z1 = _appended(X, z, Xnew[m], 1)
        raw, _ = oracle.collapsed_cond(X1, z1, N, K, alpha, beta, gamma)
        assert raw[2] == 0.0
        np.testing.assert_allclose(np.log(raw[[0, 1, 3]]), t[m, [0, 1, 3]], rtol=RTOL)
        assert np.exp(pref.logdens(t[m:m + 1]))[0] - raw.sum() == pytest.approx(np.exp(prior[m]), rel=1e-9)


def test_the_new_cluster_term_is_the_whole_difference_from_the_dp_conditional(oracle):
    """The reference's new-cluster term is P (log beta - log(beta + gamma)) whatever x is; the model's is
    sum_d x_d log beta + (1 - x_d) log gamma - P log(beta + gamma).  They differ by sum_d (1 - x_d)(log beta - log gamma)."""
    N, P, K, alpha, beta, gamma = 200, 6, 4, 0.8, 0.3, 1.1
    rng = np.random.default_rng(5)
    X, z, Nk, S = _state(rng, N, P, K)
    Xnew = (rng.random((30, P)) < 0.5).astype(np.int32)
    Xnew[0] = 1
    t = pref.dp_terms(Xnew, Nk, S, alpha, N, beta, gamma)
    for m in range(30):
        X1, z1 = _appended(X, z, Xnew[m], 1)
        logw, _ = oracle.dp_cond(X1, z1, N, K, alpha, beta, gamma)
        np.testing.assert_allclose(logw[:K], t[m, :K], rtol=RTOL)
        want = (1 - Xnew[m]).sum() * (np.log(beta) - np.log(gamma))
        np.testing.assert_allclose(logw[K] - t[m, K], want, rtol=1e-11, atol=1e-13)


# ---------------------------------------------------------------- 3. what it estimates
N7, P7 = 7, 3
BETA = GAMMA = 0.5


@pytest.fixture(scope="module")
def data7():
    """the seven observations of tests/test_oracle_posterior.py"""
    rng = np.random.default_rng(11)
    X = (rng.random((N7, P7)) < [0.8, 0.3, 0.6]).astype(np.int32)
    X[:3, 0] = 1
    X[4:, 0] = 0
    return np.asfortranarray(X)


def _ml(rows):
    """log marginal likelihood of a block of rows under the Beta-Bernoulli model (scipy, no sampler arithmetic)"""
    rows = np.atleast_2d(rows)
    n, s = rows.shape[0], rows.sum(axis=0)
    return float(np.sum(betaln(BETA + s, GAMMA + n - s) - betaln(BETA, GAMMA)))


def _partitions(n):
    def rec(prefix, m):
        if len(prefix) == n:
            yield tuple(prefix)
            return
        for v in range(m + 1):
            yield from rec(prefix + [v], max(m, v + 1))
    return list(rec([0], 1))


def _batch_means_se(series, nbatch=40):
    """standard error of the mean of a correlated series (S, M) by batch means"""
    S = series.shape[0] // nbatch * nbatch
    means = series[:S].reshape(nbatch, -1, series.shape[1]).mean(axis=1)
    return means.std(axis=0, ddof=1) / np.sqrt(nbatch)


def test_dp_lppd_estimates_the_exact_predictive_over_all_877_partitions(oracle, data7):
    """200 000 kept sweeps (2 000 burn-in) of the batch-1 oracle chain at fixed alpha = 1.3; per-sweep counts are
    recomputed from the returned labels.  Measured: standard errors 2.5e-5 .. 6.3e-5 (batch means, 40 batches),
    largest |difference| / standard error 1.43."""
    alpha, sweeps, burn = 1.3, 200_000, 2_000
    rows = pref.all_rows(P7)
    parts = _partitions(N7)
    assert len(parts) == 877
    logw, pred = [], []
    for p in parts:
        blocks = {}
        for i, b in enumerate(p):
            blocks.setdefault(b, []).append(i)
        logw.append(len(blocks) * np.log(alpha) + sum(gammaln(len(r)) + _ml(data7[r]) for r in blocks.values()))
        px = []
        for x in rows:
            v = alpha / (N7 + alpha) * np.exp(_ml(x))
            for r in blocks.values():
                v += len(r) / (N7 + alpha) * np.exp(_ml(np.vstack([data7[r], x])) - _ml(data7[r]))
            px.append(v)
        pred.append(px)
    post = np.exp(np.array(logw) - max(logw))
    post /= post.sum()
    exact = post @ np.array(pred)
    assert abs(exact.sum() - 1.0) < 1e-12
    maxK = 12  # never binds on seven observations
    r = oracle.dp(data7, sweeps + burn, alpha, BETA, GAMMA, 1, 1, burn, maxK, seed=5, batch=1)
    assert np.all(r["alpha"] == alpha)
    states, inverse = np.unique(r["z"], axis=0, return_inverse=True)
    table = np.empty((len(states), len(rows)))
    for u, z in enumerate(states):
        Nk, S = pref.counts_from_labels(data7, z, maxK)
        table[u] = pref.logdens(pref.dp_terms(rows, Nk, S, alpha, N7, BETA, GAMMA))
    trace = table[inverse.ravel()]                  # (sweeps, 2^P) log p(x* | state)
    got = np.exp(pref.lppd(trace))
    se = _batch_means_se(np.exp(trace))
    print("dp: se", se, "z-scores", (got - exact) / se)
    assert np.all(np.abs(got - exact) < 4 * se), (got, exact, se)


def test_full_lppd_estimates_the_exact_predictive_over_all_128_allocations(oracle, data7):
    """40 000 kept sweeps (2 000 burn-in) of the oracle's gibbs_full chain, K = 2, fixed alpha = 2; the exact
    predictive integrates pi and theta out over all 2^7 allocations.  Measured: standard errors 3.4e-4 .. 7.6e-4 (batch means, 40 batches),
    largest |difference| / standard error 2.45."""
    K, alpha, sweeps, burn = 2, 2.0, 40_000, 2_000
    rows = pref.all_rows(P7)
    logw, pred = [], []
    for z in itertools.product(range(K), repeat=N7):
        z = np.array(z)
        n = np.bincount(z, minlength=K)
        logw.append(float(np.sum(gammaln(alpha / K + n) - gammaln(alpha / K))) + sum(_ml(data7[z == k]) for k in range(K) if n[k]))
        px = []
        for x in rows:
            v = 0.0
            for k in range(K):
                blk = data7[z == k]
                v += (alpha / K + n[k]) / (alpha + N7) * np.exp(_ml(np.vstack([blk, x])) - (_ml(blk) if n[k] else 0.0))
            px.append(v)
        pred.append(px)
    post = np.exp(np.array(logw) - max(logw))
    post /= post.sum()
    exact = post @ np.array(pred)
    assert abs(exact.sum() - 1.0) < 1e-12
    r = oracle.full(data7, np.ones(K) / K, np.full((K, P7), 0.5), sweeps + burn, K, alpha, BETA, GAMMA, 1, 1, burn, seed=4)
    trace = np.empty((sweeps, len(rows)))
    for s in range(sweeps):
        trace[s] = pref.logdens(pref.explicit_terms(rows, r["pi"][s], r["theta"][:, :, s]))
    got = np.exp(pref.lppd(trace))
    se = _batch_means_se(np.exp(trace))
    print("full: se", se, "z-scores", (got - exact) / se)
    assert np.all(np.abs(got - exact) < 4 * se), (got, exact, se)
