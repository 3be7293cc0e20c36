"""Pins of tests/loo_ref.py, the NumPy restatement of the leave-one-out predictive of the fitted rows (DESIGN.md
section 14) that the GPU tests hold the device kernels to:

  1. it is the predictive: predictive_ref applied to statistics recounted from the labels without row i;
  2. it is the sampler's own conditional: the log-sum of the oracle's unnormalised allocation weights of row i
     wherever no label is emptied, and differs from it by exactly the stated term in the two quirk cases;
  3. it estimates what it should: log_cpo folded from batch-1 oracle chains against the exact log p(x_i | X_-i) by
     enumerating every allocation of the other six rows, within four standard errors of the harmonic mean.
"""
import itertools

import numpy as np
import pytest
from scipy.special import betaln, gammaln, logsumexp

import loo_ref as lref
import predictive_ref as pref

RTOL = 1e-12


def _state(rng, N, P, K, labels):
    X = np.asfortranarray((rng.random((N, P)) < 0.2 + 0.6 * rng.random(P)).astype(np.int32))
    z = np.asarray(labels, dtype=np.int32)
    Nk, S = pref.counts_from_labels(X, z, K)
    return X, z, Nk, S


def _labels(rng, N, live, singles=()):
    """labels over `live` (1-based), then one row alone in each label of `singles`"""
    z = rng.choice(list(live), N).astype(np.int32)
    for q, k in enumerate(singles):
        z[q] = k
    return z


# ---------------------------------------------------------------- 1. the predictive of the recount
@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
def test_loo_is_the_predictive_of_the_statistics_without_the_row(sampler):
    """labels 3 and 7 of 8 hold one row each, label 5 none: every case of the definition"""
    rng = np.random.default_rng(7)
    N, P, K, alpha, beta, gamma = 90, 11, 8, 1.3, 0.7, 0.4
    X, z, Nk, S = _state(rng, N, P, K, _labels(rng, N, [1, 2, 4, 6, 8], singles=(3, 7)))
    assert Nk[2] == 1 and Nk[6] == 1 and Nk[4] == 0
    got = lref.counting_ell(X, z, Nk, S, alpha, beta, gamma, sampler)
    want = lref.recount_ell(X, z, K, alpha, beta, gamma, sampler)
    print(sampler, "largest relative difference", np.max(np.abs(got - want) / np.abs(want)))
    np.testing.assert_allclose(got, want, rtol=RTOL)
    T = lref.counting_terms(X, z, Nk, S, alpha, beta, gamma, sampler)
    prior = (X * np.log(beta) + (1 - X) * np.log(gamma) - np.log(beta + gamma)).sum(axis=1)
    if sampler == "collapsed":  # an emptied label keeps its prior weight and the prior Bernoulli terms
        for i, k in ((0, 2), (1, 6)):
            assert T[i, k] == pytest.approx(np.log(alpha / K) - np.log(N - 1 + alpha) + prior[i], rel=RTOL)
        np.testing.assert_allclose(T[:, 4], np.log(alpha / K) - np.log(N - 1 + alpha) + prior, rtol=RTOL)
    else:  # a row that sat alone: its own label is unused; the new cluster carries alpha / (N - 1 + alpha)
        assert np.isneginf(T[0, 2]) and np.isneginf(T[1, 6]) and np.all(np.isneginf(T[:, 4]))
        np.testing.assert_allclose(T[:, K], np.log(alpha) - np.log(N - 1 + alpha) + prior, rtol=RTOL)


def test_explicit_loo_is_the_predictive_of_the_fitted_rows():
    rng = np.random.default_rng(8)
    X = (rng.random((40, 9)) < 0.5).astype(np.int32)
    pi, theta = rng.dirichlet(np.ones(5)), 0.05 + 0.9 * rng.random((5, 9))
    assert np.array_equal(lref.explicit_ell(X, pi, theta), pref.logdens(pref.explicit_terms(X, pi, theta)))
    dens = np.exp(lref.explicit_ell(pref.all_rows(9), pi, theta))
    assert abs(dens.sum() - 1.0) < 1e-12


def test_counting_loo_is_a_density_in_the_left_out_row():
    """over all 2^P values of x_i, the other rows fixed, exp(ell_i) sums to 1 -- a singleton and an empty label included"""
    rng = np.random.default_rng(9)
    N, P, K = 30, 6, 5
    z = _labels(rng, N, [1, 2, 4], singles=(3,))
    X0 = (rng.random((N, P)) < 0.5).astype(np.int32)
    for sampler in ("collapsed", "dp"):
        for i in (0, 5):
            tot = 0.0
            for x in pref.all_rows(P):
                X = X0.copy()
                X[i] = x
                Nk, S = pref.counts_from_labels(X, z, K)
                tot += np.exp(lref.counting_ell(X, z, Nk, S, 0.9, 0.3, 1.1, sampler)[i])
            assert abs(tot - 1.0) < 1e-12, (sampler, i, tot)


# ---------------------------------------------------------------- 2. the sampler's own conditional
@pytest.mark.parametrize("spec", [False, True])
def test_collapsed_loo_is_the_log_normaliser_of_the_oracle_conditional(oracle, spec):
    N, P, K, alpha, beta, gamma = 300, 7, 4, 1.3, 0.7, 0.4
    rng = np.random.default_rng(1)
    X, z, Nk, S = _state(rng, N, P, K, _labels(rng, N, [1, 2, 3, 4]))
    assert Nk.min() > 1  # no label is emptied by taking a row out
    ell = lref.counting_ell(X, z, Nk, S, alpha, beta, gamma, "collapsed")
    worst = 0.0
    for i in range(0, N, 5):
        raw, _ = oracle.collapsed_cond(X, z, i, K, alpha, beta, gamma, spec=spec)
        got = logsumexp(raw) if spec else np.log(raw.sum())
        worst = max(worst, abs(got - ell[i]) / abs(ell[i]))
        assert got == pytest.approx(ell[i], rel=RTOL)
    print("largest relative difference", worst)


@pytest.mark.parametrize("spec", [False, True])
def test_dp_loo_is_the_log_normaliser_of_the_oracle_conditional(oracle, spec):
    N, P, K, alpha, beta = 200, 6, 6, 0.8, 0.5  # beta == gamma: the only case the reference's new-cluster term is the model's
    rng = np.random.default_rng(2)
    X, z, Nk, S = _state(rng, N, P, K, _labels(rng, N, [1, 2, 4, 5], singles=(3,)))  # row 0 sits alone, label 6 is unused
    ell = lref.counting_ell(X, z, Nk, S, alpha, beta, beta, "dp")
    for i in range(0, N, 4):
        logw, _ = oracle.dp_cond(X, z, i, K, alpha, beta, beta, spec=spec)
        assert logsumexp(logw) == pytest.approx(ell[i], rel=RTOL)
    logw, _ = oracle.dp_cond(X, z, 0, K, alpha, beta, beta, spec=spec)
    assert np.isneginf(logw[2])  # the row that sat alone: its own label is unused for the sampler too


def test_an_emptied_label_is_the_whole_difference_from_the_collapsed_conditional(oracle):
    """The finite collapsed sampler gives an emptied (or empty) label probability 0 for ever; the leave-one-out
    predictive keeps its prior weight (alpha/K)/(N - 1 + alpha) and the prior Bernoulli terms.  Every other category
    is the oracle's."""
    N, P, K, alpha, beta, gamma = 150, 6, 5, 1.3, 0.7, 0.4
    rng = np.random.default_rng(4)
    X, z, Nk, S = _state(rng, N, P, K, _labels(rng, N, [1, 2, 4], singles=(3,)))  # label 3: row 0 alone; label 5 empty
    T = lref.counting_terms(X, z, Nk, S, alpha, beta, gamma, "collapsed")
    prior = np.log(alpha / K) - np.log(N - 1 + alpha) + (X * np.log(beta) + (1 - X) * np.log(gamma) - np.log(beta + gamma)).sum(axis=1)
    for i in range(0, N, 3):
        raw, _ = oracle.collapsed_cond(X, z, i, K, alpha, beta, gamma)
        gone = [4] + ([2] if i == 0 else [])  # the empty label, and for row 0 the one it empties
        live = [k for k in range(K) if k not in gone]
        assert np.all(raw[gone] == 0.0)
        np.testing.assert_allclose(np.log(raw[live]), T[i, live], rtol=RTOL)
        np.testing.assert_allclose(T[i, gone], prior[i], rtol=RTOL)
        assert np.exp(pref.logdens(T[i:i + 1]))[0] - raw.sum() == pytest.approx(len(gone) * np.exp(prior[i]), rel=1e-9)


def test_the_new_cluster_term_is_the_whole_difference_from_the_dp_conditional(oracle):
    """The reference's new-cluster term is P (log beta - log(beta + gamma)) whatever x is; the model's is
    sum_d x_d log beta + (1 - x_d) log gamma - P log(beta + gamma).  They differ by sum_d (1 - x_d)(log beta - log gamma)."""
    N, P, K, alpha, beta, gamma = 150, 6, 5, 0.8, 0.3, 1.1
    rng = np.random.default_rng(5)
    X, z, Nk, S = _state(rng, N, P, K, _labels(rng, N, [1, 2, 4], singles=(3,)))
    X[1] = 1
    Nk, S = pref.counts_from_labels(X, z, K)
    T = lref.counting_terms(X, z, Nk, S, alpha, beta, gamma, "dp")
    for i in range(0, N, 3):
        logw, _ = oracle.dp_cond(X, z, i, K, alpha, beta, gamma)
        np.testing.assert_allclose(logw[:K], T[i, :K], rtol=RTOL)
        want = (1 - X[i]).sum() * (np.log(beta) - np.log(gamma))
        np.testing.assert_allclose(logw[K] - T[i, K], want, rtol=1e-11, atol=1e-13)


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


def _harmonic_se(trace, nbatch=40):
    """standard error of log_cpo = -log mean_s exp(-ell): batch means of exp(-ell), then the delta method"""
    w = np.exp(-trace)
    S = w.shape[0] // nbatch * nbatch
    means = w[:S].reshape(nbatch, -1, w.shape[1]).mean(axis=1)
    return means.std(axis=0, ddof=1) / np.sqrt(nbatch) / w.mean(axis=0)


def test_dp_log_cpo_estimates_the_exact_leave_one_out_predictive(oracle, data7):
    """200 000 kept sweeps (2 000 burn-in) of the batch-1 oracle chain at fixed alpha = 1.3 against
    log p(x_i | X_-i) over all 203 partitions of the other six rows.  The observed differences and standard errors are
    printed.  Measured: standard errors 2.3e-4 .. 4.3e-4 (batch means of exp(-ell), 40 batches, delta method), largest
    |difference| / standard error 1.17, ess 195 000 .. 197 300 of 200 000."""
    alpha, sweeps, burn, maxK = 1.3, 200_000, 2_000, 12
    parts = _partitions(N7 - 1)
    assert len(parts) == 203
    exact = np.empty(N7)
    for i in range(N7):
        rest = np.delete(data7, i, axis=0)
        logw, px = [], []
        for p in parts:
            blocks = {}
            for q, b in enumerate(p):
                blocks.setdefault(b, []).append(q)
            logw.append(len(blocks) * np.log(alpha) + sum(gammaln(len(r)) + _ml(rest[r]) for r in blocks.values()))
            v = alpha / (N7 - 1 + alpha) * np.exp(_ml(data7[i]))
            for r in blocks.values():
                v += len(r) / (N7 - 1 + alpha) * np.exp(_ml(np.vstack([rest[r], data7[i]])) - _ml(rest[r]))
            px.append(v)
        post = np.exp(np.array(logw) - max(logw))
        exact[i] = np.log(post @ np.array(px) / post.sum())
    r = oracle.dp(data7, sweeps + burn, alpha, BETA, GAMMA, 1, 1, burn, maxK, seed=5, batch=1)
    assert np.all(r["alpha"] == alpha)
    states, inverse = np.unique(r["z"], axis=0, return_inverse=True)
    table = np.empty((len(states), N7))
    for u, z in enumerate(states):
        Nk, S = pref.counts_from_labels(data7, z, maxK)
        table[u] = lref.counting_ell(data7, z, Nk, S, alpha, BETA, GAMMA, "dp")
    trace = table[inverse.ravel()]
    out = lref.summary(trace)
    se = _harmonic_se(trace)
    print("dp: log_cpo - exact", out["log_cpo"] - exact, "se", se, "z-scores", (out["log_cpo"] - exact) / se, "ess", out["ess"])
    assert np.all(np.abs(out["log_cpo"] - exact) < 4 * se), (out["log_cpo"], exact, se)
    assert np.all(out["ess"] >= 1.0) and np.all(out["ess"] <= sweeps)
    assert out["lpml"] == pytest.approx(out["log_cpo"].sum())


def test_full_log_cpo_estimates_the_exact_leave_one_out_predictive(oracle, data7):
    """40 000 kept sweeps (2 000 burn-in) of the oracle's gibbs_full chain, K = 2, fixed alpha = 2, against
    log p(x_i | X_-i) with pi and theta integrated out over all 2^6 allocations of the other six rows.  Measured:
    standard errors 6.9e-3 .. 1.3e-2, largest |difference| / standard error 0.83, ess 4 300 .. 18 100 of 40 000 (the
    harmonic mean over explicit parameters has the heavier tail)."""
    K, alpha, sweeps, burn = 2, 2.0, 40_000, 2_000
    exact = np.empty(N7)
    for i in range(N7):
        rest = np.delete(data7, i, axis=0)
        logw, px = [], []
        for z in itertools.product(range(K), repeat=N7 - 1):
            z = np.array(z)
            n = np.bincount(z, minlength=K)
            logw.append(float(np.sum(gammaln(alpha / K + n) - gammaln(alpha / K))) + sum(_ml(rest[z == k]) for k in range(K) if n[k]))
            v = 0.0
            for k in range(K):
                blk = rest[z == k]
                v += (alpha / K + n[k]) / (alpha + N7 - 1) * np.exp(_ml(np.vstack([blk, data7[i]])) - (_ml(blk) if n[k] else 0.0))
            px.append(v)
        post = np.exp(np.array(logw) - max(logw))
        exact[i] = np.log(post @ np.array(px) / post.sum())
    r = oracle.full(data7, np.ones(K) / K, np.full((K, P7), 0.5), sweeps + burn, K, alpha, BETA, GAMMA, 1, 1, burn, seed=4)
    trace = np.empty((sweeps, N7))
    for s in range(sweeps):
        trace[s] = lref.explicit_ell(data7, r["pi"][s], r["theta"][:, :, s])
    out = lref.summary(trace, waic=True)
    se = _harmonic_se(trace)
    print("full: log_cpo - exact", out["log_cpo"] - exact, "se", se, "z-scores", (out["log_cpo"] - exact) / se, "ess", out["ess"])
    assert np.all(np.abs(out["log_cpo"] - exact) < 4 * se), (out["log_cpo"], exact, se)
    assert out["elpd_waic"] == pytest.approx(out["lppd"].sum() - out["var"].sum())
