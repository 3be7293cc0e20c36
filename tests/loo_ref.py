"""NumPy restatement of the leave-one-out predictive of the fitted rows (include/bmm_mcmc.h),
written from the formulas with np.log, np.logaddexp and scipy's logsumexp only -- nothing of the library's arithmetic.
The device kernels (csrc/kernels.hip.h, k_state_tables / k_score / k_score_generic / k_loo_finish / k_loo_reduce) compute
the same quantities; the tests hold them to each other.

For a state (labels z, statistics Nk, S, concentration alpha) and a fitted row i with label z_i:
  collapsed, dp   row i is taken out of the statistics (Nk' = Nk - [k = z_i], S'_kd = S_kd - x_id [k = z_i], N - 1 rows
                  remain) and ell_i is predictive_ref's log density of x_i for a chain fitted to those N - 1 rows
  explicit        ell_i = log sum_k pi_k prod_d theta_kd^x (1 - theta_kd)^(1-x); the labels do not enter

Every label but the row's own sees the statistics as they are, so the plain terms of all rows come from one call of
predictive_ref and only the own-label column is rewritten; tests/test_loo_ref.py holds that to the recount row by row.
"""
import numpy as np
from scipy.special import logsumexp

import predictive_ref as pref


def counting_terms(X, z, Nk, S, alpha, beta, gamma, sampler):
    """(N, Kc) log category terms of every fitted row with its own contribution removed.  z: 1-based labels, all in
    1..K; Nk (K,), S (K, P): the statistics of exactly those labels; sampler "collapsed" or "dp"."""
    X = np.asarray(X, dtype=np.float64)
    Nk = np.asarray(Nk, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    N, P = X.shape
    K = Nk.size
    k = np.asarray(z, dtype=np.int64) - 1
    if k.min() < 0 or k.max() >= K:
        raise ValueError("every row needs a label in 1..K")
    fn = pref.collapsed_terms if sampler == "collapsed" else pref.dp_terms
    T = fn(X, Nk, S, alpha, N - 1, beta, gamma)  # the labels a row does not hold: the statistics as they are
    n1 = Nk[k] - 1.0                             # the row's own label without it
    S1 = S[k] - X
    den = np.log(beta + gamma + n1)
    bern = (X * np.log(beta + S1) + (1.0 - X) * np.log(gamma + n1[:, None] - S1)).sum(axis=1) - P * den
    with np.errstate(divide="ignore"):
        w = np.log(n1 + alpha / K) if sampler == "collapsed" else np.log(n1)  # DP: a row that sat alone, log 0 = -inf
    T[np.arange(N), k] = (w - np.log(N - 1 + alpha)) + bern
    return T


def counting_ell(X, z, Nk, S, alpha, beta, gamma, sampler):
    """(N,) ell of the counting samplers"""
    return pref.logdens(counting_terms(X, z, Nk, S, alpha, beta, gamma, sampler))


def explicit_ell(X, pi, theta):
    """(N,) ell of the stick-breaking and full samplers"""
    return pref.logdens(pref.explicit_terms(X, pi, theta))


def recount_ell(X, z, K, alpha, beta, gamma, sampler, rows=None):
    """the definition, literally: for each row the statistics are recounted from the labels without it
    (predictive_ref.counts_from_labels) and predictive_ref scores the row for N - 1 fitted rows"""
    X = np.asarray(X)
    z = np.asarray(z)
    N = X.shape[0]
    fn = pref.collapsed_terms if sampler == "collapsed" else pref.dp_terms
    rows = range(N) if rows is None else rows
    out = []
    for i in rows:
        keep = np.arange(N) != i
        Nk, S = pref.counts_from_labels(X[keep], z[keep], K)
        out.append(pref.logdens(fn(X[i:i + 1], Nk, S, alpha, N - 1, beta, gamma))[0])
    return np.array(out)


def summary(trace, waic=False):
    """the outputs over the (S', N) trace of ell: per row log_cpo, ess, lppd, mean, var; lpml, min_ess, n_folded; with
    waic (the explicit samplers) p_waic and elpd_waic"""
    t = np.asarray(trace, dtype=np.float64)
    n = t.shape[0]
    lse1, lse2 = logsumexp(-t, axis=0), logsumexp(-2.0 * t, axis=0)
    out = {"log_cpo": np.log(n) - lse1, "ess": np.exp(2.0 * lse1 - lse2), "lppd": logsumexp(t, axis=0) - np.log(n),
           "mean": t.mean(axis=0), "var": t.var(axis=0, ddof=1) if n > 1 else np.full(t.shape[1], np.nan), "n_folded": n}
    out["lpml"] = float(out["log_cpo"].sum())
    out["min_ess"] = float(out["ess"].min())
    if waic:
        out["p_waic"] = float(out["var"].sum())
        out["elpd_waic"] = float(out["lppd"].sum() - out["p_waic"])
    return out
