"""NumPy restatement of the per-state posterior predictive density of a new binary row (include/bmm_mcmc.h,
DESIGN.md section 12), written from the three formulas with np.log and np.logaddexp only -- nothing of the
library's arithmetic (no group tables, no max-shift by hand, no table exponential).  The device kernels
(csrc/kernels.hip.h, k_state_tables / k_score / k_score_generic / k_predict_finish) compute the same
quantities; the tests hold them to each other.

For a state s and a new row x of P binary features:
  collapsed  (Nk, S, alpha, N)   sum over ALL K labels of
                                 (Nk + alpha/K)/(N + alpha) * prod_d (beta + S_kd)^x_d (gamma + Nk - S_kd)^(1-x_d) / (beta + gamma + Nk)
                                 -- an empty label keeps its prior weight and the prior Bernoulli terms
  dp         (Nk, S, alpha, N)   sum over used labels of Nk/(N + alpha) * (the same product), plus the new cluster:
                                 alpha/(N + alpha) * prod_d beta^x_d gamma^(1-x_d) / (beta + gamma)
  explicit   (pi, theta)         sum_k pi_k prod_d theta_kd^x_d (1 - theta_kd)^(1-x_d)

Every function returns the (M, Kc) matrix of log category terms; `logdens` reduces it, `resp` normalises it, `lppd`
averages densities over states.  Nk is (K,), S is (K, P) (counts of ones), theta is (K, P), Xnew is (M, P).
"""
import numpy as np


def _bernoulli_logterms(Xnew, l1, l0):
    """(M, K): sum_d x_d l1[k, d] + (1 - x_d) l0[k, d]"""
    X = np.asarray(Xnew, dtype=np.float64)
    return X @ l1.T + (1.0 - X) @ l0.T


def _count_terms(Xnew, Nk, S, beta, gamma):
    Nk = np.asarray(Nk, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    den = np.log(beta + gamma + Nk)[:, None]
    return _bernoulli_logterms(Xnew, np.log(beta + S) - den, np.log(gamma + Nk[:, None] - S) - den)


def collapsed_terms(Xnew, Nk, S, alpha, N, beta, gamma):
    """log of the K category terms of the finite collapsed sampler's predictive, (M, K)"""
    Nk = np.asarray(Nk, dtype=np.float64)
    K = Nk.size
    return (np.log(Nk + alpha / K) - np.log(N + alpha))[None, :] + _count_terms(Xnew, Nk, S, beta, gamma)


def dp_terms(Xnew, Nk, S, alpha, N, beta, gamma):
    """log of the maxK label terms (-inf for an unused label) and then the new-cluster term, (M, maxK + 1)"""
    Nk = np.asarray(Nk, dtype=np.float64)
    X = np.asarray(Xnew, dtype=np.float64)
    with np.errstate(divide="ignore"):
        w = np.log(Nk) - np.log(N + alpha)  # log 0 = -inf: an unused label has no weight
    labels = w[None, :] + _count_terms(Xnew, Nk, S, beta, gamma)
    new = (np.log(alpha) - np.log(N + alpha)) + (X * np.log(beta) + (1.0 - X) * np.log(gamma) - np.log(beta + gamma)).sum(axis=1)
    return np.concatenate([labels, new[:, None]], axis=1)


def explicit_terms(Xnew, pi, theta):
    """log of the K category terms for explicit (pi, theta): stick-breaking and full, (M, K)"""
    pi = np.asarray(pi, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.log(pi)[None, :] + _bernoulli_logterms(Xnew, np.log(theta), np.log(1.0 - theta))


def logdens(terms):
    """log p(x_m | s) from the (M, Kc) log category terms: np.logaddexp over the categories, in order"""
    out = terms[:, 0].copy()
    for k in range(1, terms.shape[1]):
        out = np.logaddexp(out, terms[:, k])
    return out


def resp(terms):
    """the normalised category weights, (M, Kc); rows sum to 1"""
    return np.exp(terms - logdens(terms)[:, None])


def lppd(trace):
    """log((1/S) sum_s p(x_m | s)) from the (S, M) trace of log densities"""
    trace = np.asarray(trace, dtype=np.float64)
    out = trace[0].copy()
    for s in range(1, trace.shape[0]):
        out = np.logaddexp(out, trace[s])
    return out - np.log(trace.shape[0])


def counts_from_labels(X, z, K):
    """(Nk, S) of 1-based labels z over the rows of X; labels outside 1..K (NA) are skipped"""
    X = np.asarray(X)
    z = np.asarray(z)
    Nk = np.zeros(K, dtype=np.int64)
    S = np.zeros((K, X.shape[1]), dtype=np.int64)
    for k in range(K):
        rows = z == k + 1
        Nk[k] = rows.sum()
        S[k] = X[rows].sum(axis=0)
    return Nk, S


def all_rows(P):
    """every one of the 2^P binary rows, (2^P, P)"""
    return ((np.arange(1 << P)[:, None] >> np.arange(P)[None, :]) & 1).astype(np.int32)
