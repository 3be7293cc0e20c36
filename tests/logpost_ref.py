"""The log joint of include/bmm_mcmc.h "log joint trace"  restated with SciPy in float64, from
the data and the labels -- no counts handed over, no fixed order of the sums: what tests/test_logpost_ref.py ties to
quantities independent of it, and what the host program and the device are held to within a rounding bound.

Labels are 0-based here.  `model` is one of "collapsed", "full" (the same prior), "dp", "stickbreaking", "allocation".
`bound_terms` also returns the magnitudes the bound of the GPU tests is built from: max(1, |v|) summed over every
lgamma / log value that enters a row, and the longest chain of additions of the stated order."""
import math

import numpy as np
from scipy.special import betaln, gammaln

LANES = 256  # kLjLanes of bmm_spec.h


def counts(X, z, K):
    X = np.asarray(X, dtype=np.int64)
    z = np.asarray(z, dtype=np.int64)
    Nk = np.bincount(z, minlength=K).astype(np.int64)
    S = np.zeros((K, X.shape[1]), dtype=np.int64)
    np.add.at(S, z, X)
    return Nk, S


def _cell(beta, gamma, n, s):
    return gammaln(beta + s) + gammaln(gamma + n - s) - gammaln(beta + gamma + n) - betaln(beta, gamma)


def log_lik_counts(Nk, S, N, beta, gamma, mask=None):
    Nk = np.asarray(Nk, dtype=np.int64)
    S = np.asarray(S, dtype=np.int64)
    P = S.shape[1]
    inc = np.ones(P, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    tot = 0.0
    for k in np.nonzero(Nk > 0)[0]:  # an empty label is skipped
        tot += float(np.sum(_cell(beta, gamma, float(Nk[k]), S[k, inc].astype(np.float64))))
    if mask is not None:
        T = S.sum(0)[~inc].astype(np.float64)
        tot += float(np.sum(_cell(beta, gamma, float(N), T)))  # the pooled term, once per excluded feature
    return tot


def log_prior_counts(model, Nk, N, alpha, k_open=None, log_prior_k=None):
    Nk = np.asarray(Nk, dtype=np.int64)
    K = len(Nk)
    used = Nk[Nk > 0].astype(np.float64)
    if model in ("collapsed", "full"):
        ak = alpha / K
        return float(gammaln(alpha) - gammaln(alpha + N) + np.sum(gammaln(ak + used) - gammaln(ak)))
    if model == "dp":
        return float(len(used) * math.log(alpha) + np.sum(gammaln(used)) + gammaln(alpha) - gammaln(alpha + N))
    if model == "stickbreaking":
        after = np.concatenate([np.cumsum(Nk[::-1])[::-1][1:], [0]]).astype(np.float64)
        k = np.arange(K - 1)
        return float(np.sum(betaln(1.0 + Nk[k], alpha + after[k]) - betaln(1.0, alpha)))
    if model == "allocation":
        assert np.all(Nk[k_open:] == 0)
        open_used = Nk[:k_open][Nk[:k_open] > 0].astype(np.float64)
        return float(log_prior_k[k_open - 1] + gammaln(k_open * alpha) - gammaln(k_open * alpha + N)
                     + np.sum(gammaln(alpha + open_used) - gammaln(alpha)))
    raise ValueError(model)


def log_hyper(alpha, sample_alpha, a, b, mask=None, rho=0.5):
    h = 0.0
    if sample_alpha:
        h += a * math.log(b) - gammaln(a) + (a - 1.0) * math.log(alpha) - b * alpha
    if mask is not None:
        m = np.asarray(mask).astype(bool)
        h += float(m.sum() * math.log(rho) + (~m).sum() * math.log(1.0 - rho))
    return float(h)


def rows_from_counts(model, Nk, S, N, alpha, beta, gamma, sample_alpha=False, a=1.0, b=1.0, k_open=None,
                     log_prior_k=None, mask=None, rho=0.5):
    ll = log_lik_counts(Nk, S, N, beta, gamma, mask)
    lp = log_prior_counts(model, Nk, N, alpha, k_open, log_prior_k)
    lh = log_hyper(alpha, sample_alpha, a, b, mask, rho)
    return np.array([ll, lp, lh, ll + lp + lh])


def log_joint(model, X, z, K, alpha, beta, gamma, **kw):
    """the four values of a state given as data and 0-based labels"""
    Nk, S = counts(X, z, K)
    return rows_from_counts(model, Nk, S, len(z), alpha, beta, gamma, **kw)


def bound_terms(model, Nk, S, N, alpha, beta, gamma, sample_alpha=False, a=1.0, b=1.0, k_open=None, log_prior_k=None,
                mask=None, rho=0.5):
    """(mag, depth): sum of max(1, |v|) over every lgamma / log value v entering the row, and the longest chain of
    additions in the stated order (a lane's cells, the tree, the labels, the head and the row's own three adds)"""
    Nk = np.asarray(Nk, dtype=np.int64)
    S = np.asarray(S, dtype=np.int64)
    K, P = S.shape
    inc = np.ones(P, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    vals = []
    lb0 = [gammaln(beta), gammaln(gamma), gammaln(beta + gamma)]
    top = K if k_open is None else k_open
    for k in range(top):
        n = float(Nk[k])
        if n <= 0:
            continue
        s = S[k, inc].astype(np.float64)
        vals += list(gammaln(beta + s)) + list(gammaln(gamma + n - s)) + [gammaln(beta + gamma + n)] * len(s) + lb0 * len(s)
    if mask is not None:
        T = S.sum(0)[~inc].astype(np.float64)
        vals += list(gammaln(beta + T)) + list(gammaln(gamma + N - T)) + [gammaln(beta + gamma + N)] * len(T) + lb0 * len(T)
    used = Nk[Nk > 0].astype(np.float64)
    if model in ("collapsed", "full"):
        ak = alpha / K
        vals += [gammaln(alpha), gammaln(alpha + N)] + list(gammaln(ak + used)) + [gammaln(ak)] * len(used)
    elif model == "dp":
        vals += [len(used) * math.log(alpha), gammaln(alpha), gammaln(alpha + N)] + list(gammaln(used))
    elif model == "stickbreaking":
        after = np.concatenate([np.cumsum(Nk[::-1])[::-1][1:], [0]]).astype(np.float64)
        for k in range(K - 1):
            x, y = 1.0 + Nk[k], alpha + after[k]
            vals += [gammaln(x), gammaln(y), gammaln(x + y), gammaln(1.0), gammaln(alpha), gammaln(1.0 + alpha)]
    else:
        ou = Nk[:k_open][Nk[:k_open] > 0].astype(np.float64)
        vals += [log_prior_k[k_open - 1], gammaln(k_open * alpha), gammaln(k_open * alpha + N)]
        vals += list(gammaln(alpha + ou)) + [gammaln(alpha)] * len(ou)
    if sample_alpha:
        vals += [a * math.log(b), gammaln(a), (a - 1.0) * math.log(alpha), b * alpha]
    if mask is not None:
        vals += [inc.sum() * math.log(rho), (~inc).sum() * math.log(1.0 - rho)]
    mag = float(np.sum(np.maximum(1.0, np.abs(np.asarray(vals, dtype=np.float64))))) if vals else 1.0
    depth = -(-P // LANES) + 8 + K + 1 + 8  # lane, tree, labels and the pooled term, the head / hyper / row adds
    return mag, depth


def partitions(n):
    """every set partition of range(n) as a restricted growth string (0-based labels in order of first appearance)"""
    def rec(prefix, top):
        if len(prefix) == n:
            yield tuple(prefix)
            return
        for v in range(top + 1):
            yield from rec(prefix + [v], max(top, v + 1))
    yield from rec([], 0)
