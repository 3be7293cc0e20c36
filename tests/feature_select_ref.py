"""Feature selection for the counting samplers (include/bmm_mcmc.h "feature selection"),
restated in NumPy with scipy's gammaln and the Philox of split_merge_ref.py.

Labels are 0-based here.  gamma_logit / gamma_step are the indicator step, z_conditional the masked allocation
conditional of either sampler against counts frozen at `z` with the row's own contribution removed (what the device
computes at batch = N, and the exact sequential conditional at batch = 1), joint_posterior the brute-force posterior
over (partition, mask) of the DP model, sweep_matrix the exact transition matrix of one restated sweep."""
import itertools

import numpy as np
from scipy.special import betaln, gammaln

import split_merge_ref as smr

STREAM = 9  # kStreamFeatureSelect


def fs_uniform(seed, d, sweep):
    r = smr.philox4x32_10((d, 0, sweep, STREAM), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return smr.u01(r[0], r[1])


def counts(X, z, K):
    X = np.asarray(X, dtype=np.int64)
    z = np.asarray(z)
    Nk = np.bincount(z, minlength=K).astype(np.int64)
    S = np.zeros((K, X.shape[1]), dtype=np.int64)
    np.add.at(S, z, X)
    return Nk, S


def gamma_logit(Nk, S, beta, gamma, rho, with_terms=False):
    """Lambda_d for every feature from the folded counts; empty clusters are skipped.  with_terms: also the sum of the
    magnitudes of every lgamma that enters Lambda_d and their number (for an error bound)."""
    Nk = np.asarray(Nk, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    used = Nk > 0
    n, s = Nk[used][:, None], S[used]
    N, T = Nk.sum(), S.sum(axis=0)
    lb0 = betaln(beta, gamma)
    lam = np.log(rho) - np.log1p(-rho) + np.sum(betaln(beta + s, gamma + n - s) - lb0, axis=0) - (betaln(beta + T, gamma + N - T) - lb0)
    if not with_terms:
        return lam
    mag = (np.abs(gammaln(beta + s)) + np.abs(gammaln(gamma + n - s)) + np.abs(gammaln(beta + gamma + n)) + abs(lb0) * np.ones_like(s)).sum(axis=0)
    mag = mag + np.abs(gammaln(beta + T)) + np.abs(gammaln(gamma + N - T)) + abs(gammaln(beta + gamma + N)) + abs(lb0)
    mag = mag + abs(np.log(rho)) + abs(np.log1p(-rho)) + 3.0 * (abs(gammaln(beta)) + abs(gammaln(gamma)) + abs(gammaln(beta + gamma)))
    n_terms = 4 * int(used.sum()) + 4 + 2 + 3
    return lam, mag, n_terms


def gamma_prob(lam):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(lam)))


def gamma_step(Nk, S, beta, gamma, rho, seed, sweep):
    lam = gamma_logit(Nk, S, beta, gamma, rho)
    p = gamma_prob(lam)
    u = np.array([fs_uniform(seed, d, sweep) for d in range(len(lam))])
    return lam, p, u, (u < p).astype(np.uint8)


def z_conditional(X, z, K, alpha, beta, gamma, mask, sampler, rows=None):
    """The normalised allocation conditional of every row in `rows` (default all), by label (K columns), against the
    counts of `z` with the row itself removed, the product over the features with mask = 1 only.
    collapsed: weight (n_k' + alpha/K) for a label still in use with the row removed, 0 for an emptied or empty one
    (the sampler's rule); dp: n_k' for a used label and alpha * prod_d beta / (beta + gamma) over the included features
    for the new cluster, filed under the label it would open: the smallest unused one, the row's own when removing it
    has just freed a smaller one; no unused label: the new-cluster mass is dropped.  z = -1: an unseated row (nothing
    to remove)."""
    X = np.asarray(X, dtype=np.int64)
    z = np.asarray(z)
    inc = np.flatnonzero(np.asarray(mask))
    seated = z >= 0
    Nk, S = counts(X[seated], z[seated], K)
    rows = np.arange(len(X)) if rows is None else np.asarray(rows)
    x = X[rows][:, inc].astype(np.float64)
    zr = z[rows]
    n, s = Nk.astype(np.float64), S[:, inc].astype(np.float64)
    ak = alpha / K if sampler == "collapsed" else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ll = x @ np.log(beta + s).T + (1.0 - x) @ np.log(gamma + n[:, None] - s).T - len(inc) * np.log(beta + gamma + n)[None, :]
        lw = np.where(n[None, :] > 0, np.log(n + ak)[None, :] + ll, -np.inf)
        # the row's own label: one row fewer, its own ones taken out
        own = np.flatnonzero(zr >= 0)
        zo = zr[own]
        no, so = n[zo] - 1.0, s[zo] - x[own]
        llo = np.sum(np.where(x[own] == 1, np.log(beta + so), np.log(gamma + no[:, None] - so)), axis=1) - len(inc) * np.log(beta + gamma + no)
        lw[own, zo] = np.where(no > 0, np.log(no + ak) + llo, -np.inf)
    if sampler == "dp":
        lnew = np.log(alpha) + len(inc) * (np.log(beta) - np.log(beta + gamma))
        for r in range(len(rows)):
            free = np.flatnonzero(lw[r] == -np.inf)  # unused, or just emptied by taking the row out
            if len(free):
                lw[r, free[0]] = lnew
    w = np.exp(lw - lw.max(axis=1, keepdims=True))
    return w / w.sum(axis=1, keepdims=True)


def restated_chain(X, z0, K, alpha, beta, gamma, rho, sweeps, rng, batch):
    """the finite sampler with a gamma-step behind every sweep, on a NumPy generator: batches of `batch` rows against
    counts frozen at batch start.  Returns the (sweeps, P) indicators and the final labels."""
    X = np.asarray(X, dtype=np.int64)
    z = np.array(z0)
    mask = np.ones(X.shape[1], dtype=np.uint8)
    trace = np.zeros((sweeps, X.shape[1]), dtype=np.uint8)
    for t in range(sweeps):
        for lo in range(0, len(X), batch):
            rows = np.arange(lo, min(lo + batch, len(X)))
            cond = z_conditional(X, z, K, alpha, beta, gamma, mask, "collapsed", rows=rows)
            cdf = np.cumsum(cond, axis=1)
            z[rows] = np.minimum((rng.random(len(rows))[:, None] * cdf[:, -1:] >= cdf).sum(axis=1), K - 1)
        Nk, S = counts(X, z, K)
        p = gamma_prob(gamma_logit(Nk, S, beta, gamma, rho))
        mask = (rng.random(len(p)) < p).astype(np.uint8)
        trace[t] = mask
    return trace, z


# ---------------------------------------------------------------- the exact joint posterior of a small data set (DP)
def masks(P):
    return [np.array(m, dtype=np.uint8) for m in itertools.product((0, 1), repeat=P)]


def log_joint(X, z, mask, alpha, beta, gamma, rho):
    """log p(z, mask, X) up to a constant: CRP(alpha) x Bernoulli(rho)^P x the marginal likelihood, theta integrated out"""
    X = np.asarray(X, dtype=np.int64)
    z = np.asarray(z)
    mask = np.asarray(mask).astype(bool)
    lw = float(np.sum(np.where(mask, np.log(rho), np.log1p(-rho))))
    lb0 = betaln(beta, gamma)
    for k in range(z.max() + 1):
        rows = np.flatnonzero(z == k)
        n, s = len(rows), X[rows][:, mask].sum(axis=0)
        lw += np.log(alpha) + gammaln(n) + float(np.sum(betaln(beta + s, gamma + n - s) - lb0))
    T = X[:, ~mask].sum(axis=0)
    lw += float(np.sum(betaln(beta + T, gamma + len(X) - T) - lb0))
    return lw


def joint_posterior(X, alpha, beta, gamma, rho):
    """(partitions, masks, W) with W[s, m] the posterior probability of partition s and mask m"""
    parts = smr.partitions(len(X))
    ms = masks(np.asarray(X).shape[1])
    L = np.array([[log_joint(X, z, m, alpha, beta, gamma, rho) for m in ms] for z in parts])
    W = np.exp(L - L.max())
    return parts, ms, W / W.sum()


def log_joint_finite(X, z, mask, K, alpha, beta, gamma, rho):
    """the same for the finite model: labels z in 0 .. K-1, symmetric Dirichlet(alpha / K) weights integrated out"""
    X = np.asarray(X, dtype=np.int64)
    z = np.asarray(z)
    mask = np.asarray(mask).astype(bool)
    lw = float(np.sum(np.where(mask, np.log(rho), np.log1p(-rho))))
    lb0 = betaln(beta, gamma)
    for k in range(K):
        rows = np.flatnonzero(z == k)
        n, s = len(rows), X[rows][:, mask].sum(axis=0)
        lw += gammaln(n + alpha / K) + float(np.sum(betaln(beta + s, gamma + n - s) - lb0))
    T = X[:, ~mask].sum(axis=0)
    return lw + float(np.sum(betaln(beta + T, gamma + len(X) - T) - lb0))


def sweep_matrix(X, parts, ms, alpha, beta, gamma, rho, K):
    """The transition matrix over (partition, mask) states of one restated DP sweep at batch 1: a sequential scan of
    z_conditional under the current mask, then the gamma-step from the counts of the new partition."""
    X = np.asarray(X, dtype=np.int64)
    N = len(X)
    index = {s: k for k, s in enumerate(parts)}
    n_s, n_m = len(parts), len(ms)
    # the scan: partition -> distribution over partitions, per mask
    scan = np.zeros((n_m, n_s, n_s))
    for mi, m in enumerate(ms):
        for si, z0 in enumerate(parts):
            dist = {tuple(z0): 1.0}
            for i in range(N):
                nxt = {}
                for zt, pr in dist.items():
                    z = np.array(zt)
                    cond = z_conditional(X, z, K, alpha, beta, gamma, m, "dp", rows=[i])[0]
                    for k in np.flatnonzero(cond > 0):
                        z2 = z.copy()
                        z2[i] = k
                        key = tuple(z2)
                        nxt[key] = nxt.get(key, 0.0) + pr * cond[k]
                dist = {}
                for zt, pr in nxt.items():  # states that are the same partition merge: the conditional is label-invariant
                    c = smr.canon(zt)
                    dist[c] = dist.get(c, 0.0) + pr
            for zt, pr in dist.items():
                scan[mi, si, index[zt]] += pr
    # the gamma-step: partition -> distribution over masks
    gam = np.zeros((n_s, n_m))
    for si, z in enumerate(parts):
        z = np.asarray(z)
        Nk, S = counts(X, z, z.max() + 1)
        p = gamma_prob(gamma_logit(Nk, S, beta, gamma, rho))
        for mi, m in enumerate(ms):
            gam[si, mi] = np.prod(np.where(m == 1, p, 1.0 - p))
    T = np.zeros((n_s * n_m, n_s * n_m))
    for mi in range(n_m):
        for si in range(n_s):
            T[si * n_m + mi] = (scan[mi, si][:, None] * gam).reshape(-1)
    return T
