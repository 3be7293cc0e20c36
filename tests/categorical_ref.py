"""Categorical features for the collapsed and the DP sampler (include/bmm_mcmc.h "categorical features", DESIGN.md
section 30), restated in NumPy with scipy's gammaln.

Labels are 0-based here.  `levels` is the raw vector the library takes: 1 is a binary feature in one column under
Beta(beta, gamma), L >= 2 a block of L neighbouring one-hot columns under a symmetric Dirichlet(beta, ..., beta).
expand turns an N x F matrix of level indices into the one-hot columns and the per-column bytes the table build reads,
z_conditional is the allocation conditional of either sampler against counts frozen at `z` with the row's own
contribution removed (in the shape of feature_select_ref.z_conditional), exact_posterior the CRP x Dirichlet-multinomial
posterior over every partition of a small set, sequential_dp a one-row-at-a-time sampler of that posterior."""
import numpy as np
from scipy.special import gammaln

import split_merge_ref as smr


def column_map(levels):
    """(first column of every feature, lev: per column 0 for a Bernoulli column, else the L of its block)"""
    levels = np.asarray(levels, dtype=np.int64)
    assert levels.ndim == 1 and (levels >= 1).all()
    first = np.concatenate(([0], np.cumsum(levels)))[:-1]
    lev = np.concatenate([np.full(L, 0 if L == 1 else L, dtype=np.uint8) for L in levels])
    return first, lev


def expand(Xcat, levels):
    """N x F level indices (a feature of 1 "level" holds its 0/1 value) -> (N x P int32 column-major 0/1 matrix, lev)"""
    Xcat = np.asarray(Xcat, dtype=np.int64)
    first, lev = column_map(levels)
    assert Xcat.ndim == 2 and Xcat.shape[1] == len(levels)
    X = np.zeros((len(Xcat), len(lev)), dtype=np.int32, order="F")
    rows = np.arange(len(Xcat))
    for j, L in enumerate(levels):
        if L == 1:
            assert np.isin(Xcat[:, j], (0, 1)).all()
            X[:, first[j]] = Xcat[:, j]
        else:
            assert (Xcat[:, j] >= 0).all() and (Xcat[:, j] < L).all()
            X[rows, first[j] + Xcat[:, j]] = 1
    return X, lev


def draw(N, levels, seed, comps=3):
    """N rows of level indices from a mixture of `comps` components, one Dirichlet(0.6) profile per component and feature"""
    rng = np.random.default_rng(seed)
    comp = rng.integers(comps, size=N)
    X = np.zeros((N, len(levels)), dtype=np.int64)
    for j, L in enumerate(levels):
        m = max(L, 2)
        prof = rng.dirichlet(np.full(m, 0.6), size=comps)
        X[:, j] = (rng.random(N)[:, None] > np.cumsum(prof, axis=1)[comp]).sum(axis=1).clip(0, m - 1)
    return X, comp


def counts(X, z, K):
    X = np.asarray(X, dtype=np.int64)
    z = np.asarray(z)
    Nk = np.bincount(z, minlength=K).astype(np.int64)
    S = np.zeros((K, X.shape[1]), dtype=np.int64)
    np.add.at(S, z, X)
    return Nk, S


def z_conditional(X1h, z, K, alpha, beta, gamma, lev, sampler, rows=None):
    """The normalised allocation conditional of every row in `rows` (default all), by label (K columns), against the
    counts of `z` with the row itself removed.  A Bernoulli column (lev = 0) gives log(beta + s) or log(gamma + n - s)
    less log(beta + gamma + n); a column of a block of L gives log(beta + s) - log(L beta + n) where the row has its 1
    and nothing elsewhere.  The weights, the new cluster's label and the unseated rows: as feature_select_ref.z_conditional;
    the new cluster's likelihood is beta / (beta + gamma) per Bernoulli column and 1 / L per block."""
    X = np.asarray(X1h, dtype=np.int64)
    z = np.asarray(z)
    lev = np.asarray(lev, dtype=np.int64)
    bern, oh = lev == 0, lev > 0
    seated = z >= 0
    Nk, S = counts(X[seated], z[seated], K)
    rows = np.arange(len(X)) if rows is None else np.asarray(rows)
    x = X[rows].astype(np.float64)
    zr = z[rows]
    n, s = Nk.astype(np.float64), S.astype(np.float64)
    xb, xo, sb, so_, Lo = x[:, bern], x[:, oh], s[:, bern], s[:, oh], lev[oh].astype(np.float64)
    ak = alpha / K if sampler == "collapsed" else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ll = xb @ np.log(beta + sb).T + (1.0 - xb) @ np.log(gamma + n[:, None] - sb).T - bern.sum() * np.log(beta + gamma + n)[None, :]
        ll = ll + xo @ (np.log(beta + so_) - np.log(Lo[None, :] * beta + n[:, None])).T
        lw = np.where(n[None, :] > 0, np.log(n + ak)[None, :] + ll, -np.inf)
        own = np.flatnonzero(zr >= 0)
        zo = zr[own]
        no = n[zo] - 1.0
        sbo, soo = sb[zo] - xb[own], so_[zo] - xo[own]
        llo = np.sum(np.where(xb[own] == 1, np.log(beta + sbo), np.log(gamma + no[:, None] - sbo)), axis=1) - bern.sum() * np.log(beta + gamma + no)
        llo = llo + np.sum(np.where(xo[own] == 1, np.log(beta + soo) - np.log(Lo[None, :] * beta + no[:, None]), 0.0), axis=1)
        lw[own, zo] = np.where(no > 0, np.log(no + ak) + llo, -np.inf)
    if sampler == "dp":
        # one term per block: a block of L has L columns
        lnew = np.log(alpha) + bern.sum() * (np.log(beta) - np.log(beta + gamma)) + float(np.sum((np.log(beta) - np.log(Lo * beta)) / Lo))
        for r in range(len(rows)):
            free = np.flatnonzero(lw[r] == -np.inf)
            if len(free):
                lw[r, free[0]] = lnew
    w = np.exp(lw - lw.max(axis=1, keepdims=True))
    return w / w.sum(axis=1, keepdims=True)


# ---------------------------------------------------------------- the exact posterior of a small data set (DP)
def log_marginal(Xcat, levels, rows, beta, gamma):
    """log p(the rows' cells | they share a cluster), the level probabilities integrated out"""
    lw, n = 0.0, len(rows)
    for j, L in enumerate(levels):
        if L == 1:
            s = int(Xcat[rows, j].sum())
            lw += (gammaln(beta + s) + gammaln(gamma + n - s) - gammaln(beta + gamma + n)) - (gammaln(beta) + gammaln(gamma) - gammaln(beta + gamma))
        else:
            c = np.bincount(Xcat[rows, j], minlength=L)
            lw += (gammaln(L * beta) - gammaln(L * beta + n)) + float(np.sum(gammaln(beta + c) - gammaln(beta)))
    return lw


def exact_posterior(Xcat, levels, alpha, beta, gamma=None):
    """CRP(alpha) prior x Dirichlet-multinomial (Beta-Bernoulli for a feature of 1) marginal likelihood over every
    partition of the rows (877 for seven), by brute force.  gamma: of the binary features, default beta."""
    Xcat = np.asarray(Xcat, dtype=np.int64)
    gamma = beta if gamma is None else gamma
    parts = smr.partitions(len(Xcat))
    logw = []
    for z in parts:
        z = np.asarray(z)
        lw = 0.0
        for k in range(z.max() + 1):
            rows = np.flatnonzero(z == k)
            lw += np.log(alpha) + gammaln(len(rows)) + log_marginal(Xcat, levels, rows, beta, gamma)
        logw.append(lw)
    w = np.exp(np.asarray(logw) - np.max(logw))
    return parts, w / w.sum()


def sequential_dp(Xcat, levels, alpha, beta, gamma, sweeps, rng, K=None):
    """The DP sampler one row at a time (batch = 1) on a NumPy generator, every row unseated at the start: the canonical
    partition after every sweep.  The conditional is z_conditional's, kept in running counts."""
    X, lev = expand(Xcat, levels)
    X = np.asarray(X, dtype=np.int64)
    N, P = X.shape
    K = N + 1 if K is None else K
    lev = lev.astype(np.float64)
    bern = lev == 0
    nb = float(bern.sum())
    lnew = alpha * (beta / (beta + gamma)) ** nb * float(np.prod((1.0 / lev[~bern]) ** (1.0 / lev[~bern])))
    z = np.full(N, -1)
    Nk, S = np.zeros(K), np.zeros((K, P))
    is1 = X == 1
    visited = []
    for _ in range(sweeps):
        u = rng.random(N)
        for i in range(N):
            if z[i] >= 0:
                Nk[z[i]] -= 1.0
                S[z[i]] -= X[i]
            num = np.where(is1[i][None, :], beta + S, np.where(bern[None, :], gamma + Nk[:, None] - S, 1.0)).prod(axis=1)
            den = (beta + gamma + Nk) ** nb * np.where(is1[i] & ~bern, lev[None, :] * beta + Nk[:, None], 1.0).prod(axis=1)
            w = np.where(Nk > 0, Nk * num / den, 0.0)
            free = np.flatnonzero(Nk == 0)
            if len(free):
                w[free[0]] = lnew
            cdf = np.cumsum(w)
            k = min(int(np.searchsorted(cdf, u[i] * cdf[-1], side="right")), K - 1)
            z[i] = k
            Nk[k] += 1.0
            S[k] += X[i]
        visited.append(smr.canon(z))
    return visited


# ---------------------------------------------------------------- what check_against_enumeration compares
def compared_quantities(parts, weights):
    """the exact values split_merge_checks.check_against_enumeration holds a chain to, with the indicator of each over
    the partitions: the cluster-count distribution, every co-clustering probability (the likeliest partitions are left
    to the check itself: which twenty they are depends on the posterior)"""
    Z = np.array(parts)
    N = Z.shape[1]
    nclus = Z.max(axis=1) + 1
    feats = [(nclus == k).astype(float) for k in range(1, N + 1)]
    feats += [(Z[:, i] == Z[:, j]).astype(float) for i in range(N) for j in range(i + 1, N)]
    F = np.array(feats)
    return F, F @ np.asarray(weights)


def margins(visited, parts, F, exact, n_batches=100):
    """4 standard errors of every compared quantity of this chain, by the rule of check_against_enumeration"""
    index = {s: k for k, s in enumerate(parts)}
    ids = np.array([index[s] for s in visited])
    n = len(ids) // n_batches * n_batches
    ids = ids[:n]
    out = []
    for f, p in zip(F, exact):
        bm = f[ids].reshape(n_batches, -1).mean(axis=1)
        out.append(4.0 * max(bm.std(ddof=1) / np.sqrt(n_batches), np.sqrt(max(p * (1.0 - p), 0.0) / n)))
    return np.array(out)


def seven_rows():
    """Seven rows over levels [3, 4, 1] on which the categorical posterior and the Bernoulli posterior of the same
    one-hot columns are far apart (tests/test_categorical_ref.py holds that)"""
    return np.array(SEVEN, dtype=np.int64), [3, 4, 1]


SEVEN = [[0, 0, 1], [0, 1, 1], [0, 0, 0], [1, 2, 1], [1, 3, 0], [2, 2, 0], [1, 1, 1]]
