"""Parallel tempering for the counting samplers (include/bmm_mcmc.h "parallel tempering"),
restated in NumPy with scipy's betaln, the oracle's Philox4x32-10 and the oracle's weight exponential.

Labels are 0-based here.  z_conditional is the tempered allocation conditional of either sampler against counts frozen
at `z` with the row's own contribution removed (what the device computes at batch = N, and the exact sequential
conditional at batch = 1): every per-feature log-predictive term times b, the allocation prior untouched.  exchange_*
restate the exchange rule and its uniform; restated_ladder is a whole ladder on a NumPy generator for small N;
scan_matrix / exchange_matrix are the exact transition matrices of the tempered one-row scan over the partitions of a
small data set and of one exchange point on the product space of two rungs; product_scan / product_exchange apply the
same two to a joint distribution over any number of rungs without forming the matrix.  The constants and the cases of
the device tests (ladders, swap shapes, table edges, the replayed run) are chosen here and checked on the CPU in
tests/test_temper_ref.py."""
import os
import sys

import numpy as np
from scipy.special import betaln, gammaln

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle  # noqa: E402

import feature_select_ref as fsr  # noqa: E402
import split_merge_ref as smr  # noqa: E402

STREAM = 14  # kStreamTemper

# the exchange-decision test (tests/test_gpu_temper.py section 3): N, P, K, the data's seed and the powers of ladders
# of two, four, five and eight rungs, chosen so that in 60 exchange points with one sweep between them every pair both
# accepts and rejects at least EXCHANGE_FLOOR of its proposals (tests/test_temper_ref.py holds the restated ladder to that)
EXCHANGE_SHAPE = (300, 8, 4)
EXCHANGE_THETAS = (0.5,)  # one component: the posterior over allocations is diffuse and log_lik moves smoothly with the power
EXCHANGE_DATA_SEED = 3
# (log_lik of this shape falls by about 300 per unit of power near 1 and spreads by about 15: steps of 0.03 to 0.04 at the top,
# wider further down, put d near -1)
EXCHANGE_POWERS = {2: (1.0, 0.97), 4: (1.0, 0.96, 0.915, 0.85), 5: (1.0, 0.96, 0.915, 0.85, 0.765),
                   8: (1.0, 0.96, 0.915, 0.85, 0.765, 0.66, 0.53, 0.38)}
EXCHANGE_STEPS = 60
# what every pair must both accept and reject at least, on the device and in the restatement: the ladders of four and
# of eight (an even number of rungs above two: both end rungs idle at the odd points; the full ladder: four slices of
# the exchange grid at the even points, three at the odd) are held to 3, which the restatement clears with room (its
# worst count over three generator seeds is 7 of 30)
EXCHANGE_FLOOR = {2: 10, 4: 3, 5: 10, 8: 3}

# the run a hand-built ladder replays row by row (tests/test_gpu_temper_ladders.py): N = 301 puts three of four rows of
# the label trace off a 16-byte boundary; powers in steps of 0.05, at which the restated ladder accepts 10 to 16 of
# rung 0's 20 proposals in 39 sweeps and rejects the rest, either sampler (tests/test_temper_ref.py)
REPLAY_SHAPE = (301, 33, 5)
REPLAY_THETAS = (0.3, 0.5, 0.7)
REPLAY_DATA_SEED = 4
REPLAY_POWERS = {3: (1.0, 0.95, 0.9), 4: (1.0, 0.95, 0.9, 0.85), 8: (1.0, 0.95, 0.9, 0.85, 0.8, 0.75, 0.7, 0.65)}
REPLAY_MAXK = 12    # of the DP runs
REPLAY_SWEEPS = 40  # nsamples of the run: sweeps 1 .. 39
REPLAY_BATCH = 64
REPLAY_SEED = 21

# the shapes at which temper_swap leaves its first trip and its 16-byte body: K = 37 and K * P = 1369 leave a scalar
# tail of one, S and the eight delta replicas take several passes of a one-block grid; N = 300 001 takes a second pass
# of the 256-block grid and leaves one label to the tail
SWAP_SHAPES = ((64, 37, 37), (300_001, 8, 4))


def swap_case(N, P, K):
    """(X, z_a, z_b), labels 1-based: two allocations that differ in every row -- so in the last label, the scalar
    tail of N = 300 001 -- and in the last cell of Nk and of S: z_a seats the first half of the rows, whose last
    column is all ones, under label K and the rest under label 1; z_b uses labels 2 .. K - 1 only."""
    rng = np.random.default_rng(N + 7 * P + K)
    half = N // 2
    X = (rng.random((N, P)) < np.where(np.arange(N) < half, 0.9, 0.1)[:, None]).astype(np.int32)
    X[:half, P - 1] = 1
    z_a = np.where(np.arange(N) < half, K, 1).astype(np.int32)
    z_b = rng.integers(2, K, N).astype(np.int32)
    return np.asfortranarray(X), z_a, z_b


# the table edges of the tempered build on purpose (n = 0, n = 1, n = 2, s = 0, s = n): labels 0-based
EDGE_SHAPE = (300, 37, 6)
EDGE_EMPTY, EDGE_SINGLE, EDGE_PAIR = 1, 2, 3
EDGE_ROWS = {"single": (5,), "pair": (10, 11)}


def edge_case():
    """(X, z): column 0 all zeros, column 1 all ones; label 1 empty, label 2 holds row 5 alone, label 3 rows 10 and 11,
    labels 0, 4 and 5 share the rest"""
    N, P, K = EDGE_SHAPE
    X, _ = mixture(N, P, [0.2, 0.5, 0.8], 3)
    X = np.array(X)
    X[:, 0] = 0
    X[:, 1] = 1
    z = np.array([0, 4, 5])[np.random.default_rng(9).integers(0, 3, N)]
    z[list(EDGE_ROWS["single"])] = EDGE_SINGLE
    z[list(EDGE_ROWS["pair"])] = EDGE_PAIR
    return np.asfortranarray(X.astype(np.int32)), z


def mixture(N, P, thetas, seed):
    rng = np.random.default_rng(seed)
    comp = rng.integers(len(thetas), size=N)
    X = (rng.random((N, P)) < np.asarray(thetas)[comp][:, None]).astype(np.int32)
    return np.asfortranarray(X), comp


# ---------------------------------------------------------------- the exchange rule
def exchange_uniform(seed, r, t):
    """u of pair r at exchange point t: the 52-bit uniform of the first two words of the block at counter
    (r, 0, t, STREAM) under the ladder's seed"""
    w = oracle.philox4x32_10((r, 0, t, STREAM), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return float(oracle.lib().oracle_u52(w[0], w[1]))


def log_ratio(b_r, b_r1, L_r, L_r1):
    return (np.float64(b_r) - np.float64(b_r1)) * (np.float64(L_r1) - np.float64(L_r))


def accepts(d, u):
    """accepted iff d >= 0 or u < expw(d); a NaN d rejects"""
    if d >= 0.0:
        return True
    if not d < 0.0:
        return False
    return bool(u < oracle.expw_array(np.array([d]))[0])


def proposed_pairs(R, t):
    return list(range(t % 2, R - 1, 2))


# ---------------------------------------------------------------- the tempered conditional
def z_conditional(X, z, K, alpha, beta, gamma, b, sampler, rows=None):
    """The normalised tempered conditional of every row in `rows` (default all), by label (K columns): the rules of
    feature_select_ref.z_conditional with all features in and the Bernoulli terms times b.  dp: the new-cluster option,
    alpha * (prod_d beta / (beta + gamma))^b, is filed under the label it would open."""
    X = np.asarray(X, dtype=np.int64)
    z = np.asarray(z)
    P = X.shape[1]
    seated = z >= 0
    Nk, S = fsr.counts(X[seated], z[seated], K)
    rows = np.arange(len(X)) if rows is None else np.asarray(rows)
    x = X[rows].astype(np.float64)
    zr = z[rows]
    n, s = Nk.astype(np.float64), S.astype(np.float64)
    ak = alpha / K if sampler == "collapsed" else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ll = x @ np.log(beta + s).T + (1.0 - x) @ np.log(gamma + n[:, None] - s).T - P * np.log(beta + gamma + n)[None, :]
        lw = np.where(n[None, :] > 0, np.log(n + ak)[None, :] + b * ll, -np.inf)
        own = np.flatnonzero(zr >= 0)
        zo = zr[own]
        no, so = n[zo] - 1.0, s[zo] - x[own]
        llo = np.sum(np.where(x[own] == 1, np.log(beta + so), np.log(gamma + no[:, None] - so)), axis=1) - P * np.log(beta + gamma + no)
        lw[own, zo] = np.where(no > 0, np.log(no + ak) + b * llo, -np.inf)
    if sampler == "dp":
        lnew = np.log(alpha) + b * (P * (np.log(beta) - np.log(beta + gamma)))
        for r in range(len(rows)):
            free = np.flatnonzero(lw[r] == -np.inf)  # unused, or just emptied by taking the row out
            if len(free):
                lw[r, free[0]] = lnew
    w = np.exp(lw - lw.max(axis=1, keepdims=True))
    return w / w.sum(axis=1, keepdims=True)


def log_lik(X, z, beta, gamma):
    """log p(x | z), theta integrated out: the sum over the labels in use and the features"""
    X = np.asarray(X, dtype=np.int64)
    z = np.asarray(z)
    lb0 = betaln(beta, gamma)
    total = 0.0
    for k in np.unique(z[z >= 0]):
        rows = np.flatnonzero(z == k)
        n, s = len(rows), X[rows].sum(axis=0)
        total += float(np.sum(betaln(beta + s, gamma + n - s) - lb0))
    return total


# ---------------------------------------------------------------- a whole ladder, restated
def restated_sweep(X, z, K, alpha, beta, gamma, b, sampler, rng, batch):
    for lo in range(0, len(X), batch):
        rows = np.arange(lo, min(lo + batch, len(X)))
        cond = z_conditional(X, z, K, alpha, beta, gamma, b, sampler, rows=rows)
        cdf = np.cumsum(cond, axis=1)
        z[rows] = np.minimum((rng.random(len(rows))[:, None] * cdf[:, -1:] >= cdf).sum(axis=1), K - 1)
    return z


def restated_ladder(X, z0, K, alpha, beta, gamma, powers, steps, seed, sampler="collapsed", batch=None, rng_seed=0):
    """`steps` times: one sweep of every rung (batches of `batch` rows against counts frozen at batch start, draws
    from a NumPy generator per rung), then exchange point t by the device's rule and the device's uniforms.  States
    move, temperatures stay.  Returns {"proposed", "accepted": (R - 1,), "walker": (R,), "records": per step a list of
    (r, d, u, accepted)}."""
    R = len(powers)
    batch = batch or max(1, len(X) // 8)
    zs = [np.array(z0) for _ in range(R)]
    rngs = [np.random.default_rng([rng_seed, r]) for r in range(R)]
    proposed, accepted = np.zeros(R - 1, dtype=np.int64), np.zeros(R - 1, dtype=np.int64)
    walker = np.arange(R)
    records = []
    for t in range(steps):
        for r in range(R):
            restated_sweep(X, zs[r], K, alpha, beta, gamma, powers[r], sampler, rngs[r], batch)
        L = [log_lik(X, zs[r], beta, gamma) for r in range(R)]
        step = []
        for r in proposed_pairs(R, t):
            d = log_ratio(powers[r], powers[r + 1], L[r], L[r + 1])
            u = exchange_uniform(seed, r, t)
            acc = accepts(d, u)
            proposed[r] += 1
            if acc:
                accepted[r] += 1
                zs[r], zs[r + 1] = zs[r + 1], zs[r]
                walker[[r, r + 1]] = walker[[r + 1, r]]
            step.append((r, float(d), u, acc))
        records.append(step)
    return {"proposed": proposed, "accepted": accepted, "walker": walker, "records": records}


# ---------------------------------------------------------------- exact matrices over the partitions of a small data set (DP)
def log_prior_dp(z, alpha):
    """log p(partition | alpha) of the Chinese restaurant process, up to the constant shared by all partitions"""
    n = np.bincount(np.asarray(z))
    n = n[n > 0]
    return len(n) * np.log(alpha) + float(np.sum(gammaln(n)))


def tempered_posterior(X, parts, alpha, beta, gamma, b):
    """(pi_b over `parts`, the log_lik of every partition)"""
    L = np.array([log_lik(X, np.array(z), beta, gamma) for z in parts])
    lp = np.array([log_prior_dp(z, alpha) for z in parts]) + b * L
    w = np.exp(lp - lp.max())
    return w / w.sum(), L


def scan_matrix(X, parts, alpha, beta, gamma, b, K):
    """The transition matrix over partitions of one sequential scan (batch 1) of the tempered DP conditional."""
    X = np.asarray(X, dtype=np.int64)
    N = len(X)
    index = {s: k for k, s in enumerate(parts)}
    T = np.zeros((len(parts), len(parts)))
    for si, z0 in enumerate(parts):
        dist = {tuple(z0): 1.0}
        for i in range(N):
            nxt = {}
            for zt, pr in dist.items():
                z = np.array(zt)
                cond = z_conditional(X, z, K, alpha, beta, gamma, b, "dp", rows=[i])[0]
                for k in np.flatnonzero(cond > 0):
                    z2 = z.copy()
                    z2[i] = k
                    key = smr.canon(tuple(z2))  # the conditional does not depend on the numbering of the blocks
                    nxt[key] = nxt.get(key, 0.0) + pr * cond[k]
            dist = nxt
        for zt, pr in dist.items():
            T[si, index[zt]] += pr
    return T


def product_scan(J, Ts):
    """One scan of every rung of a ladder on the product space: J[s_0, ..., s_{R-1}] the joint distribution over the
    rungs' partitions, Ts[r] the scan matrix of rung r.  The rungs move independently."""
    for r, T in enumerate(Ts):
        J = np.moveaxis(np.tensordot(J, T, axes=([r], [0])), -1, r)
    return J


def product_exchange(J, L, powers, pairs):
    """One exchange point on the product space of R rungs: every pair (r, r + 1) in `pairs` (disjoint) is swapped with
    probability min(1, exp((b_r - b_{r+1}) (L[s_{r+1}] - L[s_r]))).  exchange_matrix, without the matrix."""
    L = np.asarray(L)
    for r in pairs:
        d = (powers[r] - powers[r + 1]) * (L[None, :] - L[:, None])  # d[s_r, s_{r+1}]
        a = np.where(d >= 0, 1.0, np.exp(np.minimum(d, 0.0)))
        M = np.moveaxis(J, (r, r + 1), (0, 1))
        A = a.reshape(a.shape + (1,) * (J.ndim - 2))
        M = (1.0 - A) * M + np.swapaxes(A * M, 0, 1)  # the mass at (s, s') that moves lands at (s', s)
        J = np.moveaxis(M, (0, 1), (r, r + 1))
    return J


def exchange_matrix(L, b0, b1):
    """One exchange point of a ladder of two rungs on the product space: state (s0, s1) -> index s0 * n + s1; the pair
    is swapped with probability min(1, exp((b0 - b1) (L[s1] - L[s0])))."""
    n = len(L)
    T = np.zeros((n * n, n * n))
    for s0 in range(n):
        for s1 in range(n):
            d = (b0 - b1) * (L[s1] - L[s0])
            a = 1.0 if d >= 0 else float(np.exp(d))
            T[s0 * n + s1, s1 * n + s0] += a
            T[s0 * n + s1, s0 * n + s1] += 1.0 - a
    return T
