"""The allocation sampler (include/bmm_mcmc.h "allocation sampler"), restated in NumPy.

Labels are 0-based here.  The state is (K, z), z in {0..K-1}^N.  `log_target` is log pi(K, z) by brute force; `move` is
one eject / absorb move as the device executes it, fed by a `draws` object (PhiloxDraws: the device's own streams, with
p_E handed in from the host build of the spec, tests/alloc/alloc_host.cpp; RngDraws: a NumPy generator);
`conditional` is the sweep's conditional of one row.  `move_matrix` and `row_matrix` enumerate both exactly on a small
data set, over the labelled states, and `lump` carries them to (K, partition).
"""
import itertools
import math

import numpy as np
from scipy.special import betaln, gammaln

import split_merge_ref as sm

EJECT, ABSORB = "eject", "absorb"
OUTSIDE = 255


# ---------------------------------------------------------------- the target
def log_marginal(n, S, beta, gamma):
    """L(c) of the header; exactly 0 for an empty label"""
    if n == 0:
        return 0.0
    return sm.log_marginal(n, S, beta, gamma)


def log_target(K, z, X, a, beta, gamma, log_prior_k):
    z = np.asarray(z, dtype=np.int64)
    X = np.asarray(X, dtype=np.int64)
    N = len(z)
    lp = log_prior_k[K - 1] + gammaln(K * a) - gammaln(K * a + N)
    for k in range(K):
        rows = z == k
        n = int(rows.sum())
        lp += gammaln(a + n) - gammaln(a) + log_marginal(n, X[rows].sum(0), beta, gamma)
    return float(lp)


def poisson_prior(maxK, lam=1.0):
    """log of Poisson(lam) truncated to 1..maxK (the default of Nobile & Fearnside)"""
    k = np.arange(1, maxK + 1, dtype=np.float64)
    lw = k * math.log(lam) - gammaln(k + 1.0)
    return lw - np.log(np.sum(np.exp(lw)))


def uniform_prior(maxK):
    return np.full(maxK, -math.log(maxK))


def p_eject(K, maxK):
    return 1.0 if K == 1 else (0.0 if K == maxK else 0.5)


# ---------------------------------------------------------------- the draws
class PhiloxDraws:
    """the streams of move `move` ahead of sweep `sweep` (ea_move_draws of bmm_spec.h).  Kind, labels, u, salt and the
    members' uniforms are restated here; p_E, a Beta variate of the spec's own log / exp / sqrt, is handed in."""

    def __init__(self, seed, sweep, move, pe=None):
        key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        self.r = [sm.philox4x32_10((move, b, sweep, 11), key) for b in range(3)]
        self.salt = self.r[1][2]
        self.pe = pe

    def kind(self, K, maxK):
        if K <= 1:
            return EJECT
        if K >= maxK:
            return ABSORB
        return EJECT if sm.u01(self.r[0][0], self.r[0][1]) < 0.5 else ABSORB

    def j1(self, K):
        return min(int(sm.u01(self.r[0][2], self.r[0][3]) * float(K)), K - 1)

    def j2(self, K, j1):
        t = min(int(sm.u01(self.r[2][0], self.r[2][1]) * float(K - 1)), K - 2)
        return t + 1 if t >= j1 else t

    def log_u(self):
        return math.log(1.0 - sm.u01(self.r[1][0], self.r[1][1]))

    def p_e(self, e):
        assert self.pe is not None, "p_E comes from the host build of the spec"
        return self.pe

    def member(self, rows):
        a, b = sm.philox2x32_10(np.asarray(rows, dtype=np.uint64), 0x80000000, self.salt)
        return sm.u52(a, b)


class RngDraws:
    def __init__(self, rng):
        self.rng = rng
        self.u = rng.random(4)

    def kind(self, K, maxK):
        return EJECT if self.u[0] < p_eject(K, maxK) else ABSORB

    def j1(self, K):
        return min(int(self.u[1] * K), K - 1)

    def j2(self, K, j1):
        t = min(int(self.u[2] * (K - 1)), K - 2)
        return t + 1 if t >= j1 else t

    def log_u(self):
        return math.log(1.0 - self.u[3])

    def p_e(self, e):
        return float(self.rng.beta(e, e))

    def member(self, rows):
        return self.rng.random(len(rows))


# ---------------------------------------------------------------- one move
def ratio_parts(Kl, N, n1, S1, n2, S2, a, beta, gamma, e, log_prior_k, maxK):
    """the four parts of the eject's log r from the smaller K = Kl: the component (n1 + n2, S1 + S2) into (n1, S1) and
    (n2, S2)"""
    S1, S2 = np.asarray(S1, dtype=np.float64), np.asarray(S2, dtype=np.float64)
    n = n1 + n2
    prior = (log_prior_k[Kl] - log_prior_k[Kl - 1]
             + (gammaln((Kl + 1) * a) - gammaln((Kl + 1) * a + N)) - (gammaln(Kl * a) - gammaln(Kl * a + N))
             + gammaln(a + n1) + gammaln(a + n2) - gammaln(a + n) - gammaln(a))
    lik = log_marginal(n1, S1, beta, gamma) + log_marginal(n2, S2, beta, gamma) - log_marginal(n, S1 + S2, beta, gamma)
    log_q = betaln(e + n1, e + n2) - betaln(e, e)
    log_move = math.log(1.0 - p_eject(Kl + 1, maxK)) - math.log(p_eject(Kl, maxK))
    return float(prior), float(lik), float(log_q), float(log_move)


def abs_terms(Kl, N, n1, S1, n2, S2, a, beta, gamma):
    """sum of |lgamma| over the terms of log_prior and log_lik as the device adds them, and their number"""
    S1, S2 = np.asarray(S1, dtype=np.float64), np.asarray(S2, dtype=np.float64)
    n, P = n1 + n2, len(S1)
    v = [gammaln((Kl + 1) * a), gammaln((Kl + 1) * a + N), gammaln(Kl * a), gammaln(Kl * a + N), gammaln(a + n1), gammaln(a + n2),
         gammaln(a + n), gammaln(a)]
    for m, S in ((n1, S1), (n2, S2), (n, S1 + S2)):
        v += list(gammaln(beta + S)) + list(gammaln(gamma + m - S)) + [P * gammaln(beta + gamma + m)]
    v += [P * gammaln(beta + gamma), P * gammaln(beta), P * gammaln(gamma)]
    return float(np.sum(np.abs(v))), len(v) + 4 * P


def move(X, z, K, maxK, a, beta, gamma, e, log_prior_k, draws):
    """One move on (K, z).  Returns the diagnostics of bmm_chain_alloc_step (labels 0-based) and "z", "K" afterwards."""
    X = np.asarray(X, dtype=np.int64)
    z = np.asarray(z, dtype=np.int64)
    N = len(z)
    kind = draws.kind(K, maxK)
    j1 = draws.j1(K)
    Nk = np.bincount(z, minlength=maxK)
    side = np.full(N, OUTSIDE, dtype=np.uint8)
    out = {"kind": kind, "log_u": draws.log_u(), "k_before": K}
    znew = z.copy()
    if kind == EJECT:
        j2, Kl = K, K
        rows = np.flatnonzero(z == j1)
        pe = draws.p_e(e)
        moved = draws.member(rows) < pe
        side[rows] = moved.astype(np.uint8)
        n2, S2 = int(moved.sum()), X[rows[moved]].sum(0)
        n1, S1 = len(rows) - n2, X[rows[~moved]].sum(0)
        znew[rows[moved]] = j2
        out.update(pe=pe, n_before=(len(rows), 0), n_after=(n1, n2))
    else:
        j2, Kl = draws.j2(K, j1), K - 1
        last = K - 1
        side[z == j1] = 0
        side[z == j2] = 1
        if j2 != last:
            side[z == last] = 2
        n1, S1 = int(Nk[j1]), X[z == j1].sum(0)
        n2, S2 = int(Nk[j2]), X[z == j2].sum(0)
        znew[z == j2] = j1
        if j2 != last:
            znew[znew == last] = j2
        out.update(pe=None, n_before=(n1, n2), n_after=(n1 + n2, 0))
    prior, lik, log_q, log_move = ratio_parts(Kl, N, n1, S1, n2, S2, a, beta, gamma, e, log_prior_k, maxK)
    if kind == EJECT:
        log_r = prior + lik + log_move - log_q
    else:
        prior, lik = -prior, -lik
        log_r = prior + lik - log_move + log_q
    accepted = out["log_u"] < log_r
    out.update(labels=(j1, j2), members=n2, side=side, log_prior=prior, log_lik=lik, log_q=log_q, log_move=log_move,
               log_r=log_r, accepted=bool(accepted), z=znew if accepted else z.copy(),
               K=(K + 1 if kind == EJECT else K - 1) if accepted else K, z_proposed=znew,
               abs_terms=abs_terms(Kl, N, n1, S1, n2, S2, a, beta, gamma))
    out["k_after"] = out["K"]
    return out


# ---------------------------------------------------------------- the sweep's conditional of one row
def conditional(X, z, i, K, a, beta, gamma):
    """p(z_i = k | the other rows), k < K: (n_k' + a) prod_d predictive, the row taken out of its own label; an empty
    label has the prior terms"""
    X = np.asarray(X, dtype=np.int64)
    z = np.asarray(z, dtype=np.int64)
    keep = np.arange(len(z)) != i
    lw = np.zeros(K)
    for k in range(K):
        rows = keep & (z == k)
        n, S = int(rows.sum()), X[rows].sum(0).astype(np.float64)
        t1, t0 = np.log(beta + S), np.log(gamma + n - S)
        lw[k] = math.log(n + a) + float(np.sum(np.where(X[i] == 1, t1, t0))) - X.shape[1] * math.log(beta + gamma + n)
    w = np.exp(lw - lw.max())
    return w / w.sum()


# ---------------------------------------------------------------- exact kernels on a small data set
def labelled_states(N, maxK, fixed_K=None):
    out = []
    for K in ([fixed_K] if fixed_K else range(1, maxK + 1)):
        out += [(K, z) for z in itertools.product(range(K), repeat=N)]
    return out


def target_vector(states, X, a, beta, gamma, log_prior_k):
    lw = np.array([log_target(K, z, X, a, beta, gamma, log_prior_k) for K, z in states])
    w = np.exp(lw - lw.max())
    return w / w.sum()


def move_matrix(X, maxK, a, beta, gamma, e, log_prior_k):
    """The exact transition matrix of one eject / absorb move over the labelled states: every kind, label (pair) and
    subset of moved rows, a subset's probability being the Beta(e, e) integral exp(log q)."""
    X = np.asarray(X, dtype=np.int64)
    N = len(X)
    states = labelled_states(N, maxK)
    index = {s: k for k, s in enumerate(states)}
    T = np.zeros((len(states), len(states)))
    for K, zt in states:
        z = np.array(zt)
        row = index[(K, zt)]
        pe = p_eject(K, maxK)
        if pe > 0.0:
            for j1 in range(K):
                rows = np.flatnonzero(z == j1)
                for bits in itertools.product((False, True), repeat=len(rows)):
                    moved = np.array(bits, dtype=bool)
                    n2, n1 = int(moved.sum()), len(rows) - int(moved.sum())
                    S2, S1 = X[rows[moved]].sum(0), X[rows[~moved]].sum(0)
                    prior, lik, log_q, log_move = ratio_parts(K, N, n1, S1, n2, S2, a, beta, gamma, e, log_prior_k, maxK)
                    pr = pe / K * math.exp(log_q)
                    acc = min(1.0, math.exp(prior + lik + log_move - log_q))
                    znew = z.copy()
                    znew[rows[moved]] = K
                    T[row, index[(K + 1, tuple(znew))]] += pr * acc
                    T[row, row] += pr * (1.0 - acc)
        if pe < 1.0:
            for j1, j2 in itertools.permutations(range(K), 2):
                n1, S1 = int(np.sum(z == j1)), X[z == j1].sum(0)
                n2, S2 = int(np.sum(z == j2)), X[z == j2].sum(0)
                prior, lik, log_q, log_move = ratio_parts(K - 1, N, n1, S1, n2, S2, a, beta, gamma, e, log_prior_k, maxK)
                pr = (1.0 - pe) / (K * (K - 1))
                acc = min(1.0, math.exp(-(prior + lik + log_move - log_q)))
                znew = z.copy()
                znew[z == j2] = j1
                if j2 != K - 1:
                    znew[znew == K - 1] = j2
                T[row, index[(K - 1, tuple(znew))]] += pr * acc
                T[row, row] += pr * (1.0 - acc)
    return states, T


def row_matrix(X, K, i, a, beta, gamma):
    """the exact transition matrix of the sweep's update of row i over the labelled states of a fixed K"""
    N = len(X)
    states = labelled_states(N, K, fixed_K=K)
    index = {s: k for k, s in enumerate(states)}
    T = np.zeros((len(states), len(states)))
    for _, zt in states:
        p = conditional(X, zt, i, K, a, beta, gamma)
        for k in range(K):
            T[index[(K, zt)], index[(K, zt[:i] + (k,) + zt[i + 1:])]] += p[k]
    return states, T


def lump(states, pi, T):
    """(K, partition) classes: their target, the flow matrix F[s, t] = sum pi(z) T(z, z') over z in s, z' in t, and the
    largest difference between two members of a class in their transition probabilities into a class (0: strongly
    lumpable)"""
    classes = sorted({(K, sm.canon(z)) for K, z in states})
    cidx = {c: k for k, c in enumerate(classes)}
    member = np.array([cidx[(K, sm.canon(z))] for K, z in states])
    M = np.zeros((len(states), len(classes)))
    M[np.arange(len(states)), member] = 1.0
    into = T @ M
    spread = 0.0
    for c in range(len(classes)):
        blk = into[member == c]
        spread = max(spread, float(np.max(blk.max(0) - blk.min(0))))
    return classes, M.T @ pi, M.T @ (pi[:, None] * into), spread


def exact_posterior(X, maxK, a, beta, gamma, log_prior_k, fixed_K=None):
    """pi on the lumped states by brute force: pi(K, z) times the K! / (K - b)! labellings of a partition of b blocks.
    Returns the partitions of the rows (split_merge_ref.partitions), their posterior weights summed over K, and p(K | x)."""
    parts = sm.partitions(len(X))
    Ks = [fixed_K] if fixed_K else list(range(1, maxK + 1))
    lw = np.full((len(Ks), len(parts)), -np.inf)
    for r, K in enumerate(Ks):
        for c, z in enumerate(parts):
            b = max(z) + 1
            if b <= K:
                lw[r, c] = log_target(K, z, X, a, beta, gamma, log_prior_k) + gammaln(K + 1) - gammaln(K - b + 1)
    w = np.exp(lw - lw.max())
    w /= w.sum()
    return parts, w.sum(0), dict(zip(Ks, w.sum(1)))


def chain(X, z0, K0, maxK, a, beta, gamma, e, log_prior_k, n, rng, sweeps=True, moves=1):
    """n iterations from (K0, z0) on the CPU: `moves` moves, then (sweeps) one batch-1 sweep; returns the visited
    (K, canonical partition)"""
    z, K = np.asarray(z0, dtype=np.int64).copy(), K0
    seen = []
    for _ in range(n):
        for _ in range(moves):
            r = move(X, z, K, maxK, a, beta, gamma, e, log_prior_k, RngDraws(rng))
            z, K = r["z"], r["K"]
        if sweeps:
            for i in range(len(z)):
                z[i] = rng.choice(K, p=conditional(X, z, i, K, a, beta, gamma))
        seen.append((K, sm.canon(z)))
    return seen
