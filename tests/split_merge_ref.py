"""The split-merge move of the DP chain (include/bmm_mcmc.h "split-merge moves"), restated in NumPy.

Labels are 0-based here.  `move` is one move as the device executes it, fed by a `draws` object: PhiloxDraws gives
the device's own streams (so the integer parts of a device step can be replayed exactly), RngDraws a NumPy
generator (for long chains on the CPU).  `transition_matrix` enumerates the move exactly on a small data set.
"""
import itertools
import math

import numpy as np
from scipy.special import gammaln

SPLIT, MERGE, SKIPPED = "split", "merge", "skipped"
OUTSIDE = 255
_M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- Philox, as bmm_spec.h
def philox4x32_10(c, k):
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def philox2x32_10(c0, c1, k):
    """vectorised over c0 (uint64 arrays holding 32-bit words)"""
    c0 = np.asarray(c0, dtype=np.uint64)
    c1 = np.full_like(c0, c1)
    k = np.full_like(c0, k)
    m32 = np.uint64(_M32)
    for _ in range(10):
        pr = np.uint64(0xD256D193) * c0
        c0, c1 = (pr >> np.uint64(32)) ^ k ^ c1, pr & m32
        k = (k + np.uint64(0x9E3779B9)) & m32
    return c0, c1


def u01(a, b):
    return ((a >> 5) * 67108864.0 + (b >> 6)) * 2.0 ** -53


def u52(a, b):
    """52-bit uniform: the words fill the mantissa of a double in [1, 2), minus 1"""
    hi = np.uint64(0x3FF00000) | (a >> np.uint64(12))
    lo = ((a << np.uint64(20)) & np.uint64(_M32)) | (b >> np.uint64(12))
    return ((hi << np.uint64(32)) | lo).view(np.float64) - 1.0


class PhiloxDraws:
    """the streams of move `move` ahead of sweep `sweep` (sm_move_draws, sm_member_uniform)"""

    def __init__(self, seed, sweep, move):
        self.key = (seed & _M32, (seed >> 32) & _M32)
        self.sweep, self.move = sweep, move
        self.r0 = philox4x32_10((move, 0, sweep, 8), self.key)
        self.r1 = philox4x32_10((move, 1, sweep, 8), self.key)
        self.salt = self.r1[2]

    def pair(self, N):
        i = min(int(u01(self.r0[0], self.r0[1]) * float(N)), N - 1)
        j = min(int(u01(self.r0[2], self.r0[3]) * float(N - 1)), N - 2)
        return i, j + 1 if j >= i else j

    def log_u(self):
        return math.log(1.0 - u01(self.r1[0], self.r1[1]))

    def member(self, t, rows):
        a, b = philox2x32_10(np.asarray(rows, dtype=np.uint64), 0x80000000 | t, self.salt)
        return u52(a, b)


class RngDraws:
    def __init__(self, rng):
        self.rng = rng

    def pair(self, N):
        i = int(self.rng.integers(N))
        j = int(self.rng.integers(N - 1))
        return i, j + 1 if j >= i else j

    def log_u(self):
        return math.log(1.0 - self.rng.random())

    def member(self, t, rows):
        return self.rng.random(len(rows))


# ---------------------------------------------------------------- the restricted scan
def side_logp(X2, side, beta, gamma):
    """X2: the rows of the two labels, anchors included (n x P, 0/1); side: their sides.  Per row, the log
    probabilities of side 0 and side 1 against the statistics of `side`, the row's own contribution removed:
    w_c = (n_c - [own]) prod_d predictive.  Summed as the device sums: onto base[own], in feature order."""
    X2 = np.asarray(X2, dtype=np.int64)
    side = np.asarray(side, dtype=np.int64)
    n = np.array([np.sum(side == 0), np.sum(side == 1)], dtype=np.float64)
    S = np.stack([X2[side == 0].sum(0), X2[side == 1].sum(0)]).astype(np.float64)
    P = X2.shape[1]
    bg = beta + gamma
    D = np.zeros((P, 2, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        for own in (0, 1):
            nm, sm, npl, sp = n[own] - 1.0, S[own], n[1 - own], S[1 - own]
            denm, denp = np.log(bg + nm), np.log(bg + npl)
            m = np.stack([np.log((gamma + nm) - sm) - denm, np.log(beta + (sm - 1.0)) - denm], 1)  # [d][x]
            pl = np.stack([np.log((gamma + npl) - sp) - denp, np.log(beta + sp) - denp], 1)
            D[:, own, :] = pl - m if own else m - pl
        base = np.array([np.log(n[0] - 1.0) - np.log(n[1]), np.log(n[0]) - np.log(n[1] - 1.0)])
    acc = base[side]
    for d in range(P):
        acc = acc + D[d, side, X2[:, d]]
    pos = acc > 0.0
    with np.errstate(invalid="ignore"):
        l = -np.log(1.0 + np.exp(np.where(pos, -acc, acc)))
    return np.where(pos, l, l + acc), np.where(pos, l - acc, l)


def fixed_order_sum(v):
    """1024 partial sums, element i in partial i mod 1024, ascending; then a binary tree (k_loo_reduce's order)"""
    part = np.zeros(1024)
    np.add.at(part, np.arange(len(v)) % 1024, v)
    while len(part) > 1:
        h = len(part) // 2
        part = part[:h] + part[h:]
    return float(part[0])


def log_marginal(n, S, beta, gamma):
    """L(c) of the header: log of the Beta-Bernoulli marginal likelihood of a cluster with sizes n, counts S"""
    S = np.asarray(S, dtype=np.float64)
    return float(np.sum(gammaln(beta + S) + gammaln(gamma + n - S) - gammaln(beta + gamma + n))
                 + len(S) * (gammaln(beta + gamma) - gammaln(beta) - gammaln(gamma)))


def log_ratio_parts(kind, X2, old_side, new_side, alpha, beta, gamma):
    """log_prior and log_lik of the header's step 8.  X2: the rows of the two labels; old_side: which of the two
    labels each row carries now (a split: all 0); new_side: as proposed (a merge: all 0)."""
    X2 = np.asarray(X2, dtype=np.int64)

    def parts(sd):
        out = []
        for c in (0, 1):
            rows = X2[np.asarray(sd) == c]
            out.append((len(rows), rows.sum(0)))
        return out
    (no0, So0), (no1, So1) = parts(old_side)
    (nn0, Sn0), (nn1, Sn1) = parts(new_side)
    if kind == SPLIT:
        prior = math.log(alpha) + gammaln(nn0) + gammaln(nn1) - gammaln(no0)
        lik = log_marginal(nn0, Sn0, beta, gamma) + log_marginal(nn1, Sn1, beta, gamma) - log_marginal(no0, So0, beta, gamma)
    else:
        prior = -math.log(alpha) + gammaln(nn0) - gammaln(no0) - gammaln(no1)
        lik = log_marginal(nn0, Sn0, beta, gamma) - log_marginal(no0, So0, beta, gamma) - log_marginal(no1, So1, beta, gamma)
    return float(prior), float(lik)


# ---------------------------------------------------------------- one move
def move(X, z, maxK, alpha, beta, gamma, scans, draws, diagnostics=True):
    """One move on labels z (0-based, all seated).  Returns the diagnostics of bmm_chain_split_merge_step (labels
    0-based) and "z": the labels afterwards."""
    X = np.asarray(X, dtype=np.int64)
    z = np.asarray(z, dtype=np.int64)
    N = len(z)
    i, j = draws.pair(N)
    a, b = int(z[i]), int(z[j])
    Nk = np.bincount(z, minlength=maxK)
    out = {"rows": (i, j), "log_u": draws.log_u(), "accepted": False, "z": z.copy()}
    if a == b:
        free = np.flatnonzero(Nk == 0)
        if len(free) == 0:
            out.update(kind=SKIPPED, labels=(a, a), members=0, n_before=(int(Nk[a]), 0), n_after=(0, 0))
            return out
        kind, second = SPLIT, int(free[0])
    else:
        kind, second = MERGE, b
    rows = np.flatnonzero((z == a) | ((z == second) if kind == MERGE else False))
    anchor = (rows == i) | (rows == j)
    fixed = np.where(rows == j, 1, 0)

    def settle(new):
        return np.where(anchor, fixed, new)
    side = settle((draws.member(0, rows) >= 0.5).astype(np.int64))
    launch = side.copy()
    X2 = X[rows]
    for t in range(1, scans + 1):
        lp0, _ = side_logp(X2, side, beta, gamma)
        side = settle(np.where(draws.member(t, rows) < np.exp(lp0), 0, 1))
    lp0, lp1 = side_logp(X2, side, beta, gamma)
    if kind == SPLIT:
        prop = settle(np.where(draws.member(scans + 1, rows) < np.exp(lp0), 0, 1))
        target, old, new = prop, np.zeros(len(rows), dtype=np.int64), prop
    else:
        prop = side
        target = (z[rows] == second).astype(np.int64)
        old, new = target, np.zeros(len(rows), dtype=np.int64)
    lq_rows = np.zeros(N)
    lq_rows[rows] = np.where(anchor, 0.0, np.where(target == 0, lp0, lp1))
    log_q = fixed_order_sum(lq_rows)
    prior, lik = log_ratio_parts(kind, X2, old, new, alpha, beta, gamma)
    log_r = prior + lik - log_q if kind == SPLIT else prior + lik + log_q
    accepted = out["log_u"] < log_r

    def full(sd):
        f = np.full(N, OUTSIDE, dtype=np.uint8)
        f[rows] = np.where(anchor, 2 + fixed, sd)
        return f
    znew = z.copy()
    if accepted:
        if kind == SPLIT:
            znew[rows[prop == 1]] = second
        else:
            znew[rows] = min(a, second)
    if not diagnostics:  # (long chains on the CPU: the state is all they need)
        out.update(kind=kind, accepted=bool(accepted), z=znew)
        return out
    n_after = (int(np.sum(prop == 0)), int(np.sum(prop == 1))) if kind == SPLIT else (len(rows), 0)
    out.update(kind=kind, labels=(a, second), members=len(rows) - 2, n_before=(int(Nk[a]), int(Nk[second]) if kind == MERGE else 0),
               n_after=n_after, launch_side=full(launch), proposal_side=full(prop), log_prior=prior, log_lik=lik,
               log_q=log_q, log_r=log_r, accepted=bool(accepted), z=znew, abs_terms=_abs_terms(kind, X2, old, new, alpha, beta, gamma))
    return out


def _abs_terms(kind, X2, old, new, alpha, beta, gamma):
    """sum of |lgamma| over the terms of log_prior and log_lik, and their number: what an error bound needs"""
    tot, cnt = abs(math.log(alpha)), 1
    for sd in (old, new):
        for c in (0, 1):
            r = X2[np.asarray(sd) == c]
            if len(r) == 0:
                continue
            n, S = len(r), r.sum(0).astype(np.float64)
            v = np.concatenate([gammaln(beta + S), gammaln(gamma + n - S), np.full(len(S), gammaln(beta + gamma + n)), [gammaln(n)]])
            tot += float(np.sum(np.abs(v)))
            cnt += len(v)
    P = X2.shape[1]
    tot += P * float(abs(gammaln(beta + gamma)) + abs(gammaln(beta)) + abs(gammaln(gamma)))
    return tot, cnt + 3 * P


# ---------------------------------------------------------------- canonical partitions and the exact kernel
def canon(z):
    m, out = {}, []
    for v in z:
        out.append(m.setdefault(int(v), len(m)))
    return tuple(out)


def partitions(n):
    def rec(prefix, mx):
        if len(prefix) == n:
            yield tuple(prefix)
            return
        for v in range(mx + 2):
            yield from rec(prefix + [v], max(mx, v))
    return list(rec([0], 0))


def transition_matrix(X, alpha, beta, gamma, scans):
    """The move's exact transition matrix over the partitions of the rows of X (never skipped: a free label always
    exists): every pair, launch state, intermediate and final outcome enumerated, with the probabilities side_logp
    gives and the ratio log_ratio_parts gives."""
    X = np.asarray(X, dtype=np.int64)
    N = len(X)
    states = partitions(N)
    index = {s: k for k, s in enumerate(states)}
    T = np.zeros((len(states), len(states)))
    p_pair = 1.0 / (N * (N - 1))
    for s in states:
        z = np.array(s)
        for i, j in itertools.permutations(range(N), 2):
            a, b = z[i], z[j]
            kind = SPLIT if a == b else MERGE
            rows = np.flatnonzero((z == a) | (z == b))
            X2 = X[rows]
            anchor = (rows == i) | (rows == j)
            fixed = np.where(rows == j, 1, 0)
            mem = np.flatnonzero(~anchor)
            M = len(mem)

            def with_members(bits):
                sd = fixed.copy()
                sd[mem] = bits
                return sd

            def step_probs(sd):
                """probability of every outcome of one scan from state sd: dict bits -> prob"""
                lp0, lp1 = side_logp(X2, sd, beta, gamma)
                res = {}
                for bits in itertools.product((0, 1), repeat=M):
                    lp = sum(lp1[mem[q]] if bits[q] else lp0[mem[q]] for q in range(M))
                    res[bits] = math.exp(lp)
                return res
            # distribution over the state the final scan starts from
            dist = {bits: 0.5 ** M for bits in itertools.product((0, 1), repeat=M)}
            for _ in range(scans):
                nxt = {}
                for bits, pr in dist.items():
                    for b2, p2 in step_probs(with_members(bits)).items():
                        nxt[b2] = nxt.get(b2, 0.0) + pr * p2
                dist = nxt
            stay = 0.0
            for bits, pr in dist.items():
                fin = step_probs(with_members(bits))
                if kind == SPLIT:
                    for b2, q in fin.items():
                        prop = with_members(b2)
                        prior, lik = log_ratio_parts(SPLIT, X2, np.zeros(len(rows), dtype=int), prop, alpha, beta, gamma)
                        acc = min(1.0, math.exp(prior + lik - math.log(q)))
                        znew = z.copy()
                        znew[rows[prop == 1]] = N  # a fresh label
                        T[index[s], index[canon(znew)]] += p_pair * pr * q * acc
                        stay += pr * q * (1.0 - acc)
                else:
                    target = tuple(int(z[rows[q]] == b) for q in mem)
                    q = fin[target]
                    old = (z[rows] == b).astype(int)
                    prior, lik = log_ratio_parts(MERGE, X2, old, np.zeros(len(rows), dtype=int), alpha, beta, gamma)
                    acc = min(1.0, math.exp(prior + lik + math.log(q)))
                    znew = z.copy()
                    znew[rows] = min(a, b)
                    T[index[s], index[canon(znew)]] += p_pair * pr * acc
                    stay += pr * (1.0 - acc)
            T[index[s], index[s]] += p_pair * stay
    return states, T


def chain(X, z0, maxK, alpha, beta, gamma, scans, n_moves, rng):
    """n_moves moves from z0; returns the visited canonical partitions"""
    z = np.asarray(z0, dtype=np.int64)
    dr = RngDraws(rng)
    visited = []
    for _ in range(n_moves):
        z = move(X, z, maxK, alpha, beta, gamma, scans, dr, diagnostics=False)["z"]
        visited.append(canon(z))
    return visited
