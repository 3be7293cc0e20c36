"""The split-merge move of the allocation sampler (include/bmm_mcmc.h "split-merge moves of the allocation sampler",
DESIGN.md section 24), restated in NumPy.

Labels are 0-based here.  The state is (K, z), z in {0..K-1}^N, as in alloc_ref.py.  `move` is one move as the device
executes it, fed by a `draws` object (PhiloxDraws: the device's own streams; split_merge_ref.RngDraws: a NumPy generator)
and, if given, by the launch sides a device step reported.  `move_matrix` enumerates the move exactly over the labelled
states of a small data set; alloc_ref.lump carries it to (K, partition).  `chain` is the restatement's own chain.
"""
import itertools
import math

import numpy as np
from scipy.special import gammaln

import alloc_ref as al
import split_merge_ref as sm

SPLIT, MERGE, SKIPPED = sm.SPLIT, sm.MERGE, sm.SKIPPED
OUTSIDE = sm.OUTSIDE
STREAM = 18  # kStreamAllocSplit


class PhiloxDraws(sm.PhiloxDraws):
    """the streams of move `move` ahead of sweep `sweep` (as_move_draws: sm_move_draws on stream 18)"""

    def __init__(self, seed, sweep, move):
        self.key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        self.sweep, self.move = sweep, move
        self.r0 = sm.philox4x32_10((move, 0, sweep, STREAM), self.key)
        self.r1 = sm.philox4x32_10((move, 1, sweep, STREAM), self.key)
        self.salt = self.r1[2]


# ---------------------------------------------------------------- the restricted scan with the `+ a` weights
def side_logp(X2, side, a, beta, gamma):
    """split_merge_ref.side_logp under the allocation prior between the two sides: w_c = (n_c - [own] + a) prod_d
    predictive.  Summed as the device sums: onto base[own], in feature order."""
    X2 = np.asarray(X2, dtype=np.int64)
    side = np.asarray(side, dtype=np.int64)
    n = np.array([np.sum(side == 0), np.sum(side == 1)], dtype=np.float64)
    S = np.stack([X2[side == 0].sum(0), X2[side == 1].sum(0)]).astype(np.float64)
    P = X2.shape[1]
    bg = beta + gamma
    D = np.zeros((P, 2, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        for own in (0, 1):
            nm, s_own, npl, sp = n[own] - 1.0, S[own], n[1 - own], S[1 - own]
            denm, denp = np.log(bg + nm), np.log(bg + npl)
            m = np.stack([np.log((gamma + nm) - s_own) - denm, np.log(beta + (s_own - 1.0)) - denm], 1)  # [d][x]
            pl = np.stack([np.log((gamma + npl) - sp) - denp, np.log(beta + sp) - denp], 1)
            D[:, own, :] = pl - m if own else m - pl
    base = np.array([np.log((n[0] - 1.0) + a) - np.log(n[1] + a), np.log(n[0] + a) - np.log((n[1] - 1.0) + a)])
    acc = base[side]
    for d in range(P):
        acc = acc + D[d, side, X2[:, d]]
    pos = acc > 0.0
    with np.errstate(invalid="ignore"):
        l = -np.log(1.0 + np.exp(np.where(pos, -acc, acc)))
    return np.where(pos, l, l + acc), np.where(pos, l - acc, l)


# ---------------------------------------------------------------- the ratio
def log_prior(K, N, a, log_prior_k, n, n0, n1, split):
    """as_log_prior of bmm_spec.h: K the open labels before the move; a merge is the negative of the split from K - 1"""
    Kl = K if split else K - 1
    v = (log_prior_k[Kl] - log_prior_k[Kl - 1] + math.log(Kl + 1)
         + (gammaln((Kl + 1) * a) - gammaln((Kl + 1) * a + N)) - (gammaln(Kl * a) - gammaln(Kl * a + N))
         + gammaln(a + n0) + gammaln(a + n1) - gammaln(a + n) - gammaln(a))
    return float(v if split else -v)


def log_lik_split(X2, side, beta, gamma):
    """L(side 0) + L(side 1) - L(both): the split's marginal-likelihood ratio; a merge's is its negative"""
    X2, side = np.asarray(X2, dtype=np.int64), np.asarray(side)
    r0, r1 = X2[side == 0], X2[side == 1]
    return (al.log_marginal(len(r0), r0.sum(0), beta, gamma) + al.log_marginal(len(r1), r1.sum(0), beta, gamma)
            - al.log_marginal(len(X2), X2.sum(0), beta, gamma))


def abs_terms(X2, side, beta, gamma):
    """sum of |lgamma| over the terms of log_lik as the device adds them, and their number"""
    X2, side = np.asarray(X2, dtype=np.int64), np.asarray(side)
    P = X2.shape[1]
    tot, cnt = 0.0, 0
    for r in (X2[side == 0], X2[side == 1], X2):
        n, S = len(r), r.sum(0).astype(np.float64)
        v = np.concatenate([gammaln(beta + S), gammaln(gamma + n - S), [P * gammaln(beta + gamma + n)]])
        tot += float(np.sum(np.abs(v)))
        cnt += len(v)
    tot += P * float(abs(gammaln(beta + gamma)) + abs(gammaln(beta)) + abs(gammaln(gamma)))
    return tot, cnt + 4 * P


# ---------------------------------------------------------------- one move
def move(X, z, K, maxK, a, beta, gamma, log_prior_k, scans, draws, launch=None, diagnostics=True):
    """One move on (K, z).  Returns the diagnostics of bmm_chain_alloc_split_merge_step (labels 0-based) and "z", "K"
    afterwards.  `launch`: N side bytes of a device step; its members' sides replace the restated launch draw."""
    X = np.asarray(X, dtype=np.int64)
    z = np.asarray(z, dtype=np.int64)
    N = len(z)
    i, j = draws.pair(N)
    la, zj = int(z[i]), int(z[j])
    out = {"rows": (i, j), "log_u": draws.log_u(), "accepted": False, "z": z.copy(), "K": K, "k_before": K, "k_after": K,
           "moved": -1}
    if la == zj:
        if K == maxK:
            out.update(kind=SKIPPED, labels=(la, la), members=0, n_before=(int(np.sum(z == la)), 0), n_after=(0, 0))
            return out
        kind, lb = SPLIT, K
    else:
        kind, lb = MERGE, zj
    rows = np.flatnonzero((z == la) | (z == lb))
    anchor = (rows == i) | (rows == j)
    fixed = np.where(rows == j, 1, 0)

    def settle(new):
        return np.where(anchor, fixed, new)
    if launch is None:
        side = settle((draws.member(0, rows) >= 0.5).astype(np.int64))
    else:
        side = settle(np.asarray(launch)[rows].astype(np.int64) & 1)
    launch_side = side.copy()
    X2 = X[rows]
    for t in range(1, scans + 1):
        lp0, _ = side_logp(X2, side, a, beta, gamma)
        side = settle(np.where(draws.member(t, rows) < np.exp(lp0), 0, 1))
    lp0, lp1 = side_logp(X2, side, a, beta, gamma)
    if kind == SPLIT:
        prop = settle(np.where(draws.member(scans + 1, rows) < np.exp(lp0), 0, 1))
        target = prop
    else:
        prop = side
        target = (z[rows] == lb).astype(np.int64)
    lq_rows = np.zeros(N)
    lq_rows[rows] = np.where(anchor, 0.0, np.where(target == 0, lp0, lp1))
    log_q = sm.fixed_order_sum(lq_rows)
    n0, n1 = int(np.sum(target == 0)), int(np.sum(target == 1))
    lik = log_lik_split(X2, target, beta, gamma)
    if kind == SPLIT:
        prior = log_prior(K, N, a, log_prior_k, len(rows), n0, n1, True)
        log_r = prior + lik - log_q
    else:
        prior, lik = log_prior(K, N, a, log_prior_k, len(rows), n0, n1, False), -lik
        log_r = prior + lik + log_q
    accepted = bool(out["log_u"] < log_r)
    znew, Knew, moved = z.copy(), K, -1
    if accepted:
        if kind == SPLIT:
            znew[rows[prop == 1]] = K
            Knew = K + 1
        else:
            znew[z == lb] = la
            if lb != K - 1:
                znew[znew == K - 1] = lb
                moved = K - 1
            Knew = K - 1
    out.update(kind=kind, labels=(la, lb), accepted=accepted, z=znew, K=Knew, k_after=Knew, moved=moved)
    if not diagnostics:
        return out

    def full(sd):
        f = np.full(N, OUTSIDE, dtype=np.uint8)
        f[rows] = np.where(anchor, 2 + fixed, sd)
        return f
    n_before = (len(rows), 0) if kind == SPLIT else (n0, n1)
    n_after = (n0, n1) if kind == SPLIT else (len(rows), 0)
    out.update(members=len(rows) - 2, n_before=n_before, n_after=n_after, launch_side=full(launch_side),
               proposal_side=full(prop), log_prior=prior, log_lik=lik, log_q=log_q, log_r=log_r,
               prior_args=(K, N, len(rows), n0, n1, kind == SPLIT), abs_terms=abs_terms(X2, target, beta, gamma))
    return out


# ---------------------------------------------------------------- the exact kernel on a small data set
def move_matrix(X, maxK, a, beta, gamma, log_prior_k, scans):
    """The exact transition matrix of one move over the labelled states (alloc_ref.labelled_states): every ordered pair,
    launch state, intermediate and final outcome enumerated.  What depends on the rows of the two blocks alone (the
    scans and the likelihood ratio) is computed once per (rows, i, j)."""
    X = np.asarray(X, dtype=np.int64)
    N = len(X)
    states = al.labelled_states(N, maxK)
    index = {s: k for k, s in enumerate(states)}
    T = np.zeros((len(states), len(states)))
    p_pair = 1.0 / (N * (N - 1))
    scan_memo, lik_memo = {}, {}

    def finals(rows_t, i, j):
        """(probability of the state the final scan starts from, an outcome of the final scan as sides over the rows,
        its probability) for every pair of the two"""
        key = (rows_t, i, j)
        if key in scan_memo:
            return scan_memo[key]
        rows = np.array(rows_t)
        X2 = X[rows]
        anchor = (rows == i) | (rows == j)
        fixed = np.where(rows == j, 1, 0)
        mem = np.flatnonzero(~anchor)
        M = len(mem)
        every = list(itertools.product((0, 1), repeat=M))

        def with_members(bits):
            sd = fixed.copy()
            sd[mem] = bits
            return sd

        def step(sd):
            lp0, lp1 = side_logp(X2, sd, a, beta, gamma)
            return {bits: math.exp(sum(lp1[mem[q]] if bits[q] else lp0[mem[q]] for q in range(M))) for bits in every}
        dist = {bits: 0.5 ** M for bits in every}
        for _ in range(scans):
            nxt = {}
            for bits, pr in dist.items():
                for b2, p2 in step(with_members(bits)).items():
                    nxt[b2] = nxt.get(b2, 0.0) + pr * p2
            dist = nxt
        res = [(pr, tuple(int(v) for v in with_members(b2)), q) for bits, pr in dist.items()
               for b2, q in step(with_members(bits)).items()]
        scan_memo[key] = res
        return res

    def lik(rows_t, side_t):
        key = (rows_t, side_t)
        if key not in lik_memo:
            lik_memo[key] = log_lik_split(X[np.array(rows_t)], np.array(side_t), beta, gamma)
        return lik_memo[key]
    for K, zt in states:
        z = np.array(zt)
        row = index[(K, zt)]
        for i, j in itertools.permutations(range(N), 2):
            la, lb = int(z[i]), int(z[j])
            if la == lb:
                if K == maxK:  # skipped
                    T[row, row] += p_pair
                    continue
                rows_t = tuple(int(r) for r in np.flatnonzero(z == la))
                for pr, prop, q in finals(rows_t, i, j):
                    n1 = sum(prop)
                    lr = log_prior(K, N, a, log_prior_k, len(prop), len(prop) - n1, n1, True) + lik(rows_t, prop) - math.log(q)
                    acc = min(1.0, math.exp(lr))
                    znew = z.copy()
                    znew[[r for r, s in zip(rows_t, prop) if s == 1]] = K
                    T[row, index[(K + 1, tuple(int(v) for v in znew))]] += p_pair * pr * q * acc
                    T[row, row] += p_pair * pr * q * (1.0 - acc)
            else:
                rows_t = tuple(int(r) for r in np.flatnonzero((z == la) | (z == lb)))
                target = tuple(int(z[r] == lb) for r in rows_t)
                n1 = sum(target)
                znew = z.copy()
                znew[z == lb] = la
                if lb != K - 1:
                    znew[znew == K - 1] = lb
                col = index[(K - 1, tuple(int(v) for v in znew))]
                lp = log_prior(K, N, a, log_prior_k, len(target), len(target) - n1, n1, False) - lik(rows_t, target)
                for pr, prop, q in finals(rows_t, i, j):
                    if prop != target:
                        continue
                    acc = min(1.0, math.exp(lp + math.log(q)))
                    T[row, col] += p_pair * pr * acc
                    T[row, row] += p_pair * pr * (1.0 - acc)
    return states, T


def lumped_target(classes, X, a, beta, gamma, log_prior_k):
    """pi(K, rho) of the header by brute force, scipy's gammaln only: p(K) K!/(K - t)! Gamma(Ka)/Gamma(Ka + N)
    prod_c Gamma(a + n_c)/Gamma(a) prod_c m(x_c), normalised over `classes` = [(K, canonical partition)]"""
    X = np.asarray(X, dtype=np.int64)
    N = len(X)
    lw = []
    for K, part in classes:
        z = np.array(part)
        t = int(z.max()) + 1
        v = log_prior_k[K - 1] + gammaln(K + 1) - gammaln(K - t + 1) + gammaln(K * a) - gammaln(K * a + N)
        for c in range(t):
            r = X[z == c]
            v += gammaln(a + len(r)) - gammaln(a) + sm.log_marginal(len(r), r.sum(0), beta, gamma)
        lw.append(v)
    w = np.exp(np.array(lw) - max(lw))
    return w / w.sum()


def exact_posterior_no_empty(X, maxK, a, beta, gamma, log_prior_k):
    """the enumeration restricted to the states with no empty component (K = t <= maxK), a class closed under the move:
    the partitions (split_merge_ref.partitions), their weights (0 above maxK blocks) and p(K | x, no empty component)"""
    parts = sm.partitions(len(X))
    ok = [c for c, z in enumerate(parts) if max(z) + 1 <= maxK]
    w = np.zeros(len(parts))
    w[ok] = lumped_target([(max(parts[c]) + 1, parts[c]) for c in ok], X, a, beta, gamma, log_prior_k)
    pk = {K: float(sum(w[c] for c in ok if max(parts[c]) + 1 == K)) for K in range(1, maxK + 1)}
    return parts, w, pk


# ---------------------------------------------------------------- the restatement's own chain
def chain(X, z0, K0, maxK, a, beta, gamma, e, log_prior_k, scans, n, rng, sweeps=True, ea_moves=1, as_moves=1):
    """n iterations from (K0, z0) on the CPU: `ea_moves` eject / absorb moves, `as_moves` split-merge moves, then
    (sweeps) one batch-1 sweep; returns the visited (K, canonical partition) and the move's five counters"""
    z, K = np.asarray(z0, dtype=np.int64).copy(), K0
    seen, st = [], dict(proposed_splits=0, accepted_splits=0, proposed_merges=0, accepted_merges=0, skipped=0)
    for _ in range(n):
        for _ in range(ea_moves):
            r = al.move(X, z, K, maxK, a, beta, gamma, e, log_prior_k, al.RngDraws(rng))
            z, K = r["z"], r["K"]
        for _ in range(as_moves):
            r = move(X, z, K, maxK, a, beta, gamma, log_prior_k, scans, sm.RngDraws(rng), diagnostics=False)
            z, K = r["z"], r["K"]
            if r["kind"] == SKIPPED:
                st["skipped"] += 1
            else:
                st["proposed_%ss" % r["kind"]] += 1
                st["accepted_%ss" % r["kind"]] += int(r["accepted"])
        if sweeps:
            for i in range(len(z)):
                z[i] = rng.choice(K, p=al.conditional(X, z, i, K, a, beta, gamma))
        seen.append((K, sm.canon(z)))
    return seen, st


# ---------------------------------------------------------------- the same chain at sizes where a sweep must be quick
def sweep_batch1(X, z, K, a, beta, gamma, rng):
    """one batch-1 sweep of alloc_ref.conditional over all rows, on running counts (in place)"""
    X = np.asarray(X, dtype=np.int64)
    N, P = X.shape
    Nk = np.bincount(z, minlength=K)[:K].astype(np.float64)
    S = np.zeros((K, P))
    np.add.at(S, z, X)
    bg = beta + gamma
    U = rng.random(N)
    for i in range(N):
        x = X[i]
        Nk[z[i]] -= 1.0
        S[z[i]] -= x
        lw = np.log(Nk + a) + np.where(x == 1, np.log(beta + S), np.log(gamma + Nk[:, None] - S)).sum(1) - P * np.log(bg + Nk)
        w = np.cumsum(np.exp(lw - lw.max()))
        k = min(int(np.searchsorted(w, U[i] * w[-1], side="right")), K - 1)
        z[i] = k
        Nk[k] += 1.0
        S[k] += x
    return z


def planted_chain(X, z0, K0, maxK, a, beta, gamma, e, log_prior_k, scans, sweeps, rng, ea_moves=1, as_moves=2):
    """`sweeps` sweeps from (K0, z0), the moves ahead of every sweep from the second as a run places them; returns the
    number of non-empty labels after every sweep"""
    z, K = np.asarray(z0, dtype=np.int64).copy(), K0
    used = []
    for j in range(1, sweeps + 1):
        if j >= 2:
            for _ in range(ea_moves):
                r = al.move(X, z, K, maxK, a, beta, gamma, e, log_prior_k, al.RngDraws(rng))
                z, K = r["z"], r["K"]
            for _ in range(as_moves):
                r = move(X, z, K, maxK, a, beta, gamma, log_prior_k, scans, sm.RngDraws(rng), diagnostics=False)
                z, K = r["z"], r["K"]
        z = sweep_batch1(X, z, K, a, beta, gamma, rng)
        used.append(len(np.unique(z)))
    return used
