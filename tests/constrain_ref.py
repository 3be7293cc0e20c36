"""Constrained allocations (include/bmm_mcmc.h "constraints"), restated in Python from the oracle's
primitives: the per-row conditionals (oracle.collapsed_cond / dp_cond / sb_cond, spec=True), the draw's uniform
(oracle.z_uniform) and the inverse-CDF draw every restatement here uses (tests/test_oracle_alloc.py _draw).

`sweep` is one batched sweep with the revert and the two counters, `project_start` the rule of the starting labels,
`sweep_alpha` the concentration's update behind a counting sweep.  Labels are 1-based as the oracle's are, 0 (or any
value below 1) marks a row without a label; masks are 64-bit, bit k for label k + 1.  The second half states WHAT is
sampled: the exact kernels of the constrained row update on a 7-row data set.
"""
import itertools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from scipy.special import betaln, gammaln

# the per-row conditionals recount the statistics on every call and hold no Python lock while they do: the rows of one
# batch, which all see the same frozen state, go to a few threads
_POOL = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))


# ---------------------------------------------------------------- the lists
def allowed_labels(mask):
    """the 1-based labels of a mask, ascending"""
    return [k + 1 for k in range(64) if (int(mask) >> k) & 1]


def known_list(known):
    """(rows, masks) of N known labels: 0 marks a free row"""
    known = np.asarray(known, dtype=np.int64)
    rows = np.flatnonzero(known > 0).astype(np.int64)
    return rows, (np.uint64(1) << (known[rows] - 1).astype(np.uint64)).astype(np.uint64)


def set_list(allowed):
    """(rows, masks) of an N x K boolean array: a row that is all True is free"""
    A = np.asarray(allowed, dtype=bool)
    rows = np.flatnonzero(~A.all(axis=1)).astype(np.int64)
    masks = np.array([sum(1 << k for k in np.flatnonzero(A[i])) for i in rows], dtype=np.uint64)
    return rows, masks


def project_start(z0, rows, masks):
    """the starting labels inside the rows' sets: a listed row whose label z0 (0-based) is not allowed takes its
    (z0 mod |A_i|)-th allowed label, counted from the lowest"""
    z = np.array(z0, dtype=np.int32)
    for i, m in zip(rows, masks):
        A = allowed_labels(m)
        if z[i] >= 1 and z[i] not in A:
            z[i] = A[(int(z[i]) - 1) % len(A)]
    return z


# ---------------------------------------------------------------- one sweep
def draw(oracle, score, u):
    """the oracle's draw_index over scores_to_weights: the number of k with u * total >= c_k; -1 without a finite score"""
    m = score.max()
    if not m > -np.inf:
        return -1
    c = np.cumsum(oracle.expw_array(score - m))  # (sequential, in label order)
    n = int((u * c[-1] >= c).sum())
    return n if n < len(score) else -1


def batches(sampler, N, batch, j):
    """the launch ranges of sweep j: uniform batches, the DP's first sweep seating 1, 1, 2, 4, ... rows; one exact
    launch for the samplers that carry (pi, theta)"""
    if sampler in ("stickbreaking", "full"):
        return [(0, N)]
    out, lo = [], 0
    while lo < N:
        ln = batch
        if sampler == "dp" and j == 1:
            ln = min(ln, max(1, lo))
        out.append((lo, min(N, lo + ln)))
        lo = out[-1][1]
    return out


def _dp_label(pick, zo, nk, K):
    """the label a DP row takes when it draws the new-cluster option, against the sizes frozen at batch start"""
    if pick != K:
        return pick
    used = int((nk > 0).sum())
    free = np.flatnonzero(nk == 0)
    new = int(free[0]) if len(free) else -1
    own_single = zo >= 0 and nk[zo] == 1
    if used - int(own_single) < K - 1:
        return zo if own_single and (new < 0 or zo < new) else new
    sz = nk - (np.arange(K) == zo)
    live = np.flatnonzero(sz > 0)
    return int(live[np.argmin(sz[live])]) if len(live) else max(zo, 0)


def propose(oracle, sampler, X, frozen, i, j, K, alpha, beta, gamma, seed, pi=None, theta=None, nk=None):
    """the unconstrained draw of row i in sweep j under the frozen state, 1-based"""
    zo = int(frozen[i]) - 1 if frozen[i] >= 1 else -1
    if sampler == "collapsed":
        score, _ = oracle.collapsed_cond(X, frozen, i, K, alpha, beta, gamma, spec=True)
    elif sampler == "dp":
        score, _ = oracle.dp_cond(X, frozen, i, K, alpha, beta, gamma, spec=True)
    else:
        score, _ = oracle.sb_cond(X, i, pi, theta, spec=True)
    pick = draw(oracle, score, oracle.z_uniform(seed, i, j))
    if pick < 0:
        pick = max(zo, 0)
    if sampler == "dp":
        pick = _dp_label(pick, zo, nk, K)
    return pick + 1


def revert(z_in, z_drawn, rows, masks, lo, hi, stats):
    """the constraint on a launch range: a listed row drawn outside its set goes back to the label it had, to its
    lowest allowed label where it had none.  stats = [proposed, reverted] is updated; returns the labels."""
    z = np.array(z_drawn)
    for i, m in zip(rows, masks):
        if not lo <= i < hi:
            continue
        stats[0] += 1
        A = allowed_labels(m)
        if z[i] not in A:
            stats[1] += 1
            z[i] = z_in[i] if z_in[i] >= 1 else A[0]
    return z


def sweep(oracle, sampler, X, z, j, K, alpha, beta, gamma, seed, batch, rows, masks, stats, pi=None, theta=None):
    """sweep j from the labels z (1-based, < 1: no label): every launch range drawn under the state frozen at its
    start, then reverted.  Returns the new labels."""
    X = np.asfortranarray(X, dtype=np.int32)
    N = X.shape[0]
    z_in = np.where(np.asarray(z) >= 1, z, 0).astype(np.int32)
    cur = z_in.copy()
    for lo, hi in batches(sampler, N, batch, j):
        frozen = cur.copy()
        nk = np.bincount(frozen[frozen >= 1] - 1, minlength=K) if sampler == "dp" else None
        got = list(_POOL.map(lambda i: propose(oracle, sampler, X, frozen, i, j, K, alpha, beta, gamma, seed, pi, theta, nk),
                             range(lo, hi)))
        drawn = cur.copy()
        drawn[lo:hi] = got
        cur = revert(z_in, drawn, rows, masks, lo, hi, stats)
    return cur


def sweep_alpha(oracle, sampler, alpha, a, b, N, K, z, seed, j):
    """the concentration after counting sweep j (a chain created with alpha = 0 samples it): the finite sampler passes
    K, the DP the number of labels in use"""
    kc = K if sampler == "collapsed" else len(set(int(v) for v in z if v >= 1))
    return oracle.update_alpha(alpha, a, b, N, kc, seed, j)


def recount(X, z, K):
    """(Nk, S) under 1-based labels"""
    X, z = np.asarray(X), np.asarray(z)
    Nk = np.array([(z == k + 1).sum() for k in range(K)], dtype=np.int64)
    S = np.stack([X[z == k + 1].sum(axis=0) for k in range(K)]).astype(np.int64)
    return Nk, S


# ---------------------------------------------------------------- what is sampled: the 7-row set and its exact kernels
def seven_rows():
    """7 rows, P = 4: two loose groups"""
    return np.array([[1, 1, 0, 1], [0, 0, 1, 0], [1, 0, 0, 1], [1, 1, 1, 1], [0, 0, 1, 1], [0, 1, 0, 0], [1, 1, 0, 0]], dtype=np.int32)


SEVEN_KNOWN = np.array([1, 2, 0, 0, 0, 0, 0])  # rows 0 and 1 hold labels 1 and 2 ...
SEVEN_SET_ROW, SEVEN_SET = 2, (1, 2)            # ... and row 2 may take either of them


def seven_lists(K):
    """(rows, masks) of the 7-row set's constraints"""
    A = np.ones((7, K), dtype=bool)
    A[SEVEN_SET_ROW] = False
    A[SEVEN_SET_ROW, [k - 1 for k in SEVEN_SET]] = True
    for i, k in enumerate(SEVEN_KNOWN):
        if k:
            A[i] = False
            A[i, k - 1] = True
    return set_list(A)


def _block_loglik(X, rows, beta, gamma):
    n, s = len(rows), X[rows].sum(axis=0)
    return float(np.sum(betaln(beta + s, gamma + n - s) - betaln(beta, gamma)))


def finite_log_target(X, z, K, alpha, beta, gamma):
    """the finite mixture with Dirichlet(alpha / K) weights integrated out, z 0-based"""
    z = np.asarray(z)
    n = np.bincount(z, minlength=K)
    lp = float(np.sum(gammaln(alpha / K + n) - gammaln(alpha / K)))
    return lp + sum(_block_loglik(X, np.flatnonzero(z == k), beta, gamma) for k in range(K) if n[k])


def finite_conditional(X, z, i, K, alpha, beta, gamma):
    """p(z_i = k | the other rows) of that model"""
    z = np.array(z)
    lw = np.empty(K)
    for k in range(K):
        z[i] = k
        lw[k] = finite_log_target(X, z, K, alpha, beta, gamma)
    w = np.exp(lw - lw.max())
    return w / w.sum()


def finite_states(K, rows, masks):
    """every allocation of the 7 rows (0-based) that satisfies the constraints"""
    sets = [list(range(K))] * 7
    for i, m in zip(rows, masks):
        sets[i] = [k - 1 for k in allowed_labels(m)]
    return list(itertools.product(*sets))


def constrained_row_matrix(states, cond, i, allowed):
    """the exact transition matrix of the constrained update of row i over `states`: the proposal is cond(z, i) over
    every label, a proposal outside `allowed` (None: a free row) leaves the state where it is"""
    index = {s: k for k, s in enumerate(states)}
    T = np.zeros((len(states), len(states)))
    for zt in states:
        p = cond(zt, i)
        for k, pk in enumerate(p):
            if allowed is None or k in allowed:
                T[index[zt], index[zt[:i] + (k,) + zt[i + 1:]]] += pk
            else:
                T[index[zt], index[zt]] += pk
    return T


def restricted(states, log_target):
    lw = np.array([log_target(z) for z in states])
    w = np.exp(lw - lw.max())
    return w / w.sum()


# the DP: partitions of the 7 rows.  A known row holds its label for ever, so the block it sits in carries that label;
# a state is consistent when the known rows with different labels sit in different blocks and every row with a set sits
# in the block of one of its labels' holders.
def canonical(z):
    seen, out = {}, []
    for v in z:
        out.append(seen.setdefault(int(v), len(seen)))
    return tuple(out)


def partitions(n):
    out = []

    def grow(prefix, top):
        if len(prefix) == n:
            out.append(tuple(prefix))
            return
        for k in range(top + 2):
            grow(prefix + [k], max(top, k))
    grow([0], 0)
    return out


def dp_consistent(part, known=SEVEN_KNOWN, set_row=SEVEN_SET_ROW, set_labels=SEVEN_SET):
    holder = {int(k): i for i, k in enumerate(known) if k}
    blocks = [part[i] for i in holder.values()]
    if len(set(blocks)) != len(blocks):
        return False
    return set_row is None or part[set_row] in [part[holder[k]] for k in set_labels]


def dp_log_target(X, part, alpha, beta, gamma):
    z = np.asarray(part)
    return sum(np.log(alpha) + gammaln((z == k).sum()) + _block_loglik(X, np.flatnonzero(z == k), beta, gamma)
               for k in range(z.max() + 1))


def dp_row_matrix(X, states, i, alpha, beta, gamma, known=SEVEN_KNOWN, set_row=SEVEN_SET_ROW, set_labels=SEVEN_SET):
    """the constrained DP update of row i over the consistent partitions: the proposal is the CRP conditional over the
    other rows' blocks and a new one; a known row reverts every proposal that is not its own block (the block's label
    would be another), the row with a set every proposal that is not a block of one of its labels' holders"""
    index = {s: k for k, s in enumerate(states)}
    holder = {int(k): r for r, k in enumerate(known) if k}
    T = np.zeros((len(states), len(states)))
    for part in states:
        z = np.array(part)
        others = [b for b in sorted(set(part[:i] + part[i + 1:]))]
        opts, lw = [], []
        for b in others + [max(part) + 1]:
            z2 = z.copy()
            z2[i] = b
            opts.append(canonical(z2))
            lw.append(dp_log_target(X, canonical(z2), alpha, beta, gamma))
        w = np.exp(np.array(lw) - max(lw))
        w /= w.sum()
        for b, to, pk in zip(others + [None], opts, w):
            if known[i]:
                ok = to == part
            elif i == set_row:
                ok = b is not None and b in [part[holder[k]] for k in set_labels]
            else:
                ok = True
            T[index[part], index[to] if ok else index[part]] += pk
    return T


def literal_chain(cond_table, K, rows, masks, z0, sweeps, rng):
    """a batch-1 chain of the constrained finite update with NumPy uniforms over a table of exact conditionals
    (cond_table[i][the state with row i set to label 0] = p over labels): the codes of the visited states, base K.
    The move is `revert`'s: a draw outside the set keeps the label."""
    N = len(z0)
    allowed = {int(i): [k - 1 for k in allowed_labels(m)] for i, m in zip(rows, masks)}
    z = list(z0)
    pw = K ** np.arange(N - 1, -1, -1)
    code = int(np.dot(z, pw))
    out = np.empty(sweeps, dtype=np.int64)
    U = rng.random((sweeps, N))
    for t in range(sweeps):
        for i in range(N):
            base = code - z[i] * int(pw[i])
            c = cond_table[i][base]
            k = int(np.searchsorted(c, U[t, i], side="right"))
            k = min(k, K - 1)
            if i in allowed and k not in allowed[i]:
                continue
            z[i] = k
            code = base + k * int(pw[i])
        out[t] = code
    return out
