"""NumPy restatement of Stephens' relabelling as the reference executes it (src/stephens.cpp), written from the
algorithm: my_stephens_batch (:6-66) and my_stephens_online (:68-94), with lp_solve's assignment replaced by the
Hungarian method and the tie rule of DESIGN.md section 11.  The device kernels (csrc/kernels.hip.h, k_st_*) take
exactly these steps; the tests hold them to each other.

Quirks kept, as the reference runs them:
  - batch threshold `10^(-6)` is an integer XOR (= -16, :24): the loop never converges, it runs maxiter = 100
    iterations unless the criterion is NaN;
  - the batch replaces exact zeros of the whole window by 1e-6 first (:30-31), so Q is built from them too;
  - Q is computed once per iteration, at its start (:36-43); the Q returned is that of the last iteration;
  - batch cost uses log p (:50), online cost uses p (:79);
  - perm(l) = the row assigned to column l (:54-55, :83-84) is not inverted (`perm <- sort_index(perm)` is a
    discarded comparison, :56, :85) but is indexed as if it were (:40, :88);
  - online update Q = (j * (Q + p_reordered)) / (j + 1) (:92), j the sweep index.
"""
import itertools

import numpy as np

MAXITER = 100
MIN_PROB = 0.000001


def _augment(C, u, v, p, i):
    """One step of the Hungarian method: row i (1-based) enters the matching p (p[j] = the row of column j, 0 =
    free; index 0 is the virtual column) along the shortest augmenting path under the potentials u / v, which are
    updated elementwise.  In each scan the free column with the smallest slack wins under strict <, so the lowest
    index wins a tie."""
    K = C.shape[0]
    way = np.zeros(K + 1, dtype=np.int64)
    p[0] = i
    j0 = 0
    minv = np.full(K + 1, np.inf)
    used = np.zeros(K + 1, dtype=bool)
    while True:
        used[j0] = True
        i0 = p[j0]
        cur = (C[i0 - 1, :] - u[i0]) - v[1:]                 # slack of every column, elementwise
        free = ~used[1:]
        upd = free & (cur < minv[1:])
        minv[1:][upd] = cur[upd]
        way[1:][upd] = j0
        cand = np.where(free, minv[1:], np.inf)
        j1 = int(np.argmin(cand)) + 1                         # first minimum: lowest index wins a tie
        delta = cand[j1 - 1]
        if not np.isfinite(delta):
            raise ValueError("non-finite costs")
        u[p[used]] += delta                                   # elementwise: the used columns' rows are distinct
        v[used] -= delta
        minv[~used] -= delta
        j0 = j1
        if p[j0] == 0:
            break
    while True:
        j1 = way[j0]
        p[j0] = p[j1]
        j0 = j1
        if j0 == 0:
            break


def hungarian(C, state=False):
    """Exact min-cost assignment of rows to columns of the K x K cost C (O(K^3) shortest augmenting paths, rows
    added in index order, potentials u / v).  In each scan the free column with the smallest slack wins under
    strict <, so the lowest index wins a tie.  Returns perm with perm[l] = the row assigned to column l (and,
    with state=True, the final (u, v, p) as well)."""
    C = np.asarray(C, dtype=np.float64)
    K = C.shape[0]
    u = np.zeros(K + 1)
    v = np.zeros(K + 1)
    p = np.zeros(K + 1, dtype=np.int64)
    for i in range(1, K + 1):
        _augment(C, u, v, p, i)
    perm = (p[1:] - 1).astype(np.int32)
    return (perm, (u, v, p)) if state else perm


def brute_force(C):
    """All K! assignments: (best cost, set of optimal perms in the perm[l] = row convention)."""
    K = C.shape[0]
    best, arg = np.inf, []
    for rows in itertools.permutations(range(K)):            # rows[l] = row of column l
        c = sum(C[rows[l], l] for l in range(K))
        tol = 1e-12 * max(1.0, abs(c))
        if c < best - tol:
            best, arg = c, [rows]
        elif abs(c - best) <= tol:
            arg.append(rows)
    return best, arg


def terms(p, lq, batch_form):
    """K x N x K array t[k, n, l] = p(n,l) * (a(n,l) - log q(n,k)), a = log p (batch) or p (online); a term with
    p(n,l) == 0 is exactly 0 (an all-zero column costs 0 against every row)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.log(p) if batch_form else p
        t = p[None, :, :] * (a[None, :, :] - lq.T[:, :, None])
    return np.where(p[None, :, :] != 0.0, t, 0.0)


def cost(p, lq, batch_form):
    """C[k, l] = sum_n p(n,l) * (a(n,l) - log q(n,k)) (stephens.cpp:50 batch, :79 online)."""
    if p.shape[0] * p.shape[1] ** 2 <= 4_000_000:
        return terms(p, lq, batch_form).sum(axis=1)
    # large: the per-column term split off (allowed, it changes rounding only)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.log(p) if batch_form else p
        pa = np.where(p != 0.0, p * a, 0.0).sum(axis=0)
        lqz = np.where(np.isfinite(lq), lq, 0.0)
    return pa[None, :] - lqz.T @ p


def cost_scale(p, lq, batch_form):
    """sum_n |term| per entry: the scale of the rounding of a cost (the tests' tolerance is 1e-12 of it)."""
    if p.shape[0] * p.shape[1] ** 2 <= 4_000_000:
        return np.abs(terms(p, lq, batch_form)).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.log(p) if batch_form else p
        pa = np.abs(np.where(p != 0.0, p * a, 0.0)).sum(axis=0)
    return pa[None, :] + np.abs(lq).T @ p


def cost_blocked(p, lq, batch_form, block=1024, wide=False):
    """cost() for many rows without the reference's own rounding growing with N: row blocks of at most `block`
    rows, fp64 inside a block (as cost() does), the blocks added in np.longdouble -- the error stays below
    block * 2^-53 of cost_scale whatever N is.  wide: np.longdouble throughout (small K only: K x N x K terms)."""
    N, K = p.shape
    if wide:
        pw, lw = p.astype(np.longdouble), lq.astype(np.longdouble)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.log(pw) if batch_form else pw
            t = pw[None, :, :] * (a[None, :, :] - lw.T[:, :, None])
        return np.where(pw[None, :, :] != 0, t, 0).sum(axis=1).astype(np.float64)
    total = np.zeros((K, K), dtype=np.longdouble)
    for r0 in range(0, N, block):
        total += cost(p[r0:r0 + block], lq[r0:r0 + block], batch_form)
    return total.astype(np.float64)


def cost_scale_blocked(p, lq, batch_form, block=1024):
    """cost_scale() over row blocks (sums of non-negative terms: plain fp64 addition of the blocks)."""
    N, K = p.shape
    total = np.zeros((K, K))
    for r0 in range(0, N, block):
        total += cost_scale(p[r0:r0 + block], lq[r0:r0 + block], batch_form)
    return total


def _duplicated(A):
    """dup[i]: row i of A equals another row exactly"""
    return np.array([any(np.array_equal(A[i], A[r]) for r in range(A.shape[0]) if r != i) for i in range(A.shape[0])])


def margin(C, perm):
    """Smallest increase of the optimum when one of its (row, column) pairs is forbidden: how far the assignment
    is from a tie.  Pairs whose row or column has an exact duplicate in C are left out: swapping duplicates is a
    tie by construction (all-zero columns of p; rows of Q that are all 1e-6, a label empty over the whole batch
    window), computed bit-identically by any evaluation and resolved by the tie rule.  inf for K = 1."""
    K = C.shape[0]
    best = sum(C[perm[l], l] for l in range(K))
    big = np.abs(C).max() * (K + 1) + 1.0
    dup_row, dup_col = _duplicated(C), _duplicated(C.T)
    m = np.inf
    for l in range(K):
        if K == 1 or dup_col[l] or dup_row[perm[l]]:
            continue
        D = C.copy()
        D[perm[l], l] = big
        pp = hungarian(D)
        m = min(m, sum(D[pp[c], c] for c in range(K)) - best)
    return m


def margin_warm(C, perm=None):
    """margin() without solving K assignments from scratch: the same quantity from the optimal potentials.  With
    the pair (row r, column l) of the optimum forbidden, u / v stay feasible and every other pair of the matching
    stays tight, so one augmentation of row r from that state (column l the only free one) yields the optimum of
    the restricted problem.  tests/test_stephens_ref.py holds it to margin()."""
    C = np.asarray(C, dtype=np.float64)
    K = C.shape[0]
    opt, (u, v, p) = hungarian(C, state=True)
    if perm is not None and not np.array_equal(opt, perm):
        raise ValueError("perm is not the restatement's assignment of C")
    best = sum(C[opt[l], l] for l in range(K))
    big = np.abs(C).max() * (K + 1) + 1.0
    dup_row, dup_col = _duplicated(C), _duplicated(C.T)
    m = np.inf
    for l in range(K):
        if K == 1 or dup_col[l] or dup_row[opt[l]]:
            continue
        D = C.copy()
        D[opt[l], l] = big
        uu, vv, pp = u.copy(), v.copy(), p.copy()
        pp[l + 1] = 0
        _augment(D, uu, vv, pp, int(opt[l]) + 1)
        m = min(m, sum(D[pp[c + 1] - 1, c] for c in range(K)) - best)
    return m


def tie_inputs(D):
    """(Q, p) of an online step whose cost matrix is chosen by the caller, bit for bit: N = K, p = I and
    Q = exp2(D.T) give C[k, l] = fl(1 - log Q[l, k]) -- every other term of the sum is an exact 0.0, and x + 0.0 = x
    through any order of partial sums.  Equal entries of D give bit-equal costs, so any tie pattern can be laid
    under the assignment; a larger D is a cheaper pair (C = 1 - D log 2)."""
    D = np.asarray(D, dtype=np.float64)
    K = D.shape[0]
    return np.asfortranarray(np.exp2(D.T)), np.asfortranarray(np.eye(K))


def crafted_ties(K):
    """Tie patterns for tie_inputs with the permutation the tie rule must give, as [(name, D, perm)].  D is 0
    except where a pair is made cheaper (1) -- see tie_inputs.  Every expected permutation follows from: rows
    enter in index order, and among columns of equal slack the lowest index is taken first.
      constant      every assignment ties: each row takes the lowest free column, the identity
      cyclic        the one cheap pair of row k is column (k + 1) % K: perm[l] = (l - 1) % K
      antidiagonal  the one cheap pair of row k is column K - 1 - k
      registers     (K > 68) the last row is equally cheap in columns 3 and 67, which one lane of the device kernel
                    holds in two registers.  Column 3 is taken; its row 3 moves to the one free column, K - 1
      registers3    (K = 128) row 126 is equally cheap in columns 63 and 127: lane 0's second and third register,
                    the only lane with three.  Column 63 is taken and row 63 moves to column 126, the lowest free
                    one (column 127 is free as well and as cheap for row 126: a tie with a free column)
      lanes         (K > 71) the last row is equally cheap in columns 70 and 9: different lanes, column 70 in its
                    lane's second register.  Column 9 is taken, row 9 moves to column K - 1."""
    ident = np.arange(K)
    out = [("constant", np.zeros((K, K)), ident.copy())]
    if K >= 2:
        D = np.zeros((K, K))
        D[ident, (ident + 1) % K] = 1.0
        out.append(("cyclic", D, (ident - 1) % K))
        D = np.zeros((K, K))
        D[ident, K - 1 - ident] = 1.0
        out.append(("antidiagonal", D, K - 1 - ident))

    def one_cheap_row(r, cols):
        D = np.zeros((K, K))
        D[r, cols] = 1.0
        want = ident.copy()
        want[min(cols)], want[r] = r, min(cols)
        return D, want

    if K > 68:
        out.append(("registers",) + one_cheap_row(K - 1, [3, 67]))
    if K == 128:
        out.append(("registers3",) + one_cheap_row(126, [63, 127]))
    if K > 71:
        out.append(("lanes",) + one_cheap_row(K - 1, [70, 9]))
    return out


def online(Q, p, j):
    """my_stephens_online (stephens.cpp:68-94) -> (perm, Q_new, C)."""
    Q = np.asarray(Q, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore"):
        lq = np.log(Q)
    C = cost(p, lq, False)
    perm = hungarian(C)
    Qn = (float(j) * (Q + p[:, perm])) / float(j + 1)        # add, multiply, divide (:92)
    return perm, Qn, C


def batch(p, maxiter=MAXITER, on_iter=None):
    """my_stephens_batch (stephens.cpp:6-66) -> (Q of the last iteration's start, perm M x K of the last
    iteration, iterations run).  on_iter(t, q, perm_before, costs) is called once per iteration."""
    p = np.array(p, dtype=np.float64)
    N, K, M = p.shape
    p[p == 0] = MIN_PROB                                      # p.replace(0, min_prob) (:31)
    perm = np.tile(np.arange(K, dtype=np.int32), (M, 1))
    previous, criterion, threshold = -99.0, 99.0, float(10 ^ (-6))   # = -16.0 (:22-24)
    t = 0
    q = None
    while criterion > threshold and t < maxiter:
        t += 1
        q = np.zeros((N, K))
        for it in range(M):                                   # q.col(k) += p.slice(iter).col(perm(iter,k))
            q += p[:, perm[it], it]
        q = q / M
        lq = np.log(q)
        costs = []
        before = perm.copy()
        for it in range(M):
            C = cost(p[:, :, it], lq, True)
            costs.append(C)
            perm[it] = hungarian(C)                           # not inverted (:56)
        sol = np.zeros((K, K))
        sol[perm[M - 1], np.arange(K)] = 1.0
        current = float(np.sum(costs[-1] * sol))              # accu(cost_matrix % solution) of the last slice
        criterion = abs(previous - current)
        previous = current
        if on_iter is not None:
            on_iter(t, q, before, costs)
    return q, perm, t


class Stephens:
    """The restatement behind the hook path of the package (stephens=<this>): batch(p) -> Q, online(Q, p, j)
    -> (perm, Q_new).  Records the smallest optimality margin it met (relative to the cost scale), so that a
    test can assert its comparisons are far from ties."""

    def __init__(self):
        self.min_margin = np.inf
        self.batch_perm = None

    def _note(self, C, perm, scale, p):
        m = margin(C, perm)
        self.min_margin = min(self.min_margin, m / max(float(scale.max()), 1e-300))

    def batch(self, p):
        p = np.asarray(p, dtype=np.float64)
        last = {}

        def keep(t, q, before, costs):
            last["q"], last["costs"] = q, costs

        q, perm, _ = batch(p, on_iter=keep)
        pr = np.where(p == 0, MIN_PROB, p)
        lq = np.log(last["q"])
        for it in range(p.shape[2]):
            self._note(last["costs"][it], perm[it], cost_scale(pr[:, :, it], lq, True), pr[:, :, it])
        self.batch_perm = perm
        return q

    def online(self, Q, p, j):
        p = np.array(p, dtype=np.float64)
        perm, Qn, C = online(Q, p, j)
        with np.errstate(divide="ignore"):
            self._note(C, perm, cost_scale(p, np.log(Q), False), p)
        return perm, Qn
