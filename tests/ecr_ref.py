"""NumPy restatement of the ECR relabelling (include/bmm_mcmc.h "ECR"), written from the
definitions; the device kernels (csrc/kernels.hip.h, k_ecr_*) must match it exactly -- every quantity is an integer.

Labels are 0-based here.  z is S x N with labels in 0 .. K-1, c a pivot of N labels.
  table        n_t[a, b] = #{i : z_t[i] = a, c[i] = b}
  permutation  perm_t = stephens_ref.hungarian(-n_t.T): rows of the cost are pivot labels, columns draw labels, and
               perm_t[l] = the row assigned to column l = the pivot label draw label l leaves as (z = perm[z])
  agreement    agree_t = sum_a n_t[a, perm_t[a]]
  votes        c[i] = the label with the most votes among perm_t[z_t[i]], the lowest label on a tie
  iteration    perm = identity; repeat votes, tables, permutations, total = sum_t agree_t; stop after the first
               iteration whose total equals the previous one (converged) or after max_iter (not converged).
"""
import itertools

import numpy as np

from stephens_ref import hungarian


def tables(z, c, K):
    """(S, K, K) uint32: n[t, a, b]."""
    S, N = z.shape
    n = np.zeros((S, K, K), dtype=np.uint32)
    for t in range(S):
        np.add.at(n[t], (z[t], c), 1)
    return n


def permutations(n):
    """(S, K) int32: perm_t for every table."""
    return np.stack([hungarian(-n[t].T.astype(np.float64)) for t in range(n.shape[0])]).astype(np.int32)


def agreement(n, perm):
    K = n.shape[1]
    return np.array([int(n[t][np.arange(K), perm[t]].astype(np.int64).sum()) for t in range(n.shape[0])], dtype=np.int64)


def votes(z, perm, K):
    """(N,) int32: the majority label of perm_t[z_t[i]] over the rows, lowest label on a tie."""
    S, N = z.shape
    cnt = np.zeros((K, N), dtype=np.int64)
    for t in range(S):
        np.add.at(cnt, (perm[t][z[t]], np.arange(N)), 1)
    return np.argmax(cnt, axis=0).astype(np.int32)  # first maximum: the lowest label


def ecr(z, K, pivot=None, max_iter=50):
    """The whole call: dict of permutations (S, K), agree (S,), pivot (N,), tables (S, K, K), z (relabelled),
    iterations, converged, totals (the total agreement of every iteration run)."""
    z = np.asarray(z)
    S, N = z.shape
    if pivot is not None:
        c = np.asarray(pivot).astype(np.int32)
        n = tables(z, c, K)
        perm = permutations(n)
        agree = agreement(n, perm)
        its, conv, totals = 1, True, [int(agree.sum())]
    else:
        perm = np.tile(np.arange(K, dtype=np.int32), (S, 1))
        prev, its, conv, totals = -1, 0, False, []
        for it in range(1, max_iter + 1):
            c = votes(z, perm, K)
            n = tables(z, c, K)
            perm = permutations(n)
            agree = agreement(n, perm)
            total = int(agree.sum())
            totals.append(total)
            its = it
            if total == prev:
                conv = True
                break
            prev = total
    zr = np.stack([perm[t][z[t]] for t in range(S)]).astype(np.int32)
    return {"permutations": perm, "agree": agree, "pivot": c, "tables": n, "z": zr, "iterations": its,
            "converged": conv, "totals": totals}


def brute_agree(n):
    """max over all K! permutations of sum_a n[a, perm[a]]."""
    K = n.shape[0]
    return max(int(sum(int(n[a, p[a]]) for a in range(K))) for p in itertools.permutations(range(K)))


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------
def noisy(seed, S, N, K, noise, weights=None, used=None):
    """A true allocation, S noisy copies of it (a share `noise` of the labels redrawn), each under a planted
    permutation s_t: returns (z, truth, s) with z[t] = s[t][noisy copy]."""
    rng = np.random.default_rng(seed)
    Ku = K if used is None else used
    w = np.ones(Ku) / Ku if weights is None else np.asarray(weights, dtype=float) / np.sum(weights)
    truth = rng.choice(Ku, size=N, p=w).astype(np.int32)
    z = np.empty((S, N), dtype=np.int32)
    s = np.empty((S, K), dtype=np.int32)
    for t in range(S):
        row = truth.copy()
        flip = rng.random(N) < noise
        row[flip] = rng.choice(Ku, size=int(flip.sum()), p=w)
        s[t] = rng.permutation(K)
        z[t] = s[t][row]
    return z, truth, s


def make(case):
    """(z, pivot or None) of a case, labels 0-based."""
    kind = case["kind"]
    S, N, K = case["S"], case["N"], case["K"]
    if kind == "noisy":
        z, truth, _ = noisy(case["seed"], S, N, K, case["noise"])
        return z, (truth if case["pivot"] else None)
    if kind == "skewed":  # a few big clusters, most labels empty: many equal (zero) costs
        w = np.array([0.7, 0.2, 0.1])
        z, truth, _ = noisy(case["seed"], S, N, K, case["noise"], weights=w, used=3)
        return z, (truth if case["pivot"] else None)
    if kind == "short_pivot":  # the rows use all K labels, the pivot fewer
        z, _, _ = noisy(case["seed"], S, N, K, case["noise"])
        pivot = (np.arange(N) % max(1, K // 2)).astype(np.int32)
        return z, pivot
    if kind == "identical":  # all rows one allocation
        z, _, _ = noisy(case["seed"], 1, N, K, 0.0)
        return np.repeat(z, S, axis=0), None
    if kind == "equal_cells":  # every cell of every table is N / K^2: the tie rule alone decides
        i = np.arange(N)
        z = np.tile((i % K).astype(np.int32), (S, 1))
        pivot = ((i // K) % K).astype(np.int32)
        return z, pivot
    raise ValueError(kind)


def _c(kind, S, N, K, pivot, seed=1, noise=0.3):
    return {"kind": kind, "S": S, "N": N, "K": K, "pivot": pivot, "seed": seed, "noise": noise}


# Shapes: N in {1, 63, 64, 65, 257, 4099}, K in {1, 2, 3, 20, 63, 64, 65, 88, 89, 128} (the assignment's LDS / global
# forms and its columns per lane; tables in LDS up to 110, vote counters in LDS up to 96), S in {1, 17, 33, 65};
# N = 4099 gives several workgroups along N in both passes, S > 8 several along S.
CASES = [
    _c("noisy", 1, 1, 1, True),
    _c("noisy", 1, 1, 1, False),
    _c("noisy", 17, 63, 2, True, seed=2),
    _c("noisy", 17, 64, 3, False, seed=3),
    _c("noisy", 33, 65, 3, True, seed=4),
    _c("noisy", 65, 257, 20, False, seed=5, noise=0.4),
    _c("noisy", 17, 4099, 20, True, seed=6, noise=0.5),
    _c("noisy", 33, 4099, 3, False, seed=7, noise=0.6),
    _c("noisy", 17, 4099, 63, False, seed=8),
    _c("noisy", 17, 257, 64, True, seed=9),
    _c("noisy", 17, 4099, 65, False, seed=10, noise=0.15),
    _c("noisy", 17, 4099, 88, True, seed=11),
    _c("noisy", 17, 4099, 89, False, seed=12, noise=0.15),
    _c("noisy", 17, 4099, 128, True, seed=13),
    _c("noisy", 17, 4099, 128, False, seed=14, noise=0.15),
    _c("noisy", 5, 65, 128, False, seed=20, noise=0.15),
    _c("noisy", 1, 257, 20, False, seed=15),
    _c("skewed", 33, 4099, 20, True, seed=16),
    _c("skewed", 33, 257, 20, False, seed=17),
    _c("short_pivot", 17, 257, 20, True, seed=18),
    _c("identical", 17, 257, 3, False, seed=19),
    _c("equal_cells", 17, 4 * 9 * 7, 3, True),
    _c("equal_cells", 5, 64 * 64, 64, True),
]


def case_id(case):
    return "%s-S%d-N%d-K%d-%s" % (case["kind"], case["S"], case["N"], case["K"], "pivot" if case["pivot"] else "iter")


_SOLVED = {}


def solved(case):
    """The restatement's answer for a case, computed once and shared (do not modify it)."""
    key = case_id(case) + "-%d" % case["seed"]
    if key not in _SOLVED:
        z, pivot = make(case)
        _SOLVED[key] = (z, pivot, ecr(z, case["K"], pivot, 50))
    return _SOLVED[key]
