"""NumPy restatement of the credible ball and the row-to-cluster similarity of include/bmm_mcmc.h ("credible ball"),
over partition_ref: the distance of every draw to a centre, the ball with its radius and three bounds written from the
definitions, and sim[i][a] = sum_t T_t[a][z_t,i].  Labels are 1-based, rows of an (S, N) integer array, as the
library's z; the centre has labels in 1 .. Ka.  Everything Binder and every count is in Python integers (exact)."""
import math

import numpy as np

import partition_ref as pr
import partition_search_ref as psr


def distances(c, z, Kc, criterion):
    """(d2, D, k) per draw: d2_t = 2 B(c, z_t) as Python integers; D_t the criterion's distance in its natural unit
    (B as a Python integer, or partition_ref.vi: VI in nats); k_t the non-empty labels of draw t.  Kc: at least every
    label of c and of z."""
    z = np.asarray(z)
    d2 = [pr.binder2(c, row, Kc) for row in z]
    D = [v // 2 for v in d2] if criterion == "binder" else [pr.vi(c, row, Kc) for row in z]
    k = [len(np.unique(row)) for row in z]
    return d2, D, k


def _bound(D, k, ball, kk):
    """among the draws of the ball (with k_t = kk, or any for kk None) those with the largest D_t: the lowest, how many,
    its k"""
    pool = [t for t in ball if kk is None or k[t] == kk]
    top = max(D[t] for t in pool)
    at = [t for t in pool if D[t] == top]
    return {"sweep": at[0], "ties": len(at), "n_clusters": k[at[0]]}


def ball(D, k, level):
    """The credible ball from the distances D_t (compared as they are given) and the cluster counts k_t: the draws
    ordered by (D_t, t), m = min(S, max(1, ceil(level S))), the radius the D of the m-th, the ball {t : D_t <= radius};
    then the horizontal bound (largest D in the ball) and the vertical upper and lower bounds (largest D among the
    ball's draws with the smallest and with the largest k), each the lowest such t and the number of them."""
    S = len(D)
    order = sorted(range(S), key=lambda t: (D[t], t))
    m = min(S, max(1, math.ceil(level * S)))
    at = order[m - 1]
    radius = D[at]
    inside = [t for t in range(S) if D[t] <= radius]
    return {"m": m, "at": at, "radius": radius, "n_in": len(inside),
            "horizontal": _bound(D, k, inside, None),
            "upper": _bound(D, k, inside, min(k[t] for t in inside)),
            "lower": _bound(D, k, inside, max(k[t] for t in inside))}


def sim(c, z, Ka):
    """sim[i][a] = sum_t T_t[a][z_t,i] = sum_t #{j : c_j = a, z_t,j = z_t,i}: (N, Ka) of Python integers"""
    c = np.asarray(c, dtype=np.int64) - 1
    z = np.asarray(z, dtype=np.int64) - 1
    S, N = z.shape
    Kc = int(z.max()) + 1
    out = np.zeros((N, Ka), dtype=np.int64)
    for row in z:
        T = np.bincount(c * Kc + row, minlength=Ka * Kc).reshape(Ka, Kc)
        out += T[:, row].T
    return out.astype(object)


def membership(s, c, S):
    """(sim - S own) / (S (n_a - own)) from the definitions, one cell at a time; NaN where the denominator is 0"""
    c = np.asarray(c, dtype=np.int64) - 1
    N, Ka = s.shape
    n = np.bincount(c, minlength=Ka)
    out = np.full((N, Ka), np.nan)
    for i in range(N):
        for a in range(Ka):
            own = int(a == c[i])
            den = S * (int(n[a]) - own)
            if den > 0:
                out[i, a] = (int(s[i, a]) - S * own) / den
    return out


# The shapes the device is held to (tests/test_gpu_credible_ball.py), and that tests/test_credible_ball_cpu.py feeds to
# the plan to prove that they reach every form it can name: (Kc, Ka, N, S, subset rows).
CASES = [
    (3, 5, 257, 17, 7),      # two empty slots, N no multiple of the workgroup or of 16
    (20, 24, 4099, 70, 9),   # three threads per row
    (64, 64, 1000, 9, 5),    # LDS bounds D: several blocks of draws
    (2, 2, 64, 300, 3),      # duplicated rows: ties at the radius
]


def case_id(case):
    return "Kc%d-Ka%d-N%d-S%d" % case[:4]


def case_trace(case):
    """(z, centre, subset) of a case: a noisy trace around a truth; the centre is draw 1 renumbered into 1 .. Kc (the
    slots above stay empty); the last shape repeats every row of a short trace, so that distances tie"""
    Kc, Ka, N, S, m = case
    seed = 1000 + Kc
    if S == 300:
        base = psr.make_trace(Kc, N, 30, 0.2, seed)[0]
        z = np.asfortranarray(np.tile(base, (10, 1)), dtype=np.int32)
    else:
        z = psr.make_trace(Kc, N, S, 0.15, seed)[0]
    centre = np.ascontiguousarray(z[1], dtype=np.int32)
    rng = np.random.default_rng(seed + 1)
    subset = rng.integers(0, N, m)
    subset[-1] = subset[0]  # a repeated index
    return z, centre, subset.astype(np.int64)
