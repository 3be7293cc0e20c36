"""NumPy restatement of the partition summaries of include/bmm_mcmc.h ("clustering point estimate and posterior
similarity"): Binder and VI distances between label rows, the expected loss of every candidate, the point estimate
with its tie rule, and the posterior similarity counts.  Labels are 1-based, rows of an (S, N) integer array, as the
library's z.  Everything Binder is in Python integers (exact); VI sums with math.fsum (correctly rounded) over
math.log, so that the device's error can be held against a bound and not against another rounding."""
import math

import numpy as np


def contingency(c, z, Kc):
    """n_ab = #{i : c_i = a, z_i = b}, a Kc x Kc int64 table (labels 1-based)"""
    c = np.asarray(c, dtype=np.int64) - 1
    z = np.asarray(z, dtype=np.int64) - 1
    return np.bincount(c * Kc + z, minlength=Kc * Kc).reshape(Kc, Kc)


def _sq(v):
    return sum(int(x) * int(x) for x in np.asarray(v).ravel() if x)


def binder2(c, z, Kc):
    """2 B(c, z) = sum_a n_a.^2 + sum_b n_.b^2 - 2 sum_ab n_ab^2, a Python integer"""
    n = contingency(c, z, Kc)
    return _sq(n.sum(1)) + _sq(n.sum(0)) - 2 * _sq(n)


def binder(c, z, Kc):
    return binder2(c, z, Kc) // 2


def _f(n):
    n = int(n)
    return n * math.log(n) if n else 0.0


def vi(c, z, Kc):
    """VI(c, z) = (sum_a f(n_a.) + sum_b f(n_.b) - 2 sum_ab f(n_ab)) / N, f(n) = n log n; 0 for one partition"""
    n = contingency(c, z, Kc)
    if _sq(n.sum(1)) + _sq(n.sum(0)) - 2 * _sq(n) == 0:
        return 0.0
    terms = [_f(x) for x in n.sum(1)] + [_f(x) for x in n.sum(0)] + [-2.0 * _f(x) for x in n.ravel() if x]
    return math.fsum(terms) / len(np.asarray(c))


def candidates(S, stride):
    return list(range(0, S, stride))


def distances(z, Kc, criterion="binder", stride=1):
    """the C x S matrix: Python integers B (object array) or float VI; the diagonal is 0 by construction"""
    z = np.asarray(z)
    S = z.shape[0]
    cand = candidates(S, stride)
    D = np.zeros((len(cand), S), dtype=object if criterion == "binder" else np.float64)
    for ci, r in enumerate(cand):
        for t in range(S):
            if t == r:
                continue
            D[ci, t] = binder(z[r], z[t], Kc) if criterion == "binder" else vi(z[r], z[t], Kc)
    return D


def binder2_totals(z, Kc, stride=1, D=None):
    """sum_t 2 B(c, z_t) per candidate, Python integers"""
    D = distances(z, Kc, "binder", stride) if D is None else D
    return [2 * sum(int(x) for x in row) for row in D]


def expected_loss(z, Kc, criterion="binder", stride=1, D=None):
    """L(c) per candidate: binder2 / (2 S) (the integer converted once), or the fsum of the VI row over S"""
    S = np.asarray(z).shape[0]
    if criterion == "binder":
        return np.array([float(t) / (2.0 * S) for t in binder2_totals(z, Kc, stride, D)])
    D = distances(z, Kc, "vi", stride) if D is None else D
    return np.array([math.fsum(row) / S for row in D])


def point_estimate(z, Kc, criterion="binder", stride=1, D=None):
    """row of z (0-based) with the smallest expected loss, lowest index on ties (Binder: on the exact integers)"""
    if criterion == "binder":
        tot = binder2_totals(z, Kc, stride, D)
        return stride * min(range(len(tot)), key=lambda i: (tot[i], i))
    return stride * int(np.argmin(expected_loss(z, Kc, "vi", stride, D)))  # argmin: the first minimum


def similarity(z, idx):
    """cnt[u, v] = #{t : z_t[idx_u] = z_t[idx_v]}, uint32 M x M (idx 0-based)"""
    g = np.asarray(z)[:, np.asarray(idx, dtype=np.int64)]
    M = g.shape[1]
    cnt = np.zeros((M, M), dtype=np.uint32)
    for row in g:
        cnt += (row[:, None] == row[None, :])
    return cnt


def binder_brute(c, z):
    """pairs i < j on which the two partitions disagree, counted one by one"""
    c, z = np.asarray(c), np.asarray(z)
    n = 0
    for i in range(len(c)):
        for j in range(i + 1, len(c)):
            n += int((c[i] == c[j]) != (z[i] == z[j]))
    return n


def vi_from_entropies(c, z):
    """H(c) + H(z) - 2 I(c, z) from the definitions, in nats"""
    c, z = np.asarray(c), np.asarray(z)
    N = len(c)

    def H(lab):
        return -math.fsum((m / N) * math.log(m / N) for m in np.unique(lab, return_counts=True)[1])

    pairs, counts = np.unique(np.stack([c, z]), axis=1, return_counts=True)
    info = []
    for (a, b), m in zip(pairs.T, counts):
        pa = np.count_nonzero(c == a) / N
        pb = np.count_nonzero(z == b) / N
        info.append((m / N) * math.log((m / N) / (pa * pb)))
    return H(c) + H(z) - 2.0 * math.fsum(info)


def dahl_least_squares(c, cnt, S):
    """sum_{i<j} (S delta_ij - cnt_ij)^2 against a full similarity matrix, a Python integer"""
    c = np.asarray(c)
    tot = 0
    for i in range(len(c)):
        d = (c[i] == c[i + 1:]).astype(np.int64) * S - cnt[i, i + 1:].astype(np.int64)
        tot += int((d * d).sum())
    return tot


def vi_bound(Kc, N):
    """absolute error allowed to the device's VI against this restatement (the issue's figure): log_ below 1 ulp,
    sums of at most Kc^2 + 2 Kc terms, each N-normalised term at most log N"""
    return 8 * (Kc * Kc + 2 * Kc) * 2.0 ** -52 * math.log(N)


# The shapes the device is held to (tests/test_gpu_partition.py), and that tests/test_partition_cpu.py feeds to the
# plan to prove that they reach every form it can name: (Kc, N, S, stride, criterion, skewed).
CASES = [
    (1, 1, 1, 1, "binder", False),
    (2, 63, 2, 1, "vi", False),
    (3, 64, 3, 3, "binder", True),
    (4, 65, 17, 3, "vi", True),
    (5, 10007, 17, 1, "binder", True),
    (20, 10 ** 6, 17, 1, "binder", True),
    (20, 10 ** 6, 3, 1, "vi", False),
    (21, 10007, 200, 3, "vi", True),
    (32, 10007, 17, 17, "binder", False),
    (33, 65, 17, 1, "vi", False),
    (64, 10007, 3, 1, "binder", True),
    (65, 10007, 17, 1, "vi", True),
    (100, 64, 17, 3, "binder", False),
    (100, 65, 3, 1, "binder", True),
    (65, 63, 17, 17, "vi", False),
    (300, 10007, 3, 1, "binder", True),
    (300, 65, 17, 3, "vi", False),
    (300, 64, 2, 1, "vi", True),
    (300, 63, 17, 17, "binder", False),
    (4, 10007, 200, 1, "binder", True),
]


def make_rows(Kc, N, S, skewed, seed):
    """S label rows (1-based, int32, column-major as the library's z): uniform over the Kc labels, or skewed -- one
    cluster holds 99 % of the observations, the case in which most lanes of a wave hit one bin"""
    rng = np.random.default_rng(seed)
    if Kc == 1:
        lab = np.zeros((S, N), dtype=np.int64)
    elif skewed:
        p = np.full(Kc, 0.01 / (Kc - 1))
        p[0] = 0.99
        lab = rng.choice(Kc, size=(S, N), p=p)
    else:
        lab = rng.integers(0, Kc, size=(S, N))
    return np.asfortranarray(lab + 1, dtype=np.int32)
