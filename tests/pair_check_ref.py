"""NumPy restatement of the pairwise local-dependence check (include/bmm_mcmc.h "pairwise local-dependence check",
DESIGN.md section 22): per label Xk.T @ Xk in int64, then the formulas in plain float64.  Nothing here shares code with
the library; the pair order is numpy.triu_indices(M, 1)."""
import numpy as np

EPS = 2.0 ** -53


def pairs(M):
    return np.triu_indices(M, 1)


def gram(X, z0, Kc, feat):
    """(Kc, M, M) int64: G[k] = Xk.T @ Xk over the chosen features, rows with 0-based label k; (Kc,) rows per label"""
    Xf = np.asarray(X)[:, feat].astype(np.int64)
    G = np.zeros((Kc, len(feat), len(feat)), dtype=np.int64)
    n = np.zeros(Kc, dtype=np.int64)
    for k in range(Kc):
        Xk = Xf[z0 == k]
        G[k] = Xk.T @ Xk
        n[k] = Xk.shape[0]
    return G, n


def counts(X, z0, Kc, feat):
    """c (Kc, npairs), margins s (Kc, M), rows n (Kc,), all int64"""
    G, n = gram(X, z0, Kc, feat)
    i, j = pairs(len(feat))
    return G[:, i, j], np.diagonal(G, axis1=1, axis2=2).copy(), n


def terms(c, s, n):
    """per label and pair a_k = c - E and v_k, float64, zero where n_k < 2: (Kc, npairs) each.  As the definition
    states them: the integers num = c n - s_d s_e, pd = s_d (n - s_d), pe = s_e (n - s_e), nn = n n in int64, each
    converted once, then a_k = num / n and v_k = (pd pe) / (nn (n - 1))."""
    M = s.shape[1]
    i, j = pairs(M)
    c, s, n = c.astype(np.int64), s.astype(np.int64), n.astype(np.int64)
    nc = n[:, None]
    sd, se = s[:, i], s[:, j]
    use = (n >= 2)[:, None]
    num, pd, pe, nn = c * nc - sd * se, sd * (nc - sd), se * (nc - se), nc * nc
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(use, num.astype(np.float64) / nc.astype(np.float64), 0.0)
        v = np.where(use, (pd.astype(np.float64) * pe.astype(np.float64)) / (nn.astype(np.float64) * (nc - 1).astype(np.float64)), 0.0)
    return a, v


def stats_from_counts(c, s, n):
    """{"A", "V", "z", "x2" (npairs,) float64, "df" int32}; z is NaN where V = 0"""
    a, v = terms(c, s, n)
    A, V = a.sum(axis=0), v.sum(axis=0)
    pos = v > 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        x2 = np.where(pos, a * a / np.where(pos, v, 1.0), 0.0).sum(axis=0)
        z = np.where(V > 0.0, A / np.sqrt(np.where(V > 0.0, V, 1.0)), np.nan)
    return {"A": A, "V": V, "z": z, "x2": x2, "df": pos.sum(axis=0).astype(np.int32)}


def stats(X, z0, Kc, feat):
    return stats_from_counts(*counts(X, z0, Kc, feat))


def bounds(c, s, n):
    """The rounding bounds of the fixed arithmetic against this restatement, from the operation count, not tuned.  a_k is
    one correctly rounded division of exact integers on either side and v_k three roundings; a sum of Kc terms adds at
    most Kc - 1 roundings of partial sums that the sum of magnitudes bounds, on either side: |A - A_ref| <= 4 Kc eps
    sum |a_k|, and the same form for V over v_k and for X2 over a_k^2 / v_k.  Z = A / sqrt(V) is then within
    (bA + |A| bV / (2 V)) / sqrt(V) to first order, plus the division and the square root on either side: 4 eps |Z|;
    the first-order term is doubled to cover the second order."""
    a, v = terms(c, s, n)
    Kc = c.shape[0]
    pos = v > 0.0
    sa, sv = np.abs(a).sum(axis=0), v.sum(axis=0)
    A = a.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        sx = np.where(pos, a * a / np.where(pos, v, 1.0), 0.0).sum(axis=0)
        bA, bV = 4 * Kc * EPS * sa, 4 * Kc * EPS * sv
        V1 = np.where(sv > 0.0, sv, 1.0)
        zb = np.where(sv > 0.0, 2.0 * (bA + np.abs(A) * bV / (2.0 * V1)) / np.sqrt(V1) + 4 * EPS * np.abs(A) / np.sqrt(V1), 0.0)
    return {"A": bA, "V": bV, "x2": 4 * Kc * EPS * sx, "z": zb}


def planted(seed, N=4096, P=37, K=3):
    """the data of the calibration and power test: rates uniform on (0.1, 0.9), labels uniform; feature 1 copies feature
    0 in 60 % of cluster 0, feature 3 copies feature 2 in 60 % of cluster 2 and 1 - feature 2 in 60 % of cluster 1.
    Returns X (N, P) int32 and the generating labels (0-based)."""
    rng = np.random.default_rng(seed)
    theta = rng.uniform(0.1, 0.9, (K, P))
    z0 = rng.integers(0, K, N)
    X = (rng.random((N, P)) < theta[z0]).astype(np.int32)
    pick = rng.random((3, N)) < 0.6
    m = (z0 == 0) & pick[0]
    X[m, 1] = X[m, 0]
    m = (z0 == 2) & pick[1]
    X[m, 3] = X[m, 2]
    m = (z0 == 1) & pick[2]
    X[m, 3] = 1 - X[m, 2]
    return X, z0


PLANTED = ((0, 1), (2, 3))
# the bounds of the issue; the worst cases this generator gives over seeds 0..7 are max |Z| 3.67,
# Z(0,1) 7.73, X2(2,3) 734 and max X2 21.1 on the untouched pairs
Z_NULL_MAX, Z_01_MIN, X2_23_MIN, X2_NULL_MAX = 4.5, 5.0, 100.0, 40.0
PLANTED_SEED = 0


def planted_figures(zs, x2s, M=37):
    """(max |Z| untouched, Z(0,1), X2(2,3), max X2 untouched) of (npairs,) vectors over all M features"""
    i, j = pairs(M)
    touched = np.zeros(i.size, dtype=bool)
    for d, e in PLANTED:
        touched |= (i == d) & (j == e)
    q01 = int(np.nonzero((i == 0) & (j == 1))[0][0])
    q23 = int(np.nonzero((i == 2) & (j == 3))[0][0])
    return float(np.nanmax(np.abs(zs[~touched]))), float(zs[q01]), float(x2s[q23]), float(np.max(x2s[~touched]))


def check_planted(zs, x2s, M=37):
    zn, z01, x23, xn = planted_figures(zs, x2s, M)
    print("planted: max |Z| null %.3f  Z(0,1) %.3f  X2(2,3) %.1f  max X2 null %.2f" % (zn, z01, x23, xn))
    assert zn <= Z_NULL_MAX and z01 >= Z_01_MIN and x23 >= X2_23_MIN and xn <= X2_NULL_MAX, (zn, z01, x23, xn)
