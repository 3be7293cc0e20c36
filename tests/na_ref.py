"""Missing data by augmentation (include/bmm_mcmc.h "missing data"), restated in NumPy, and the
runner of tests/na/na_host.cpp, the host statement of one imputation step over bmm_spec.h.

The restatement has the step's integer parts and its uniforms exactly as the device has them (sites, census,
observed-only counts, na_uniform, the S deltas); the auxiliary Beta draw of a counting chain comes from bmm_spec.h's
variate generator, which only the host program and the device share, so where a test needs those bits it takes phi from
the host program.  The reference chains at the end use a NumPy generator for every draw: they state WHAT is sampled.
"""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
from scipy.special import betaln, gammaln

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_merge_ref as smr  # noqa: E402  (Philox as bmm_spec.h)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "na", "na_host.cpp")
INC = os.path.join(ROOT, "bmm-mcmc_amd", "csrc")
_DIR = tempfile.TemporaryDirectory(prefix="na_host_")
STREAM_MISSING = 15  # bmm_spec.h kStreamMissing


# ---------------------------------------------------------------- the step's exact parts
def na_uniform(seed, cell, sweep):
    """bmm_spec.h na_uniform: one Philox4x32 block at (cell lo, cell hi, sweep, stream id) under the seed"""
    r = smr.philox4x32_10((cell & 0xFFFFFFFF, (cell >> 32) & 0xFFFFFFFF, sweep, STREAM_MISSING),
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return smr.u01(r[0], r[1])


def sites(rows, cols):
    """[(row, word, mask, first cell)]: one site per (row, plane word) with a hole, cells sorted by (row, column)"""
    out = []
    for q, (i, j) in enumerate(zip(rows, cols)):
        w = int(j) >> 5
        if not out or out[-1][0] != int(i) or out[-1][1] != w:
            out.append([int(i), w, 0, q])
        out[-1][2] |= 1 << (int(j) & 31)
    return [tuple(s) for s in out]


def pack(X):
    """bit planes [W][N] of an N x P 0/1 matrix, flattened (word w of row i at w * N + i)"""
    X = np.asarray(X)
    N, P = X.shape
    W = (P + 31) // 32
    Xb = np.zeros((W, N), dtype=np.uint64)
    for j in range(P):
        Xb[j >> 5] |= X[:, j].astype(np.uint64) << np.uint64(j & 31)
    return Xb.astype(np.uint32).ravel()


def unpack(Xb, N, P):
    Xb = np.asarray(Xb, dtype=np.uint32).reshape(-1, N)
    return np.stack([(Xb[j >> 5] >> np.uint32(j & 31)) & np.uint32(1) for j in range(P)], axis=1).astype(np.int32)


def recount(X, z, K):
    """(Nk, S) of the matrix under 0-based labels (rows with z < 0 have no seat)"""
    X, z = np.asarray(X), np.asarray(z)
    Nk = np.zeros(K, dtype=np.int64)
    S = np.zeros((K, X.shape[1]), dtype=np.int64)
    for k in range(K):
        Nk[k] = int((z == k).sum())
        S[k] = X[z == k].sum(axis=0)
    return Nk, S


def census(X, z, rows, cols, K):
    """M_kj, the missing cells among label k's rows, and O_kj, how many of them hold a 1"""
    P = np.asarray(X).shape[1]
    M, O = np.zeros((K, P), dtype=np.int64), np.zeros((K, P), dtype=np.int64)
    for i, j in zip(rows, cols):
        k = int(z[i])
        if k < 0:
            continue
        M[k, j] += 1
        O[k, j] += int(X[i, j])
    return M, O


def step_given_phi(X, z, S, rows, cols, phi, seed, sweep):
    """the draw: bit = na_uniform(seed, i * P + j, sweep) < phi[z_i, j]; returns (X', S', bits, u)"""
    X, S = np.array(X), np.array(S)
    P = X.shape[1]
    bits, us = [], []
    for i, j in zip(rows, cols):
        k = int(z[i])
        if k < 0:
            bits.append(int(X[i, j])); us.append(np.nan)
            continue
        u = na_uniform(seed, int(i) * P + int(j), sweep)
        nb = int(u < phi[k, j])
        S[k, j] += nb - int(X[i, j])
        X[i, j] = nb
        bits.append(nb); us.append(u)
    return X, S, np.array(bits, dtype=np.uint8), np.array(us)


# ---------------------------------------------------------------- the host program
@functools.lru_cache(maxsize=None)
def program():
    exe = os.path.join(_DIR.name, "na_host")
    # -ffp-contract=off: as the library is built (bmm_spec.h fuses only where it says fma_)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", INC, SRC, "-o", exe], check=True)
    return exe


def _hex(x):
    return " ".join("%016x" % int(v) for v in np.asarray(x, dtype=np.float64).reshape(-1).view(np.uint64))


def _f64(hexes):
    return np.array([int(h, 16) for h in hexes], dtype=np.uint64).view(np.float64)


def host_step(X, z, Nk, S, rows, cols, seed, sweep, beta, gamma, theta=None, mode=1, fold=True, reps=1, sum_phi=None, ones=None):
    """one step (or `reps` in a row) through the host program.  X N x P 0/1 completed matrix, z 0-based labels (-1: no
    seat), Nk (K,), S (K, P), theta (K, P) for an explicit chain.  Returns a dict: "sites", "cnt" {kj: (M, O, s, n, a,
    b, phi)}, "u", "phi_cell", "bits" (reps, n_cells), "S" (K, P), "X" (N, P), "sum", "ones"."""
    X = np.asarray(X)
    N, P = X.shape
    K = len(Nk)
    nc = len(rows)
    sum_phi = np.zeros(nc) if sum_phi is None else sum_phi
    ones = np.zeros(nc, dtype=np.int64) if ones is None else ones
    ints = lambda a: " ".join(str(int(v)) for v in np.asarray(a).reshape(-1))
    lines = ["%d %d %d %d %d %d %d" % (N, P, K, theta is not None, mode, fold, reps), _hex([beta, gamma]),
             "%d %d %d" % (seed, sweep, nc), ints(z), ints(pack(X)), ints(Nk), ints(S)]
    if theta is not None:
        lines.append(_hex(np.asarray(theta, dtype=np.float64).T))  # k + j * K
    lines += [ints(rows), ints(cols), _hex(sum_phi), ints(ones)]
    path = os.path.join(_DIR.name, "step_%d.txt" % os.getpid())
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([program(), path], capture_output=True, text=True, check=True)
    out = {"sites": [], "cnt": {}, "u": np.full(nc, np.nan), "phi_cell": np.full(nc, np.nan), "bits": []}
    for ln in r.stdout.splitlines():
        t = ln.split()
        if t[0] == "site":
            out["sites"].append(tuple(int(v) for v in t[1:]))
        elif t[0] == "cnt":
            a, b, ph = _f64(t[6:9])
            out["cnt"][int(t[1])] = (int(t[2]), int(t[3]), int(t[4]), int(t[5]), a, b, ph)
        elif t[0] == "cell":
            out["u"][int(t[1])], out["phi_cell"][int(t[1])] = _f64(t[2:4])
        elif t[0] == "bits":
            out["bits"].append([int(v) for v in t[1:]])
        elif t[0] == "S":
            out["S"] = np.array([int(v) for v in t[1:]], dtype=np.int64).reshape(K, P)
        elif t[0] == "X":
            out["X"] = unpack(np.array([int(v) for v in t[1:]], dtype=np.uint32), N, P)
        elif t[0] == "sum":
            out["sum"] = _f64(t[1:])
        elif t[0] == "ones":
            out["ones"] = np.array([int(v) for v in t[1:]], dtype=np.int64)
    out["bits"] = np.array(out["bits"], dtype=np.uint8).reshape(reps, nc)
    return out


# ---------------------------------------------------------------- what is sampled: exact targets and reference chains
def block_loglik_observed(X, obs, rows_of_block, beta, gamma):
    """log marginal likelihood of the observed cells of a block of rows: per feature, the rows that have it observed"""
    Xb, ob = X[rows_of_block], obs[rows_of_block]
    n = ob.sum(axis=0)
    s = (Xb * ob).sum(axis=0)
    return float(np.sum(betaln(beta + s, gamma + n - s) - betaln(beta, gamma)))


def exact_dp_posterior(X, obs, alpha, beta, gamma):
    """CRP(alpha) x observed-cell marginal likelihood over every partition (split_merge_ref.partitions order)"""
    parts = smr.partitions(len(X))
    logw = []
    for z in parts:
        z = np.asarray(z)
        lw = 0.0
        for k in range(z.max() + 1):
            r = np.flatnonzero(z == k)
            lw += np.log(alpha) + gammaln(len(r)) + block_loglik_observed(X, obs, r, beta, gamma)
        logw.append(lw)
    w = np.exp(np.asarray(logw) - np.max(logw))
    return parts, w / w.sum()


def canonical(z):
    seen, out = {}, []
    for v in z:
        out.append(seen.setdefault(int(v), len(seen)))
    return tuple(out)


def impute_counting(X, obs, z, beta, gamma, rng, plug_in=False):
    """the counting chains' step with NumPy draws: phi_kj from the observed-only counts, then the cells given phi
    (plug_in: the cells from the posterior-mean rate instead -- NOT exact, kept to show that a test tells the two
    apart).  Returns phi per missing cell, in (row, column) order."""
    mis = ~obs
    phis = []
    cache = {}
    for i, j in zip(*np.nonzero(mis)):
        k = int(z[i])
        if (k, j) not in cache:
            r = (z == k) & obs[:, j]
            n, s = int(r.sum()), int(X[r, j].sum())
            cache[(k, j)] = (beta + s) / (beta + gamma + n) if plug_in else rng.beta(beta + s, gamma + n - s)
        phis.append(cache[(k, j)])
    for (i, j), ph in zip(zip(*np.nonzero(mis)), phis):
        X[i, j] = int(rng.random() < ph)
    return np.array(phis)


def dp_chain(X0, obs, alpha, beta, gamma, sweeps, seed):
    """the DP sampler's literal conditional, one row at a time on the completed matrix, and the imputation step behind
    every sweep; returns the canonical partition after every sweep"""
    rng = np.random.default_rng(seed)
    X = np.array(X0)
    N, P = X.shape
    X[~obs] = rng.random(int((~obs).sum())) < beta / (beta + gamma)
    z = np.zeros(N, dtype=np.int64)
    visited = []
    for _ in range(sweeps):
        for i in range(N):
            z[i] = -1
            labels = sorted(set(z[z >= 0].tolist()))
            w = []
            for k in labels:
                r = z == k
                n, s = int(r.sum()), X[r].sum(axis=0)
                w.append(n * np.prod(np.where(X[i] == 1, beta + s, gamma + n - s) / (beta + gamma + n)))
            w.append(alpha * np.prod(np.where(X[i] == 1, beta, gamma) / (beta + gamma)))
            w = np.array(w)
            c = int(np.searchsorted(np.cumsum(w), rng.random() * w.sum(), side="right"))
            c = min(c, len(w) - 1)
            z[i] = labels[c] if c < len(labels) else (max(labels) + 1 if labels else 0)
        impute_counting(X, obs, z, beta, gamma, rng)
        visited.append(canonical(z))
    return visited


def finite_chain(X0, obs, K, alpha, beta, gamma, sweeps, burn, seed):
    """a finite collapsed chain with batch 1 (an emptied label keeps its prior weight alpha / K here: the statistical
    reference of the planted-data case, not a replay) and the imputation step; returns the mean over the kept sweeps of
    phi per missing cell"""
    rng = np.random.default_rng(seed)
    X = np.array(X0)
    N, P = X.shape
    X[~obs] = rng.random(int((~obs).sum())) < beta / (beta + gamma)
    z = rng.integers(0, K, N)
    Nk = np.bincount(z, minlength=K).astype(np.float64)
    S = np.stack([X[z == k].sum(axis=0) for k in range(K)]).astype(np.float64)
    acc, kept = 0.0, 0
    for t in range(sweeps):
        u = rng.random(N)
        for i in range(N):
            k0 = z[i]
            Nk[k0] -= 1; S[k0] -= X[i]
            lw = np.log(Nk + alpha / K) + (np.log(np.where(X[i] == 1, beta + S, gamma + Nk[:, None] - S)).sum(axis=1)
                                           - P * np.log(beta + gamma + Nk))
            w = np.exp(lw - lw.max())
            k1 = min(int(np.searchsorted(np.cumsum(w), u[i] * w.sum(), side="right")), K - 1)
            z[i] = k1
            Nk[k1] += 1; S[k1] += X[i]
        phis = impute_counting(X, obs, z, beta, gamma, rng)
        S = np.stack([X[z == k].sum(axis=0) for k in range(K)]).astype(np.float64)
        if t >= burn:
            acc, kept = acc + phis, kept + 1
    return acc / kept


def brier(p, truth):
    return float(np.mean((np.asarray(p, dtype=np.float64) - np.asarray(truth, dtype=np.float64)) ** 2))
