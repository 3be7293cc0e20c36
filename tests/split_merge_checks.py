"""Shared by the CPU and GPU tests of the split-merge move: the host build of lgamma_, its arguments and recorded
error, the exact posterior of the 7-observation set and the comparison of a chain with it."""
import os
import subprocess

import numpy as np
from scipy.special import betaln, gammaln

import split_merge_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(HERE, "..", "bmm-mcmc_amd", "csrc")
SRC = os.path.join(HERE, "split_merge", "lgamma_host.cpp")

# Largest error of lgamma_ against scipy's gammaln found by test_split_merge_ref.py over lgamma_arguments(), in ulps
# of max(1, |lgamma(x)|) (near the zeros at 1 and 2 the result is small and the error absolute), rounded up; and the
# documented bound of log_ (bmm_spec.h: below 1 ulp).  The GPU test's bounds are built from these.
LGAMMA_ULPS = 10.0  # measured 9.35 (x = prior + small integer: the shift below 8 cancels about three bits)
LOG_ULPS = 1.0
EPS = 2.0 ** -52


def build_lgamma_host(tmp_dir):
    exe = os.path.join(str(tmp_dir), "lgamma_host")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", INC, SRC, "-o", exe], check=True)
    return exe


def lgamma_host(exe, x, tmp_dir):
    fin, fout = os.path.join(str(tmp_dir), "lg_in.bin"), os.path.join(str(tmp_dir), "lg_out.bin")
    np.asarray(x, dtype=np.float64).tofile(fin)
    subprocess.run([exe, fin, fout], check=True)
    return np.fromfile(fout, dtype=np.float64)


def lgamma_arguments():
    """prior + integer, from 0.01 to 1e7 + 1: every integer up to 300, then a geometric ladder, for six priors"""
    ints = np.unique(np.concatenate([np.arange(0, 301), np.round(np.geomspace(300, 1e7, 400)).astype(np.int64), [10 ** 7]]))
    priors = [0.01, 0.1, 0.5, 1.0, 1.3, 2.5]
    return np.concatenate([p + ints.astype(np.float64) for p in priors])


def lgamma_error_ulps(got, x):
    want = gammaln(x)
    return np.abs(got - want) / (EPS * np.maximum(1.0, np.abs(want)))


# ---------------------------------------------------------------- the exact posterior of a small data set
def exact_posterior(X, alpha, beta, gamma):
    """CRP(alpha) prior x Beta-Bernoulli marginal likelihood over every partition, by brute force with scipy"""
    X = np.asarray(X)
    parts = ref.partitions(len(X))
    logw = []
    for z in parts:
        z = np.asarray(z)
        lw = 0.0
        for k in range(z.max() + 1):
            rows = np.flatnonzero(z == k)
            n, s = len(rows), X[rows].sum(axis=0)
            lw += np.log(alpha) + gammaln(n) + float(np.sum(betaln(beta + s, gamma + n - s) - betaln(beta, gamma)))
        logw.append(lw)
    w = np.exp(np.asarray(logw) - np.max(logw))
    return parts, w / w.sum()


def check_against_enumeration(visited, parts, weights, n_batches=100):
    """visited: the canonical partition after every move (or sweep).  The cluster-count distribution, every
    co-clustering probability and the twenty likeliest partitions against the enumeration, each within 4 standard
    errors: the batch-means estimate (n_batches consecutive batches), and never less than the standard error
    sqrt(p (1 - p) / n) an independent sample of the same length would have (a chain's is not smaller; it keeps a
    quantity the chain happened never to visit from being held to a margin of 0).  Returns the worst ratio."""
    N = len(parts[0])
    index = {s: k for k, s in enumerate(parts)}
    ids = np.array([index[s] for s in visited])
    n = len(ids) // n_batches * n_batches
    ids = ids[:n]
    Z = np.array(parts)
    nclus = Z.max(axis=1) + 1
    feats, exact, names = [], [], []
    for k in range(1, N + 1):
        feats.append((nclus == k).astype(float)); exact.append(weights[nclus == k].sum()); names.append("clusters=%d" % k)
    for i in range(N):
        for j in range(i + 1, N):
            f = (Z[:, i] == Z[:, j]).astype(float)
            feats.append(f); exact.append(float(f @ weights)); names.append("co(%d,%d)" % (i, j))
    for s in np.argsort(-weights)[:20]:
        f = np.zeros(len(parts)); f[s] = 1.0
        feats.append(f); exact.append(weights[s]); names.append("partition %s" % (parts[s],))
    worst = 0.0
    for f, p, name in zip(feats, exact, names):
        series = f[ids]
        bm = series.reshape(n_batches, -1).mean(axis=1)
        se = max(bm.std(ddof=1) / np.sqrt(n_batches), np.sqrt(max(p * (1.0 - p), 0.0) / n))
        dev = abs(series.mean() - p)
        print("%-40s exact %.5f chain %.5f  dev/se %.2f" % (name, p, series.mean(), dev / se if se > 0 else 0.0))
        assert dev <= 4.0 * se, (name, p, series.mean(), se)
        if se > 0:
            worst = max(worst, dev / se)
    return worst
