"""Shared by the CPU and GPU tests of the allocation sampler: the host build of the spec's draws and log q, the
seven-observation data set's exact posterior over (K, partition) and the comparison of a chain's K with it."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(HERE, "..", "bmm-mcmc_amd", "csrc")
SRC = os.path.join(HERE, "alloc", "alloc_host.cpp")


def build_host(tmp_dir, sanitize=False):
    exe = os.path.join(str(tmp_dir), "alloc_host_san" if sanitize else "alloc_host")
    if not os.path.exists(exe):
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I", INC, SRC, "-o", exe], check=True)
    return exe


def _run(exe, mode, lines, tmp_dir):
    fin, fout = os.path.join(str(tmp_dir), mode + "_in.txt"), os.path.join(str(tmp_dir), mode + "_out.txt")
    with open(fin, "w") as f:
        f.write("".join(line + "\n" for line in lines))
    subprocess.run([exe, mode, fin, fout], check=True)
    with open(fout) as f:
        return [ln.split() for ln in f.read().splitlines()]


def host_draws(exe, tmp_dir, seed, sweep, move, K, maxK, e):
    """ea_move_draws on the host: kind (0 eject, 1 absorb), j1, j2 (0-based), u, p_E (NaN for an absorb), salt"""
    (kind, j1, j2, ub, pb, salt), = _run(exe, "draws", ["%d %d %d %d %d %r" % (seed, sweep, move, K, maxK, float(e))], tmp_dir)
    u = np.array([int(ub)], dtype=np.uint64).view(np.float64)[0]
    return {"kind": int(kind), "j1": int(j1), "j2": int(j2), "u": float(u), "pe_bits": int(pb),
            "pe": float(np.array([int(pb)], dtype=np.uint64).view(np.float64)[0]), "salt": int(salt)}


def host_logq(exe, tmp_dir, triples):
    """lgamma_(e + n1), lbeta_(e + n1, e + n2), ea_log_q(e, n1, n2) on the host for (e, n1, n2) triples"""
    rows = _run(exe, "logq", ["%r %d %d" % (float(e), n1, n2) for e, n1, n2 in triples], tmp_dir)
    return np.array([[int(v) for v in r] for r in rows], dtype=np.uint64).view(np.float64)


def check_k_posterior(Ks, exact, n_batches=100):
    """the visited K against p(K | x), each within 4 standard errors by the batch-means rule of
    split_merge_checks.check_against_enumeration.  Returns the worst ratio."""
    Ks = np.asarray(Ks)
    n = len(Ks) // n_batches * n_batches
    Ks = Ks[:n]
    worst = 0.0
    for K, p in sorted(exact.items()):
        series = (Ks == K).astype(float)
        bm = series.reshape(n_batches, -1).mean(axis=1)
        se = max(bm.std(ddof=1) / np.sqrt(n_batches), np.sqrt(max(p * (1.0 - p), 0.0) / n))
        dev = abs(series.mean() - p)
        print("K=%d exact %.5f chain %.5f  dev/se %.2f" % (K, p, series.mean(), dev / se if se > 0 else 0.0))
        assert dev <= 4.0 * se, (K, p, series.mean(), se)
        if se > 0:
            worst = max(worst, dev / se)
    return worst
