"""Builds and runs tests/logpost/logpost_host.cpp, the host statement of the log joint (bmm_spec.h log_joint_spec), for
the CPU test that holds it to the SciPy restatement and the GPU tests that hold the device to it bit for bit; and the
rounding bound both use."""
import functools
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logpost_ref as ref  # noqa: E402
import split_merge_checks as smchk  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "logpost", "logpost_host.cpp")
INC = os.path.join(ROOT, "bmm-mcmc_amd", "csrc")
KIND = {"collapsed": 0, "full": 0, "dp": 1, "stickbreaking": 2, "allocation": 3}
_DIR = tempfile.TemporaryDirectory(prefix="logpost_host_")


@functools.lru_cache(maxsize=None)
def program():
    exe = os.path.join(_DIR.name, "logpost_host")
    # -ffp-contract=off: as the library is built (bmm_spec.h fuses only where it says fma_)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", INC, SRC, "-o", exe], check=True)
    return exe


def _hex(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def mask_words(mask, P):
    words = [0] * ((P + 31) // 32)
    for d in range(P):
        if mask[d]:
            words[d >> 5] |= 1 << (d & 31)
    return words


def run(model, Nk, S, N, alpha, beta, gamma, sample_alpha=False, a=1.0, b=1.0, k_open=None, log_prior_k=None, mask=None,
        rho=0.5):
    """the row of one state through the host program: (bits as uint64[4], values as float64[4])"""
    Nk = np.asarray(Nk, dtype=np.int64)
    S = np.asarray(S, dtype=np.int64)
    K, P = S.shape
    ko = K if k_open is None else int(k_open)
    lpk = 0.0 if log_prior_k is None else float(log_prior_k[ko - 1])
    lines = ["%d %d %d %d %d" % (KIND[model], K, ko, P, N),
             " ".join(_hex(v) for v in (beta, gamma, alpha, a, b, lpk, rho)),
             "%d %d" % (1 if sample_alpha else 0, 0 if mask is None else 1),
             " ".join(str(int(v)) for v in Nk), " ".join(str(int(v)) for v in S.ravel())]
    if mask is not None:
        lines.append(" ".join("%x" % w for w in mask_words(mask, P)))
    path = os.path.join(_DIR.name, "state_%d.txt" % os.getpid())
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([program(), path], capture_output=True, text=True, check=True)
    rows = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert len(rows) == 4, r.stdout
    return (np.array([int(h, 16) for h, _ in rows], dtype=np.uint64), np.array([float(v) for _, v in rows]))


def bound(model, Nk, S, N, alpha, beta, gamma, **kw):
    """eps (LGAMMA_ULPS + 2 + depth) sum max(1, |v_i|) over every lgamma_ / log_ value v_i entering the row: each such
    value is within LGAMMA_ULPS ulps of max(1, |v|) (tests/split_merge_checks.py), `depth` is the longest chain of
    additions of the stated order, each within an ulp of a partial sum that the magnitudes bound, 2 for the restatement's
    own float64 rounding"""
    mag, depth = ref.bound_terms(model, Nk, S, N, alpha, beta, gamma, **kw)
    return smchk.EPS * (smchk.LGAMMA_ULPS + 2 + depth) * mag


def check(model, got, Nk, S, N, alpha, beta, gamma, **kw):
    """got (4 values) against the restatement within the bound; returns the largest error / bound ratio"""
    want = ref.rows_from_counts(model, Nk, S, N, alpha, beta, gamma, **kw)
    bnd = bound(model, Nk, S, N, alpha, beta, gamma, **kw)
    err = np.abs(np.asarray(got) - want)
    print("logpost %s K=%d P=%d N=%d: max |diff| %.3e, bound %.3e, ratio %.3e" % (model, len(Nk), np.shape(S)[1], N, err.max(), bnd, err.max() / bnd))
    assert np.all(err <= bnd), (model, got, want, bnd)
    return float(err.max() / bnd)
