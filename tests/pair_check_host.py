"""Builds and runs tests/pair_check/pair_check_host.cpp, the host statement of the pairwise local-dependence check
(bmm_spec.h pair_check_spec), for the CPU test that holds it to the NumPy restatement and the GPU tests that hold the
device to it bit for bit."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_check_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pair_check", "pair_check_host.cpp")
INC = os.path.join(ROOT, "bmm-mcmc_amd", "csrc")
_DIR = tempfile.TemporaryDirectory(prefix="pair_check_host_")


@functools.lru_cache(maxsize=None)
def program():
    exe = os.path.join(_DIR.name, "pair_check_host")
    # -ffp-contract=off: as the library is built (bmm_spec.h fuses only where it says fma_)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", INC, SRC, "-o", exe], check=True)
    return exe


def _f64(hexes):
    return np.array([int(h, 16) for h in hexes], dtype=np.uint64).view(np.float64)


def run(c, s, n):
    """one state's counts c (Kc, npairs), margins s (Kc, M), rows n (Kc,) through the host program:
    {"A", "V", "z", "x2" float64 (npairs,), "df" int32}"""
    c, s, n = np.asarray(c), np.asarray(s), np.asarray(n)
    Kc, M = s.shape
    lines = ["%d %d" % (Kc, M), " ".join(str(int(v)) for v in n), " ".join(str(int(v)) for v in s.ravel()),
             " ".join(str(int(v)) for v in c.ravel())]
    path = os.path.join(_DIR.name, "state_%d.txt" % os.getpid())
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([program(), path], capture_output=True, text=True, check=True)
    rows = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert len(rows) == M * (M - 1) // 2, r.stdout[:200]
    cols = list(zip(*rows))
    return {"A": _f64(cols[0]), "V": _f64(cols[1]), "z": _f64(cols[2]), "x2": _f64(cols[3]),
            "df": np.array([int(v) for v in cols[4]], dtype=np.int32)}


def check(got, c, s, n, what=""):
    """got (a dict with any of "A", "V", "z", "x2", "df") against the restatement within ref.bounds; returns the largest
    error / bound ratio"""
    want, bnd = ref.stats_from_counts(c, s, n), ref.bounds(c, s, n)
    worst = 0.0
    for key in ("A", "V", "x2", "z"):
        if key not in got:
            continue
        g, w = np.asarray(got[key]), want[key]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, key)
        ok = ~np.isnan(w)
        err = np.abs(g[ok] - w[ok])
        assert np.all(err <= bnd[key][ok]), (what, key, float(err.max()), g[ok][np.argmax(err)], w[ok][np.argmax(err)])
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bnd[key][ok] > 0, err / bnd[key][ok], 0.0)
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
    if "df" in got:
        assert np.array_equal(np.asarray(got["df"]), want["df"]), (what, "df")
    print("pair check %s Kc=%d M=%d: worst error / bound %.3e" % (what, s.shape[0], s.shape[1], worst))
    return worst
