#!/usr/bin/env python3
"""Cost of the fold of INCOMPLETE new rows per kept sweep at the north-star shape (ns) and C2,
on a resident chain: M = N/10 and M = N new rows with 1 %, 10 % and 30 % of their cells missing, beside the
complete-row fold (the existing kernels) of the same rows against the same chain in the same
process.  Host clock around whole synchronised calls after a warm-up; a per-sweep figure is the difference of two
calls that differ only in the number of sweeps, the best of three; the cost of a fold is that figure less the sweep's
own (no new rows).  Prints one JSON line (profiles/predict_na_probe.json keeps it)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bmm_mcmc_amd as bm  # noqa: E402
from bmm_mcmc_amd import synth  # noqa: E402

FRACTIONS = (0.01, 0.1, 0.3)


def per_sweep(step, n1, n2, reps=3):
    """milliseconds per sweep: best of `reps` of (time of n2 sweeps - time of n1 sweeps) / (n2 - n1)"""
    best = None
    for _ in range(reps):
        t = []
        for n in (n1, n2):
            t0 = time.perf_counter()
            step(n)
            t.append((time.perf_counter() - t0) * 1e3)
        ms = (t[1] - t[0]) / (n2 - n1)
        best = ms if best is None else min(best, ms)
    return best


def shape(wl, n1, n2):
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[wl]
    X = synth.host_matrix(N, P, K_true, dseed)[0]
    Xnew = synth.host_matrix(N, P, K_true, dseed + 100)[0]
    z0 = np.random.default_rng(1).integers(1, K + 1, N).astype(np.int32)
    out = {"shape": wl, "N": N, "K": K, "P": P, "plan": bm.predict_na_plan(sampler, K, P), "rows": []}
    with bm.Chain(sampler, N, P, K, alpha=1.0, seed=3) as c:
        c.set_data(X)
        c.set_initial_labels(z0)
        c.sweeps(30)  # past the first sweeps, where every observation moves
        c.sync()

        def plain(n):
            c.sweeps(n)
            c.sync()

        def folded(n):
            c.sweeps_predict(n)
            c.sync()

        plain(n1)
        out["ms_sweep_M0"] = round(per_sweep(plain, n1, n2), 4)
        for M in (N // 10, N):
            Xm = np.asfortranarray(Xnew[:M])
            c.set_newdata(Xm)
            folded(n1)
            ms_c = per_sweep(folded, n1, n2) - out["ms_sweep_M0"]
            for frac in FRACTIONS:
                miss = np.random.default_rng(int(frac * 1000) + M % 1000).random((M, P)) < frac
                rows, cols = np.nonzero(miss)
                c.set_newdata_missing(rows, cols)
                folded(n1)
                ms_m = per_sweep(folded, n1, n2) - out["ms_sweep_M0"]
                out["rows"].append({"M": M, "missing": frac, "cells": int(rows.size),
                                    "ms_fold_complete": round(ms_c, 4), "ms_fold_masked": round(ms_m, 4),
                                    "ratio": round(ms_m / ms_c, 3),
                                    "ns_per_row_complete": round(ms_c * 1e6 / M, 3),
                                    "ns_per_row_masked": round(ms_m * 1e6 / M, 3)})
            c.set_newdata_missing([], [])
            folded(n1)
            ms_c2 = per_sweep(folded, n1, n2) - out["ms_sweep_M0"]  # the complete-row fold again, after the masked ones
            out["rows"].append({"M": M, "missing": 0.0, "ms_fold_complete": round(ms_c, 4),
                                "ms_fold_complete_again": round(ms_c2, 4)})
    return out


def counters():
    """What a `rocprofv3 --pmc` run of its own (counters alone, no tracing) is taken over: at the north star, M = N new
    rows, 20 folds with 10 % of the cells missing (k_score_na) and 20 complete-row folds of the same rows (k_score)."""
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS["ns"]
    X = synth.host_matrix(N, P, K_true, dseed)[0]
    Xnew = np.asfortranarray(synth.host_matrix(N, P, K_true, dseed + 100)[0])
    with bm.Chain(sampler, N, P, K, alpha=1.0, seed=3) as c:
        c.set_data(X)
        c.set_initial_labels(np.random.default_rng(1).integers(1, K + 1, N).astype(np.int32))
        c.sweeps(30)
        c.set_newdata(Xnew)
        c.sweeps_predict(20)
        c.set_newdata_missing(*np.nonzero(np.random.default_rng(100).random((N, P)) < 0.1))
        c.sweeps_predict(20)
        c.sync()


def main():
    if "--counters" in sys.argv[1:]:
        return counters()
    out = [shape("ns", 10, 60), shape("c2", 50, 550)]
    print(json.dumps({"predict_na_probe": out}))


if __name__ == "__main__":
    main()
