"""Cost and mixing of missing=.

Cost: a resident chain at the north-star shape and at C2 with 0, 1, 10 and 30 % of the cells declared missing, host clock
around `sweeps(n)` and a synchronisation, warm, best of five, against the same chain unarmed; the step alone from
`impute_step()` queued n times, on the counting chain (census, rates and draw) and on a full-sampler chain of the same
shape (the draw alone: its rates are its theta), so the difference is what the census and the rates cost.
Mixing: the package's K3 / N1000 / P5 set with 0, 10, 30 and 50 % of the cells hidden, gibbs_collapsed with K = 3, the
integrated autocorrelation time (kept sweeps / ess()) of the largest cluster's size over four seeds.
Writes profiles/missing_probe.json and prints it as one JSON line.

    python tools/na_probe.py [--only cost|mixing]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bmm_mcmc_amd as bm  # noqa: E402
from bmm_mcmc_amd import synth  # noqa: E402

FRACTIONS = (0.0, 0.01, 0.1, 0.3)


def best_ms(fn, reps=5):
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t) * 1e3
        best = ms if best is None or ms < best else best
    return best


def chain_for(sampler, X, K, mis, seed=3):
    N, P = X.shape
    c = bm.Chain(sampler, N, P, K, seed=seed)
    c.set_data(X if mis is None else np.asfortranarray(np.where(mis, 0, X).astype(np.int32)))
    rng = np.random.default_rng(seed)
    if sampler == "collapsed":
        c.set_initial_labels(rng.integers(1, K + 1, N).astype(np.int32))
    elif sampler in ("full", "stickbreaking"):
        c.set_initial_params(np.ones(K) / K, 0.1 + 0.8 * rng.random((K, P)))
    if mis is not None and mis.any():
        c.set_missing(mask=mis)
    return c


def cost(workload, n):
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[workload]
    X = synth.host_matrix(N, P, K_true, dseed)[0]
    rows = []
    for frac in FRACTIONS:
        mis = np.random.default_rng(7).random(X.shape) < frac if frac > 0 else None
        rec = {"fraction": frac, "n_cells": 0 if mis is None else int(mis.sum())}
        with chain_for(sampler, X, K, mis) as c:
            c.sweeps(30); c.sync()  # warm, and past the start

            def sweeps():
                c.sweeps(n); c.sync()
            rec["ms_per_sweep"] = round(best_ms(sweeps) / n, 4)
            if mis is not None:
                def steps():
                    for _ in range(n):
                        c.impute_step()
                    c.sync()
                rec["step_ms_census_rates_draw"] = round(best_ms(steps) / n, 4)
        if mis is not None:
            with chain_for("full", X, K, mis) as c:
                c.sweeps(3); c.sync()

                def steps():
                    for _ in range(n):
                        c.impute_step()
                    c.sync()
                rec["step_ms_draw_alone"] = round(best_ms(steps) / n, 4)
        rows.append(rec)
    base = rows[0]["ms_per_sweep"]
    for r in rows:
        r["over_unarmed"] = round(r["ms_per_sweep"] / base, 3)
    return {"shape": workload, "sampler": sampler, "K": K, "N": N, "P": P, "sweeps_timed": n, "rows": rows}


def mixing():
    path = os.path.join(ROOT, "tests", "golden", "K3_N1000_P5.txt")
    X = np.asfortranarray(np.array([[int(ch) for ch in ln.strip()] for ln in open(path) if ln.strip()], dtype=np.int32))
    S, burnin, rows = 5000, 1000, []
    for frac in (0.0, 0.1, 0.3, 0.5):
        taus = []
        for seed in range(4):
            mis = np.random.default_rng(100 + seed).random(X.shape) < frac
            r = bm.gibbs_collapsed(X, S + burnin, 3, burnin=burnin, seed=seed, missing=mis if frac > 0 else None)
            size = np.stack([(r["z"] == k).sum(axis=1) for k in (1, 2, 3)]).max(axis=0)
            taus.append(S / bm.ess(size))
        rows.append({"fraction": frac, "iat_largest_cluster": [round(float(t), 2) for t in taus],
                     "iat_mean": round(float(np.mean(taus)), 2)})
    return {"data": "K3_N1000_P5", "K": 3, "kept_sweeps": S, "burnin": burnin, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    res = {}
    if a.only in (None, "cost"):
        res["cost"] = [cost("ns", 50), cost("c2", 200)]
    if a.only in (None, "mixing"):
        res["mixing"] = mixing()
    if a.only is None:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "missing_probe.json"), "w") as f:
            f.write(json.dumps({"missing_probe": res}, indent=1) + "\n")
    print(json.dumps({"missing_probe": res}))


if __name__ == "__main__":
    main()
