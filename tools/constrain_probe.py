"""Cost and stickiness of known= / allowed=.

Cost: a resident chain at the north-star shape and at C2 with 0, 1, 10 and 50 % of the rows known (their generating
component), host clock around `sweeps(n)` and a synchronisation, warm, best of five, against the same chain unarmed in the
same process.  The draws of held rows are still computed: the resample kernels are untouched, so what is measured is
k_constrain behind every launch and the moves it undoes.
Revert rate: planted K = 3, N = 4096, P = 24 data; every row either known (8 per class) or, for a share of the others,
allowed every class but one that is not its own; gibbs_collapsed over 200 kept sweeps.
Anchoring: the same data with the 8 known rows per class alone, eight seeds from a random start: how often label k ends
as generating component k (tests/tolerance_cases.py's owner rule), against the unconstrained chain.
Writes profiles/constrain_probe.json (merging the part that ran into what is there) and prints it as one JSON line.

    python tools/constrain_probe.py [--only cost|revert|anchor]
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

FRACTIONS = (0.0, 0.01, 0.1, 0.5)
OUT = os.path.join(ROOT, "profiles", "constrain_probe.json")


def best_ms(fn, reps=5):
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t) * 1e3
        best = ms if best is None or ms < best else best
    return best


def cost(workload, n):
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[workload]
    X, labels, _, _ = synth.host_matrix(N, P, K_true, dseed)
    rows = []
    for frac in FRACTIONS:
        known = np.where(np.random.default_rng(7).random(N) < frac, labels % K + 1, 0)
        with bm.Chain(sampler, N, P, K, seed=3) as c:
            c.set_data(X)
            c.set_initial_labels(np.random.default_rng(3).integers(1, K + 1, N).astype(np.int32))
            if frac > 0:
                c.set_known(known)
            c.sweeps(30); c.sync()  # warm, and past the start

            def sweeps():
                c.sweeps(n); c.sync()
            rec = {"fraction": frac, "n_rows": int((known > 0).sum()), "ms_per_sweep": round(best_ms(sweeps) / n, 4)}
            if frac > 0:
                st = c.constraint_stats()
                rec["revert_rate"] = round(st["rate"], 5)
        rows.append(rec)
    base = rows[0]["ms_per_sweep"]
    for r in rows:
        r["over_unarmed"] = round(r["ms_per_sweep"] / base, 3)
    return {"shape": workload, "sampler": sampler, "K": K, "N": N, "P": P, "batch": int(bm.default_batch(sampler, N)),
            "sweeps_timed": n, "rows": rows}


def planted():
    N, P, K = 4096, 24, 3
    X, labels, theta, _ = synth.host_matrix(N, P, K, 41)
    known = np.zeros(N, dtype=np.int64)
    for k in range(K):
        known[np.flatnonzero(labels == k)[:8]] = k + 1
    return X, labels, theta, known, K


def revert():
    X, labels, _, known, K = planted()
    N = len(X)
    rows = []
    for share in (0.1, 0.5, 1.0):
        rng = np.random.default_rng(11)
        A = np.ones((N, K), dtype=bool)
        for i in np.flatnonzero((known == 0) & (rng.random(N) < share)):
            A[i, (labels[i] + 1 + rng.integers(K - 1)) % K] = False
        r = bm.gibbs_collapsed(X, 250, K, burnin=50, seed=1, known=known, allowed=A)
        c = r["constraints"]
        rows.append({"share_of_rows_with_a_set": share, "n_rows": c["n_rows"], "n_known": c["n_known"],
                     "proposed": c["proposed"], "reverted": c["reverted"], "rate": round(c["rate"], 5)})
    return {"data": "planted K3 N4096 P24, data seed 41", "kept_sweeps": 200, "rows": rows}


def anchor():
    X, labels, _, known, K = planted()

    def owners(z):
        tab = np.zeros((K, K), dtype=np.int64)
        np.add.at(tab, (z - 1, labels), 1)
        return tab.argmax(axis=1).tolist()
    rows = []
    for seed in range(1, 9):
        a = bm.gibbs_collapsed(X, 100, K, burnin=50, seed=seed, known=known)
        f = bm.gibbs_collapsed(X, 100, K, burnin=50, seed=seed)
        rows.append({"seed": seed, "anchored": owners(a["z"][-1]), "unconstrained": owners(f["z"][-1]),
                     "revert_rate": round(a["constraints"]["rate"], 5)})
    ident = list(range(K))
    return {"data": "planted K3 N4096 P24, data seed 41, 8 known rows per class, random start", "rows": rows,
            "anchored_identity": sum(r["anchored"] == ident for r in rows),
            "unconstrained_identity": sum(r["unconstrained"] == ident for r in rows), "seeds": len(rows)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    res = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            res = json.load(f).get("constrain_probe", {})
    if a.only in (None, "cost"):
        res["cost"] = [cost("ns", 50), cost("c2", 200)]
    if a.only in (None, "revert"):
        res["revert"] = revert()
    if a.only in (None, "anchor"):
        res["anchor"] = anchor()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(json.dumps({"constrain_probe": res}, indent=1) + "\n")
    print(json.dumps({"constrain_probe": res}))


if __name__ == "__main__":
    main()
