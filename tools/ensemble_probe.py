"""What an ensemble of exact chains costs and what it removes.

Speed: chain-sweeps per second of bm.gibbs_ensemble at 1, 64, 256 and 1024 chains on the bundled K3_N1000_P5 (K = 3) and on
a synthetic K = 20, P = 50, N = 4096 mixture -- the host clock around two whole calls that differ in their number of
sweeps only, so that what a call costs once (the upload, the allocations, the traces' way back) cancels -- beside
  (a) the exact route there was: gibbs_collapsed(batch=1) through chains=, a few sweeps;
  (b) the default-batch chain, which is an approximation of the sequential scan and so not like for like;
  (c) the oracle's batch = 1 chain on 16 host threads (oracle_time_sweeps).
Bias: the DP's mean number of clusters in use on K2_N1000_P5 over 64 exact chains beside default-batch chains.
Trace: `--only trace` runs a few ensemble sweeps of both shapes and nothing else: the run to put under a kernel trace of
its own.
Writes profiles/ensemble_probe.json (merging the part that ran into what is there) and prints it as one JSON line.

    python tools/ensemble_probe.py [--only speed|bias|trace]
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
from oracle import oracle  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "ensemble_probe.json")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def bundled(name):
    with open(os.path.join(GOLDEN, name + ".txt")) as f:
        return np.asfortranarray(np.array([[int(c) for c in line.strip()] for line in f if line.strip()], dtype=np.int32))


def mixture(N, P, K, seed):
    rng = np.random.default_rng(seed)
    theta = 0.1 + 0.8 * rng.random((K, P))
    lab = rng.integers(0, K, N)
    return np.asfortranarray((rng.random((N, P)) < theta[lab]).astype(np.int32))


def wall(fn, reps=3):
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        s = time.perf_counter() - t
        best = s if best is None or s < best else best
    return best


def per_sweep(run, n1, n2):
    """seconds per sweep from two calls of n1 and n2 sweeps"""
    return (wall(lambda: run(n2)) - wall(lambda: run(n1))) / (n2 - n1)


def speed_shape(name, X, K, n1, n2, old_chains, old_sweeps):
    N, P = X.shape
    rows = []
    for chains in (1, 64, 256, 1024):
        def run(n):
            bm.gibbs_ensemble(X, n + 1, K, chains=chains, burnin=n, seed=7, keep_trace=False)
        run(2)  # warm
        s = per_sweep(run, n1, n2)
        plan = bm.ensemble_plan("collapsed", N, P, K, chains)
        rows.append({"chains": chains, "ms_per_sweep_of_the_ensemble": round(s * 1e3, 4), "chain_sweeps_per_s": round(chains / s, 1),
                     "launches_per_sweep": plan["launches_per_sweep"], "ms_per_launch": round(s * 1e3 / plan["launches_per_sweep"], 4),
                     "us_per_observation_of_a_chain": round(s * 1e6 / N, 4), "workgroups": plan["workgroups"],
                     "chains_per_workgroup": plan["chains_per_workgroup"]})

    def old(n):
        bm.gibbs_collapsed(X, n + 1, K, burnin=n, seed=7, batch=1, chains=old_chains, keep_trace=True)
    old(1)
    s_old = per_sweep(old, 1, 1 + old_sweeps)

    def dflt(n):
        bm.gibbs_collapsed(X, n + 1, K, burnin=n, seed=7)
    dflt(5)
    s_dflt = per_sweep(dflt, 20, 120)
    sw = max(n2, 20)
    t_or = oracle.time_sweeps("collapsed", X, K, sw, 1, 7, 16)
    res = {"data": name, "N": N, "P": P, "K": K, "sweeps_timed": [n1, n2], "ensemble": rows,
           "a_batch1_through_chains": {"chains": old_chains, "sweeps_timed": old_sweeps, "chain_sweeps_per_s": round(old_chains / s_old, 2)},
           "b_default_batch_one_chain_approximate": {"batch": int(bm.default_batch("collapsed", N)), "chain_sweeps_per_s": round(1.0 / s_dflt, 1)},
           "c_oracle_batch1_16_threads": {"sweeps": sw, "chain_sweeps_per_s": round(16 * sw / t_or, 1)}}
    e256 = rows[2]["chain_sweeps_per_s"]
    res["ensemble_256_over_a"] = round(e256 / res["a_batch1_through_chains"]["chain_sweeps_per_s"], 1)
    res["ensemble_256_over_b"] = round(e256 / res["b_default_batch_one_chain_approximate"]["chain_sweeps_per_s"], 2)
    res["ensemble_256_over_c"] = round(e256 / res["c_oracle_batch1_16_threads"]["chain_sweeps_per_s"], 2)
    return res


def speed():
    return [speed_shape("K3_N1000_P5", bundled("K3_N1000_P5"), 3, 20, 80, 4, 4),
            speed_shape("mixture K20 P50 N4096, data seed 11", mixture(4096, 50, 20, 11), 20, 4, 16, 2, 2)]


def bias():
    X = bundled("K2_N1000_P5")
    ns, burn, maxK = 300, 100, 30
    ens = bm.gibbs_ensemble(X, ns, maxK, sampler="dp", chains=64, burnin=burn, seed=100, keep_trace=False)
    exact = [float((o["sizes"] > 0).sum(axis=1).mean()) for o in ens]
    dflt = []
    for c in range(16):
        z = bm.gibbs_dp(X, ns, burnin=burn, maxK=maxK, seed=100 + c)["z"]
        dflt.append(float(np.mean([np.unique(r).size for r in z])))
    return {"data": "K2_N1000_P5", "sampler": "gibbs_dp", "maxK": maxK, "sweeps": ns, "burnin": burn,
            "exact_64_chains_mean_clusters_in_use": round(float(np.mean(exact)), 3), "exact_sd_over_chains": round(float(np.std(exact)), 3),
            "default_batch": int(bm.default_batch("dp", 1000)), "default_batch_16_chains_mean_clusters_in_use": round(float(np.mean(dflt)), 3),
            "default_batch_sd_over_chains": round(float(np.std(dflt)), 3)}


def trace():
    bm.gibbs_ensemble(bundled("K3_N1000_P5"), 21, 3, chains=256, burnin=20, seed=7, keep_trace=False)
    bm.gibbs_ensemble(mixture(4096, 50, 20, 11), 6, 20, chains=256, burnin=5, seed=7, keep_trace=False)
    bm.gibbs_ensemble(bundled("K2_N1000_P5"), 21, 30, sampler="dp", chains=64, burnin=20, seed=7, keep_trace=False)
    return {"launches": "256 chains x 20 sweeps of K3_N1000_P5; 256 chains x 5 sweeps (2 launches each) of K20 P50 N4096; 64 DP chains x 20 sweeps of K2_N1000_P5"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    if a.only == "trace":
        print(json.dumps({"ensemble_probe_trace": trace()}))
        return
    res = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            res = json.load(f).get("ensemble_probe", {})
    if a.only in (None, "speed"):
        res["speed"] = speed()
    if a.only in (None, "bias"):
        res["bias"] = bias()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(json.dumps({"ensemble_probe": res}, indent=1) + "\n")
    print(json.dumps({"ensemble_probe": res}))


if __name__ == "__main__":
    main()
