"""Cost and gain of categorical features.

Cost: a resident categorical chain -- N = 10^6, K = 20, ten 5-level features, P = 50 one-hot columns -- beside the
Bernoulli north star of the same P (bmm_mcmc_amd.synth "ns"), host clock around `sweeps(n)` and a synchronisation, warm,
best of five, in one process; which resample form each ran (kernel_shape, and the plan's word on the packed kernel).
Gain: planted data, N = 4096, three classes, eight 4-level items; the adjusted Rand index of the partition="vi" estimate
against the generating allocation for the categorical chain and for the Bernoulli chain on the same one-hot columns,
gibbs_dp, eight seeds each.
Trace: `--only trace` runs a few sweeps of both chains of the cost part and nothing else: the run to put under a kernel
trace of its own, which then holds the launches of k_count_tables<TAB_CAT> beside those of <TAB_PLAIN>.
Writes profiles/categorical_probe.json (merging the part that ran into what is there) and prints it as one JSON line.

    python tools/categorical_probe.py [--only cost|gain|trace]
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

OUT = os.path.join(ROOT, "profiles", "categorical_probe.json")


def best_ms(fn, reps=5):
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t) * 1e3
        best = ms if best is None or ms < best else best
    return best


def planted(N, levels, classes, seed, conc=0.4):
    """level indices from `classes` components, one Dirichlet(conc) profile per component and feature; the allocation"""
    rng = np.random.default_rng(seed)
    comp = rng.integers(classes, size=N)
    X = np.zeros((N, len(levels)), dtype=np.int64)
    for j, L in enumerate(levels):
        prof = rng.dirichlet(np.full(L, conc), size=classes)
        X[:, j] = (rng.random(N)[:, None] > np.cumsum(prof, axis=1)[comp]).sum(axis=1).clip(0, L - 1)
    return X, comp


def cost_chains():
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS["ns"]
    Xb = synth.host_matrix(N, P, K_true, dseed)[0]
    D = bm.categorical(planted(N, [5] * 10, K_true, dseed)[0])
    assert D.shape == (N, P)
    return sampler, K, N, P, (("bernoulli", Xb, None), ("categorical", np.asarray(D), D.chain_levels))


def cost(n):
    sampler, K, N, P, chains = cost_chains()
    rows = []
    for name, X, levels in chains:
        with bm.Chain(sampler, N, P, K, seed=3) as c:
            c.set_data(X)
            if levels is not None:
                c.set_categorical(levels)
            c.set_initial_labels(np.random.default_rng(3).integers(1, K + 1, N).astype(np.int32))
            c.sweeps(30); c.sync()  # warm, and past the start

            def sweeps():
                c.sweeps(n); c.sync()
            ms = best_ms(sweeps) / n
            rows.append({"chain": name, "ms_per_sweep": round(ms, 4), "sweeps_per_s": round(1e3 / ms, 1), "kernel_shape": c.kernel_shape(),
                         "plan_packed": bm.categorical_plan(sampler, N, K, [1] * P if levels is None else levels)["packed"]})
    return {"sampler": sampler, "K": K, "N": N, "P": P, "batch": int(bm.default_batch(sampler, N)), "sweeps_timed": n, "rows": rows,
            "categorical_over_bernoulli": round(rows[1]["ms_per_sweep"] / rows[0]["ms_per_sweep"], 3)}


def trace(n):
    sampler, K, N, P, chains = cost_chains()
    for name, X, levels in chains:
        with bm.Chain(sampler, N, P, K, seed=3) as c:
            c.set_data(X)
            if levels is not None:
                c.set_categorical(levels)
            c.set_initial_labels(np.random.default_rng(3).integers(1, K + 1, N).astype(np.int32))
            c.sweeps(n); c.sync()
    return {"sweeps_per_chain": n}


def ari(a, b):
    """adjusted Rand index of two allocations"""
    a, b = np.unique(a, return_inverse=True)[1], np.unique(b, return_inverse=True)[1]
    tab = np.zeros((a.max() + 1, b.max() + 1), dtype=np.int64)
    np.add.at(tab, (a, b), 1)
    c2 = lambda v: (v * (v - 1) // 2).sum()  # noqa: E731
    n2 = len(a) * (len(a) - 1) // 2
    exp = c2(tab.sum(axis=1)) * c2(tab.sum(axis=0)) / n2
    mx = 0.5 * (c2(tab.sum(axis=1)) + c2(tab.sum(axis=0)))
    return float((c2(tab) - exp) / (mx - exp))


def gain():
    N, levels, classes = 4096, [4] * 8, 3
    Xc, comp = planted(N, levels, classes, 41, conc=1.0)
    D = bm.categorical(Xc)
    rows = []
    for seed in range(1, 9):
        rec = {"seed": seed}
        for name, data in (("categorical", D), ("bernoulli", np.asarray(D))):
            out = bm.gibbs_dp(data, 300, burnin=100, seed=seed, partition="vi")
            z = out["partition"]["z"]
            rec[name] = {"ari": round(ari(z, comp), 4), "clusters": int(len(np.unique(z)))}
        rows.append(rec)
    mean = {k: round(float(np.mean([r[k]["ari"] for r in rows])), 4) for k in ("categorical", "bernoulli")}
    return {"data": "planted N4096, 3 classes, eight 4-level items, Dirichlet(1) profiles, data seed 41", "sampler": "gibbs_dp",
            "sweeps": 300, "burnin": 100, "rows": rows, "mean_ari": mean}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    if a.only == "trace":
        print(json.dumps({"categorical_probe_trace": trace(20)}))
        return
    res = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            res = json.load(f).get("categorical_probe", {})
    if a.only in (None, "cost"):
        res["cost"] = cost(50)
    if a.only in (None, "gain"):
        res["gain"] = gain()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(json.dumps({"categorical_probe": res}, indent=1) + "\n")
    print(json.dumps({"categorical_probe": res}))


if __name__ == "__main__":
    main()
