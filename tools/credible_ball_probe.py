"""Cost of the credible ball and the row-to-cluster similarity: host clock around whole,
synchronised runs -- each shape is run warm with partition= and partition_search=, then inside run_options(credible_ball=)
(distances and bounds alone; with the similarity of 4096 rows; with the similarity of all rows), and the ball is the
difference.  The centre is the searched partition, device to device; what crosses PCIe for it is 24 S bytes, three rows
and, with the similarity, 8 M Ka bytes.  Per shape and criterion: the three differences in ms, the radius, the draws
inside and the bounds' cluster counts, and the plan.  Writes profiles/credible_ball_probe.json and prints it.  Kernel
times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/credible_ball_probe.py --only ns`.

    python tools/credible_ball_probe.py [--only ns|c2|c3] [--out FILE]
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

SHAPES = {"ns": ("ns", 200), "c2": ("c2", 1000), "c3": ("c3", 200)}
SUBSET = 4096


def timed(fn, **kw):
    t = time.perf_counter()
    out = fn(**kw)
    return (time.perf_counter() - t) * 1e3, out


def best_of(fn, n=3, **kw):
    """(the smallest of n warm timings, every timing, the last result)"""
    timed(fn, **kw)
    runs = [timed(fn, **kw) for _ in range(n)]
    return min(r[0] for r in runs), [round(r[0], 2) for r in runs], runs[-1][1]


def shape(name):
    workload, S = SHAPES[name]
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[workload]
    X = synth.host_matrix(N, P, K_true, dseed)[0]
    burn = 20
    if sampler == "dp":
        run = lambda **kw: bm.gibbs_dp(X, S + burn, burnin=burn, seed=3, maxK=K, **kw)
    else:
        run = lambda **kw: bm.gibbs_collapsed(X, S + burn, K, burnin=burn, seed=3, **kw)
    rec = {"shape": name, "sampler": sampler, "K": K, "N": N, "S": S, "criteria": {}}
    rows = np.random.default_rng(1).choice(N, SUBSET, replace=False)
    for crit in ("binder", "vi"):
        base_ms, base_all, base = best_of(run, partition=crit, partition_search=True)
        c = {"run_with_search_ms": base_all, "plan": bm.credible_ball_plan(S, N, K, criterion=crit)}
        for key, opt in (("ball", True), ("ball_subset", {"membership_of": rows}), ("ball_all_rows", {"membership": True})):
            with bm.run_options(credible_ball=opt):
                ms, every, out = best_of(run, partition=crit, partition_search=True)
            assert np.array_equal(out["z"], base["z"]) and np.array_equal(out["partition"]["search"]["z"], base["partition"]["search"]["z"])
            c[key + "_ms"] = round(ms - base_ms, 2)
            c[key + "_runs_ms"] = every
        b = out["partition"]["credible_ball"]
        own = b["membership"][np.arange(N), base["partition"]["search"]["z"] - 1]
        c.update(radius=b["radius"], n_in=b["n_in"], n_used=b["n_used"],
                 bounds={q: {"sweep": b[q]["sweep"], "ties": b[q]["ties"], "n_clusters": b[q]["n_clusters"],
                             "distance": b[q]["distance"]} for q in ("horizontal", "upper", "lower")},
                 centre_clusters=base["partition"]["search"]["n_clusters"], mean_own_membership=float(np.nanmean(own)),
                 sim_bytes=int(b["sim"].nbytes))
        rec["criteria"][crit] = c
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "credible_ball_probe.json"))
    a = ap.parse_args()
    res = [shape(k) for k in SHAPES if a.only in (None, k)]
    doc = {"credible_ball_probe": res}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
