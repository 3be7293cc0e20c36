"""Cost and gain of the greedy search for the point estimate: host clock around whole,
synchronised runs -- each shape is run warm with partition= alone and with partition_search= on top, and the search is
the difference; it starts from the visited estimate, device to device, so no trace crosses PCIe for it.  Per shape and
criterion: the search's ms, passes, halvings, ms per pass (search ms over passes: the rebuilds and the totals are in
it), start_loss -> loss, and the same at batch N/4, N/16 and N/64 beside the default N/8.  Writes
profiles/partition_search_probe.json and prints it.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/partition_search_probe.py --only ns --batches default`.

    python tools/partition_search_probe.py [--only ns|c2|c3] [--batches default|all] [--out FILE]
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


def timed(fn, **kw):
    t = time.perf_counter()
    out = fn(**kw)
    return (time.perf_counter() - t) * 1e3, out


def shape(name, all_batches):
    workload, S = SHAPES[name]
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[workload]
    X = synth.host_matrix(N, P, K_true, dseed)[0]
    burn = 20
    if sampler == "dp":
        run = lambda **kw: bm.gibbs_dp(X, S + burn, burnin=burn, seed=3, maxK=K, **kw)
    else:
        run = lambda **kw: bm.gibbs_collapsed(X, S + burn, K, burnin=burn, seed=3, **kw)
    rec = {"shape": name, "sampler": sampler, "K": K, "N": N, "S": S, "criteria": {}}
    timed(run)  # warm: code objects, pools
    plain_ms, _ = timed(run)
    rec["run_ms"] = round(plain_ms, 2)
    for crit in ("binder", "vi"):
        timed(run, partition=crit)
        a_ms, base = timed(run, partition=crit)
        b_ms, base2 = timed(run, partition=crit)
        c = {"run_with_summary_ms": [round(a_ms, 2), round(b_ms, 2)], "summary_ms": round(min(a_ms, b_ms) - plain_ms, 2),
             "plan": bm.partition_search_plan(S, N, K, criterion=crit), "batches": {}}
        with_ms = min(a_ms, b_ms)
        divs = (8, 4, 16, 64) if all_batches else (8,)
        for div in divs:
            B = -(-N // div)
            opt = True if div == 8 else {"batch": B}
            timed(run, partition=crit, partition_search=opt)
            ms, out = timed(run, partition=crit, partition_search=opt)
            assert np.array_equal(out["z"], base["z"])
            s = out["partition"]["search"]
            halvings = len(set(s["batch"])) - 1
            c["batches"]["N/%d" % div] = {
                "batch": B, "search_ms": round(ms - with_ms, 2), "passes": s["passes"], "halvings": halvings,
                "ms_per_pass": round((ms - with_ms) / s["passes"], 3), "start_loss": s["start_loss"], "loss": s["loss"],
                "ratio": s["loss"] / s["start_loss"] if s["start_loss"] else None, "moved": s["moved"],
                "pass_batch": s["batch"], "converged": s["converged"], "n_clusters": s["n_clusters"]}
        rec["criteria"][crit] = c
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--batches", default="all", choices=["default", "all"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partition_search_probe.json"))
    a = ap.parse_args()
    res = [shape(k, a.batches == "all") for k in SHAPES if a.only in (None, k)]
    doc = {"partition_search_probe": res}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
