#!/usr/bin/env python3
"""Cost of the pairwise local-dependence check at the north-star shape (ns) and C5, on a resident
chain: sweeps with nothing armed (three runs: their spread is the yardstick), armed but not folding, folding at stride 1
and at stride 10, all P features chosen (ns: 50, 1225 pairs; C5: 100, 4950 pairs).  Host clock around whole synchronised
calls after a warm-up; a per-sweep figure is the difference of two calls that differ only in the number of sweeps (best
of three).  --unarmed-only measures nothing but the unarmed sweeps and calls nothing this feature added, so that it runs
against a build of the parent commit (BMM_LIB_PATH) for the comparison in alternating visits.  --kernels N: only N
folded sweeps after arming, for a kernel-trace run of the profiler around this script (the kernels' own times come from
its statistics, not from here).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (its HIP runtime first, as bench.py)

torch.cuda.init()
import bmm_mcmc_amd as bm  # noqa: E402
from bmm_mcmc_amd import synth  # noqa: E402

SWEEPS = {"ns": (10, 60), "c5": (10, 40)}


def per_sweep(step, n1, n2, reps=3):
    """milliseconds per sweep, one value per repetition: (time of n2 sweeps - time of n1 sweeps) / (n2 - n1)"""
    vals = []
    for _ in range(reps):
        t = []
        for n in (n1, n2):
            t0 = time.perf_counter()
            step(n)
            t.append((time.perf_counter() - t0) * 1e3)
        vals.append((t[1] - t[0]) / (n2 - n1))
    return vals


def shape(wl, unarmed_only, kernels):
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[wl]
    n1, n2 = SWEEPS[wl]
    X, _ = synth.device_matrix(N, P, K_true, dseed, torch.device("cuda", 0))
    z0 = np.random.default_rng(1).integers(1, K + 1, N).astype(np.int32)
    out = {"shape": wl, "N": N, "K": K, "P": P}
    with bm.Chain(sampler, N, P, K, alpha=1.0, seed=3) as c:
        c.set_data_device(X.data_ptr(), keepalive=X)
        c.set_initial_labels(z0)
        c.sweeps(30 if N < 5_000_000 else 10)  # past the first sweeps, where every observation moves
        c.sync()

        def plain(n):
            c.sweeps(n)
            c.sync()

        def folded(n):
            c.sweeps_pair_check(n)
            c.sync()

        if kernels:
            c.set_pair_check(True)
            folded(kernels)
            out["folded_sweeps"] = kernels
            return out
        plain(n1)
        v = per_sweep(plain, n1, n2)
        out["ms_sweep_unarmed"] = round(min(v), 4)
        out["ms_sweep_unarmed_runs"] = [round(x, 4) for x in v]
        if unarmed_only:
            return out
        out["plan"] = bm.pair_check_plan(N, K, P)
        t0 = time.perf_counter()
        c.set_pair_check(True)
        out["ms_arm"] = round((time.perf_counter() - t0) * 1e3, 3)
        plain(n1)
        out["ms_sweep_armed_idle"] = round(min(per_sweep(plain, n1, n2)), 4)
        folded(n1)
        out["ms_sweep_folding"] = round(min(per_sweep(folded, n1, n2)), 4)
        out["ms_per_evaluated_state"] = round(out["ms_sweep_folding"] - out["ms_sweep_unarmed"], 4)
        out["state_in_sweeps"] = round(out["ms_per_evaluated_state"] / out["ms_sweep_unarmed"], 3)
        c.set_pair_check(True, stride=10)
        folded(n1)
        out["ms_sweep_folding_stride10"] = round(min(per_sweep(folded, n1, n2)), 4)
        t0 = time.perf_counter()
        for _ in range(5):
            c.pair_check_state()
        out["ms_pair_check_state"] = round((time.perf_counter() - t0) * 1e3 / 5, 4)
        f = c.pair_check()
        out["n_folded"] = f["n_folded"]
        out["max_abs_z_mean"], out["max_x2_mean"] = float(np.nanmax(np.abs(f["z_mean"]))), float(np.max(f["x2_mean"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ns,c5")
    ap.add_argument("--unarmed-only", action="store_true")
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    out = [shape(wl, args.unarmed_only, args.kernels) for wl in args.shapes.split(",")]
    print(json.dumps({"pair_check_probe": out, "tag": args.tag}))


if __name__ == "__main__":
    main()
