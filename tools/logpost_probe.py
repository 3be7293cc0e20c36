#!/usr/bin/env python3
"""Cost of the log joint trace per kept sweep at the north-star shape (ns), C2 and C5, on a
resident chain: sweeps with nothing armed (three runs: their spread is the yardstick), armed but not folding, folding,
folding with the trace on; the stand-alone call per state; and the host route the feature replaces, a NumPy recount of
one state from the labels (per-feature bincount) and the SciPy restatement (tests/logpost_ref.py).
Host clock around whole synchronised calls after a warm-up; a per-sweep figure is the difference of two calls that
differ only in the number of sweeps (best of three).  --unarmed-only measures nothing but the unarmed sweeps and calls
nothing this feature added, so that it runs against a build of the parent commit (BMM_LIB_PATH) for the comparison in
alternating visits.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (its HIP runtime first, as bench.py)

torch.cuda.init()
import bmm_mcmc_amd as bm  # noqa: E402
from bmm_mcmc_amd import synth  # noqa: E402

SWEEPS = {"ns": (10, 60), "c2": (50, 550), "c5": (10, 60)}


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


def host_recount(Xh, z, K):
    """Nk, S of one state on the host: what the trace a run returns would have to go through, per kept sweep"""
    Nk = np.bincount(z, minlength=K)
    S = np.stack([np.bincount(z, weights=Xh[:, d], minlength=K) for d in range(Xh.shape[1])], axis=1)
    return Nk, S.astype(np.int64)


def shape(wl, unarmed_only):
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
            c.sweeps_logpost(n)
            c.sync()

        def traced(n):
            c.sweeps_logpost(n, trace=True)

        plain(n1)
        v = per_sweep(plain, n1, n2)
        out["ms_sweep_unarmed"] = round(min(v), 4)
        out["ms_sweep_unarmed_runs"] = [round(x, 4) for x in v]
        if unarmed_only:
            return out
        c.set_logpost()
        plain(n1)
        out["ms_sweep_armed_idle"] = round(min(per_sweep(plain, n1, n2)), 4)
        folded(n1)
        out["ms_sweep_folding"] = round(min(per_sweep(folded, n1, n2)), 4)
        out["ms_sweep_folding_trace"] = round(min(per_sweep(traced, n1, n2)), 4)
        out["us_fold"] = round((out["ms_sweep_folding"] - out["ms_sweep_unarmed"]) * 1e3, 2)
        out["fold_share_of_sweep"] = round((out["ms_sweep_folding"] - out["ms_sweep_unarmed"]) / out["ms_sweep_unarmed"], 4)
        best = c.best()
        out["best_sweep"], out["best_log_joint"] = best["sweep"], best["log_joint"]
        t0 = time.perf_counter()
        for _ in range(20):
            c.logpost_state()
        out["ms_logpost_state"] = round((time.perf_counter() - t0) * 1e3 / 20, 4)
        z = c.labels()
        state = c.logpost_state()
    # the stand-alone call: X packed once per call, then per state the labels up, the recount and the score
    Xh = X.cpu().numpy().T  # N x P, column-major
    del X
    t = []
    for S in (1, 3):
        t0 = time.perf_counter()
        r = bm.log_joint(Xh, np.tile(z, (S, 1)), sampler, K, 1.0)
        t.append((time.perf_counter() - t0) * 1e3)
    out["ms_standalone_first_state"] = round(t[0], 3)
    out["ms_standalone_per_state"] = round((t[1] - t[0]) / 2, 3)
    out["standalone_bits_equal"] = bool(np.float64(r["log_joint"][0]).tobytes() == np.float64(state["log_joint"]).tobytes())
    # the host route: a NumPy recount of one state, then the restatement
    import logpost_ref as ref
    t0 = time.perf_counter()
    Nk, S = host_recount(Xh, z - 1, K)
    out["ms_host_recount"] = round((time.perf_counter() - t0) * 1e3, 3)
    t0 = time.perf_counter()
    want = ref.rows_from_counts("collapsed", Nk, S, N, 1.0, 0.5, 0.5)
    out["ms_host_restatement"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["host_minus_device"] = float(want[3] - state["log_joint"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ns,c2,c5")
    ap.add_argument("--unarmed-only", action="store_true")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    out = [shape(wl, args.unarmed_only) for wl in args.shapes.split(",")]
    print(json.dumps({"logpost_probe": out, "tag": args.tag}))


if __name__ == "__main__":
    main()
