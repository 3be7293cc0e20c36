#!/usr/bin/env python3
"""relabel=True cost on the device: per kept sweep, plain against stephens="device", at the north-star shape (ns)
and C2, the batch step, and the hook path with bm.DeviceStephens (every kept sweep's N x K matrix over PCIe and
back).  Host clock around whole synchronised calls after a warm-up call; a per-sweep figure is the difference of
two calls that differ only in the number of kept sweeps.  Prints one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bmm_mcmc_amd as bm  # noqa: E402
from bmm_mcmc_amd import synth  # noqa: E402


def timed(fn, reps=2):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def shape(wl, burnin, W, s1, s2, hook_sweeps):
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[wl]
    X = synth.host_matrix(N, P, K_true, dseed)
    X = X[0] if isinstance(X, tuple) else X
    z0 = np.random.default_rng(1).integers(1, K + 1, N).astype(np.int32)

    def run(S, **kw):
        return lambda: bm.gibbs_collapsed(X, burnin + S, K, alpha=1.0, burnin=burnin, seed=3, initial_K=z0, **kw)

    rel = dict(relabel=True, burnrelabel=W, stephens="device")
    run(s1, **rel)()  # warm-up (pools, kernels)
    plain1, plain2 = timed(run(s1)), timed(run(s2))
    rel1, rel2 = timed(run(s1, **rel)), timed(run(s2, **rel))
    ms_plain = (plain2 - plain1) / (s2 - s1)
    ms_relabel = (rel2 - rel1) / (s2 - s1)
    # what the batch step adds: the relabelled call minus the plain one, less the kept sweeps' online steps and
    # the second label trace out (measured as the same difference at s1 kept sweeps minus s1 online steps)
    batch_ms = (rel1 - plain1) - s1 * (ms_relabel - ms_plain)
    hook = dict(relabel=True, burnrelabel=W, stephens=bm.DeviceStephens(0))
    h1 = timed(run(1, **hook), reps=1)
    h2 = timed(run(1 + hook_sweeps, **hook), reps=1)
    return {"shape": wl, "N": N, "K": K, "burnin": burnin, "burnrelabel": W,
            "ms_plain": round(ms_plain, 4), "ms_relabel": round(ms_relabel, 4),
            "ratio": round(ms_relabel / ms_plain, 2), "batch_ms": round(batch_ms, 2),
            "ms_hook_device_stephens": round((h2 - h1) / hook_sweeps, 3)}


def main():
    out = [shape("ns", 12, 10, 20, 120, 5), shape("c2", 12, 10, 50, 550, 20)]
    print(json.dumps({"relabel_probe": out}))


if __name__ == "__main__":
    main()
