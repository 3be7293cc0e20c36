#!/usr/bin/env python3
"""Cost of the leave-one-out fold per kept sweep at the north-star shape (ns) and C2, on a
resident chain: sweeps with nothing armed, armed but not folding, folding, and folding with the trace on.
Host clock around whole synchronised calls after a warm-up; a per-sweep figure is the difference of two calls that
differ only in the number of sweeps (best of three; the unarmed figure's three values are kept as its spread).
Two yardsticks that are not the code under test:
  (a) the resample kernel's own time per observation in the same run (Chain.profile, HIP events on the launches);
  (b) the host route the feature replaces: Chain.counts() / labels() / alpha() after every sweep and the NumPy
      restatement (tests/loo_ref.py) over the fitted rows.
Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import bmm_mcmc_amd as bm  # noqa: E402
import loo_ref as lref  # noqa: E402
from bmm_mcmc_amd import synth  # noqa: E402


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


def shape(wl, n1, n2, host_sweeps):
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[wl]
    X = synth.host_matrix(N, P, K_true, dseed)[0]
    z0 = np.random.default_rng(1).integers(1, K + 1, N).astype(np.int32)
    out = {"shape": wl, "N": N, "K": K, "P": P}
    with bm.Chain(sampler, N, P, K, alpha=1.0, seed=3) as c:
        c.set_data(X)
        c.set_initial_labels(z0)
        c.sweeps(30)  # past the first sweeps, where every observation moves
        c.sync()

        def plain(n):
            c.sweeps(n)
            c.sync()

        def folded(n):
            c.sweeps_loo(n)
            c.sync()

        def traced(n):
            c.sweeps_loo(n, trace=True)

        plain(n1)
        v = per_sweep(plain, n1, n2)
        out["ms_sweep_unarmed"] = round(min(v), 4)
        out["ms_sweep_unarmed_runs"] = [round(x, 4) for x in v]
        c.set_loo()
        plain(n1)
        out["ms_sweep_armed_idle"] = round(min(per_sweep(plain, n1, n2)), 4)
        folded(n1)
        c.profile(1)
        folded(n1)
        ms, launches = c.profile_read()
        c.profile(0)
        out["resample_ns_per_observation"] = round(ms * 1e6 / (n1 * N), 4)
        ms_f = min(per_sweep(folded, n1, n2))
        out["ms_sweep_folding"] = round(ms_f, 4)
        out["loo_ns_per_row"] = round((ms_f - out["ms_sweep_unarmed"]) * 1e6 / N, 4)
        nt1, nt2 = max(1, n1 // 5), max(2, n2 // 5)  # (the trace is n x N doubles on the device and over PCIe)
        out["ms_sweep_folding_trace"] = round(min(per_sweep(traced, nt1, nt2, reps=2)), 4)
        t0 = time.perf_counter()
        summary = c.loo()
        out["ms_get_loo"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["n_folded"], out["min_ess"] = summary["n_folded"], round(summary["min_ess"], 2)
        # (b) the host route: statistics, labels and concentration over PCIe after every sweep, NumPy on the host
        t0 = time.perf_counter()
        for _ in range(host_sweeps):
            c.sweeps(1)
            Nk, S = c.counts()
            lref.counting_ell(X, c.labels(), Nk, S, c.alpha(), 0.5, 0.5, "collapsed")
        out["ms_sweep_host_route"] = round((time.perf_counter() - t0) * 1e3 / host_sweeps, 3)
    return out


def main():
    out = [shape("ns", 10, 60, 3), shape("c2", 50, 550, 5)]
    print(json.dumps({"loo_probe": out}))


if __name__ == "__main__":
    main()
