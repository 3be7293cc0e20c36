#!/usr/bin/env python3
"""Cost of the posterior predictive per kept sweep at the north-star shape (ns) and C2, on a
resident chain: sweeps with no new rows, with M = N/10 and with M = N new rows, log-density trace off and on.
Host clock around whole synchronised calls after a warm-up; a per-sweep figure is the difference of two calls that
differ only in the number of sweeps.  Two yardsticks that are not the code under test:
  (a) the resample kernel's own time per observation at the same shape (Chain.profile, HIP events on the launches);
  (b) the host route the feature replaces: Chain.counts() / alpha() after every sweep and the NumPy restatement
      (tests/predictive_ref.py) over the same new rows.
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
import predictive_ref as pref  # noqa: E402
from bmm_mcmc_amd import synth  # noqa: E402


def per_sweep(step, n1, n2, reps=3):
    """milliseconds per sweep: best of `reps` of (time of n2 sweeps - time of n1 sweeps) / (n2 - n1)"""
    best = None
    for _ in range(reps):
        t = []
        for n in (n1, n2):
            t0 = time.perf_counter()
            step(n)
            t.append((time.perf_counter() - t0) * 1e3)
        ms = (t[1] - t[0]) / (n2 - n1)
        best = ms if best is None else min(best, ms)
    return best


def shape(wl, n1, n2, host_sweeps):
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[wl]
    X = synth.host_matrix(N, P, K_true, dseed)[0]
    Xnew = synth.host_matrix(N, P, K_true, dseed + 100)[0]
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

        plain(n1)
        out["ms_sweep_M0"] = round(per_sweep(plain, n1, n2), 4)
        c.profile(1)
        plain(n1)
        ms, launches = c.profile_read()
        c.profile(0)
        out["resample_ns_per_observation"] = round(ms * 1e6 / (n1 * N), 4)
        for tag, M in (("N10", N // 10), ("N", N)):
            c.set_newdata(Xnew[:M])

            def folded(n):
                c.sweeps_predict(n)
                c.sync()

            def traced(n):
                c.sweeps_predict(n, trace=True)

            folded(n1)
            ms_f = per_sweep(folded, n1, n2)
            out["ms_sweep_M" + tag] = round(ms_f, 4)
            out["predict_ns_per_row_M" + tag] = round((ms_f - out["ms_sweep_M0"]) * 1e6 / M, 4)
            out["ms_sweep_M" + tag + "_trace"] = round(per_sweep(traced, n1, n2, reps=2), 4)
            plain(n1)
            out["ms_sweep_M" + tag + "_set_not_folded"] = round(per_sweep(plain, n1, n2), 4)
        # (b) the host route over M = N/10 rows: state over PCIe after every sweep, NumPy on the host
        M = N // 10
        Xh = Xnew[:M]
        t0 = time.perf_counter()
        for _ in range(host_sweeps):
            c.sweeps(1)
            Nk, S = c.counts()
            pref.logdens(pref.collapsed_terms(Xh, Nk, S, c.alpha(), N, 0.5, 0.5))
        out["ms_sweep_host_route_MN10"] = round((time.perf_counter() - t0) * 1e3 / host_sweeps, 3)
    return out


def main():
    out = [shape("ns", 10, 60, 3), shape("c2", 50, 550, 5)]
    print(json.dumps({"predict_probe": out}))


if __name__ == "__main__":
    main()
