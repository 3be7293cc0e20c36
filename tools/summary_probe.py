"""Cost of summary= and what keep_trace=False buys: host clock around whole, synchronised calls,
best of five warm calls, one session -- the method of tools/ecr_probe.py.  At the north star and at C2: a plain run,
summary= at stride 1 and 10 (and without a pivot, and without the label trace), and relabel="ecr" against the same
pivot, the post-pass the online fold replaces.  At C5 (N = 1e7): a plain run of S = 200 against summary= with
keep_trace=False, run_bytes of both, and one keep_trace=False run of S = 2000, whose trace would take 80 GB on either
side.  Writes profiles/summary_probe.json (the shapes that were run) and prints it as one JSON line.

    python tools/summary_probe.py [--only ns|c2|c5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bmm_mcmc_amd as bm  # noqa: E402
from bmm_mcmc_amd import _capi, synth  # noqa: E402

BURNIN = 12


def phases():
    ms = (C.c_double * 6)()
    _capi.lib().bmm_last_run_phases(ms)
    return [round(float(v), 3) for v in ms]


def timed(fn, reps=5, **kw):
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn(**kw)
        ms = (time.perf_counter() - t) * 1e3
        if best is None or ms < best[0]:
            best = (ms, out, phases())
        else:
            del out
    return best


def big_matrix(N, P, K_true, seed, rows=1_000_000):
    """synth.host_matrix's recipe a block of rows at a time (binary32 uniforms): N = 1e7 without a 8 GB temporary"""
    rng = np.random.Generator(np.random.PCG64(seed))
    w, theta = synth.truth(K_true, P, seed)
    labels = rng.permutation(np.repeat(np.arange(K_true), synth.counts(N, w)))
    X = np.empty((N, P), dtype=np.int32, order="F")
    th = theta.astype(np.float32)
    for lo in range(0, N, rows):
        hi = min(N, lo + rows)
        X[lo:hi] = rng.random((hi - lo, P), dtype=np.float32) < th[labels[lo:hi]]
    return X


def shape(name, workload, S):
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[workload]
    X = synth.host_matrix(N, P, K_true, dseed)[0]
    run = lambda **kw: bm.gibbs_collapsed(X, S + BURNIN, K, burnin=BURNIN, seed=3, **kw)
    run(summary=True)                                      # warm: code objects, pools
    plain_ms, out, ph_plain = timed(run)
    s1_ms, o1, ph_s1 = timed(run, summary=True)
    s10_ms, o10, _ = timed(run, summary=True, summary_stride=10)
    none_ms, _, _ = timed(run, summary=True, summary_pivot=None)
    lean_ms, ol, ph_lean = timed(run, summary=True, keep_trace=False)
    pivot = o1["summary"]["pivot"]
    ecr_ms, oe, ph_ecr = timed(run, relabel="ecr", ecr_pivot=pivot)
    assert np.array_equal(out["z"], o1["z"]) and np.array_equal(out["z"], oe["z_original"]) and ol["z"] is None
    assert np.array_equal(o1["summary"]["permutations"], oe["permutations"]) and np.array_equal(o1["summary"]["agree"], oe["ecr"]["agree"])
    assert np.array_equal(o1["summary"]["z_hat"], ol["summary"]["z_hat"]) and o10["summary"]["n_folded"] == len(range(0, S, 10))
    sweeps_ms = ph_plain[2] + ph_plain[3]
    sure = o1["summary"]["n_max"] / float(o1["summary"]["n_folded"])
    return {"shape": name, "sampler": sampler, "K": K, "N": N, "P": P, "S": S, "burnin": BURNIN,
            "run_ms": round(plain_ms, 2), "sweeps_ms_phases_2_3": round(sweeps_ms, 2),
            "plain_sweep_ms": round(sweeps_ms / (S + BURNIN - 1), 4),
            "summary_stride1_ms": round(s1_ms - plain_ms, 2), "summary_stride1_per_folded_sweep_ms": round((s1_ms - plain_ms) / S, 4),
            "summary_stride10_ms": round(s10_ms - plain_ms, 2),
            "summary_stride10_per_folded_sweep_ms": round((s10_ms - plain_ms) / len(range(0, S, 10)), 4),
            "summary_no_pivot_ms": round(none_ms - plain_ms, 2), "summary_no_pivot_per_folded_sweep_ms": round((none_ms - plain_ms) / S, 4),
            "summary_without_trace_ms": round(lean_ms - plain_ms, 2), "ecr_given_pivot_post_pass_ms": round(ecr_ms - plain_ms, 2),
            "ecr_given_pivot_per_row_ms": round((ecr_ms - plain_ms) / S, 4),
            "armed_over_plain_sweep": round(((s1_ms - plain_ms) / S + sweeps_ms / (S + BURNIN - 1)) / (sweeps_ms / (S + BURNIN - 1)), 3),
            "phases_plain_ms": ph_plain, "phases_summary_ms": ph_s1, "phases_without_trace_ms": ph_lean, "phases_ecr_ms": ph_ecr,
            "share_of_rows_sure_above_0.9": round(float((sure > 0.9).mean()), 4),
            "run_bytes_with_trace": bm.run_bytes(sampler, N, P, K, S), "run_bytes_summary_with_trace": bm.run_bytes(sampler, N, P, K, S, True, True),
            "run_bytes_summary_without_trace": bm.run_bytes(sampler, N, P, K, S, False, True), "plan": bm.summary_plan(N, P, K)}


def c5(S=200, S_long=2000):
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS["c5"]
    X = big_matrix(N, P, K_true, dseed)
    run = lambda S_, **kw: bm.gibbs_collapsed(X, S_ + BURNIN, K, burnin=BURNIN, seed=3, **kw)
    run(20, summary=True, keep_trace=False)                # warm
    plain_ms, out, ph_plain = timed(lambda **kw: run(S, **kw))
    last = out["z"][-1].copy()
    del out
    lean_ms, ol, ph_lean = timed(lambda **kw: run(S, **kw), summary=True, keep_trace=False)
    t = time.perf_counter()
    long_ = run(S_long, summary=True, keep_trace=False)
    long_ms = (time.perf_counter() - t) * 1e3
    ph_long = phases()
    su = long_["summary"]
    sure = su["n_max"] / float(su["n_folded"])
    return {"shape": "c5", "sampler": sampler, "K": K, "N": N, "P": P, "S": S, "burnin": BURNIN,
            "run_ms": round(plain_ms, 2), "phases_plain_ms": ph_plain,
            "summary_without_trace_run_ms": round(lean_ms, 2), "phases_without_trace_ms": ph_lean,
            "plain_sweeps_ms_phases_2_3": round(ph_plain[2] + ph_plain[3], 2), "without_trace_sweeps_ms_phases_2_3": round(ph_lean[2] + ph_lean[3], 2),
            "z_hat_agrees_with_last_plain_state": round(float((ol["summary"]["z_hat"] == last).mean()), 4),
            "run_bytes_with_trace": bm.run_bytes(sampler, N, P, K, S), "run_bytes_summary_without_trace": bm.run_bytes(sampler, N, P, K, S, False, True),
            "host_trace_bytes": 4 * S * N,
            "long": {"S": S_long, "run_ms": round(long_ms, 2), "phases_ms": ph_long, "n_folded": su["n_folded"],
                     "sweeps_per_s": round((S_long + BURNIN - 1) / ((ph_long[2] + ph_long[3]) * 1e-3), 1),
                     "run_bytes_summary_without_trace": bm.run_bytes(sampler, N, P, K, S_long, False, True),
                     "run_bytes_with_trace": bm.run_bytes(sampler, N, P, K, S_long), "host_trace_bytes": 4 * S_long * N,
                     "share_of_rows_sure_above_0.9": round(float((sure > 0.9).mean()), 4),
                     "pi_mean": [round(float(v), 5) for v in su["pi_mean"]]},
            "plan": bm.summary_plan(N, P, K)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_probe.json"))
    a = ap.parse_args()
    jobs = {"ns": lambda: shape("ns_S200", "ns", 200), "c2": lambda: shape("c2_S1000", "c2", 1000), "c5": c5}
    res = {"summary_probe": [jobs[k]() for k in jobs if a.only in (None, k)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
