"""Cost of the clustering summary: host clock around whole, synchronised calls -- each shape
is run without and with partition=, warm, and the summary is the difference (its share of phase [3] of
bmm_last_run_phases is printed beside it); the host route it replaces, NumPy bincount per pair of rows, is timed on a
stated number of pairs in one thread and scaled to all pairs over 16 threads (labelled "scaled").  Prints one JSON
line.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/partition_probe.py --only ns`.

    python tools/partition_probe.py [--only ns|ns10|c2|c3|psm] [--host-pairs 12]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bmm_mcmc_amd as bm  # noqa: E402
from bmm_mcmc_amd import _capi, synth  # noqa: E402


def phases():
    ms = (C.c_double * 6)()
    _capi.lib().bmm_last_run_phases(ms)
    return [round(float(v), 3) for v in ms]


def timed(fn, **kw):
    t = time.perf_counter()
    out = fn(**kw)
    return (time.perf_counter() - t) * 1e3, out, phases()


def host_route(z, Kc, pairs):
    """NumPy bincount per pair of rows on `pairs` pairs, one thread: seconds per pair"""
    S = z.shape[0]
    rng = np.random.default_rng(0)
    zz = np.ascontiguousarray(z.astype(np.int64) - 1)
    t = time.perf_counter()
    for _ in range(pairs):
        a, b = rng.integers(0, S, 2)
        n = np.bincount(zz[a] * Kc + zz[b], minlength=Kc * Kc)
        int((n.astype(np.int64) ** 2).sum())
    return (time.perf_counter() - t) / pairs


def shape(name, workload, S, stride, host_pairs, similarity=None, crit="binder"):
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[workload]
    X = synth.host_matrix(N, P, K_true, dseed)[0]
    burn = 20
    if sampler == "dp":
        run = lambda **kw: bm.gibbs_dp(X, S + burn, burnin=burn, seed=3, maxK=K, **kw)
    else:
        run = lambda **kw: bm.gibbs_collapsed(X, S + burn, K, burnin=burn, seed=3, **kw)
    timed(run)                                             # warm: code objects, pools
    plain_ms, out, ph0 = timed(run)
    kw = dict(partition=crit, partition_stride=stride)
    timed(run, **kw)
    with_ms, outp, ph1 = timed(run, **kw)
    assert np.array_equal(out["z"], outp["z"])
    Cn = -(-S // stride)
    pairs = S * (S - 1) // 2 if stride == 1 else Cn * S
    summary_ms = with_ms - plain_ms
    rec = {"shape": name, "sampler": sampler, "K": K, "N": N, "S": S, "stride": stride, "criterion": crit,
           "run_ms": round(plain_ms, 2), "run_with_summary_ms": round(with_ms, 2), "summary_ms": round(summary_ms, 2),
           "phases_plain_ms": ph0, "phases_with_ms": ph1, "pairs": pairs,
           "label_pairs_per_s": pairs * N / (summary_ms * 1e-3) if summary_ms > 0 else None,
           "sweeps_ms_phases_2_3": round(ph0[2] + ph0[3], 2), "trace_out_ms_phase_4": ph0[4],
           "plan": bm.partition_plan(S, N, K, Cn, crit), "best": outp["partition"]["best"]}
    if host_pairs:
        per = host_route(out["z"], K, host_pairs)
        rec["host_s_per_pair_one_thread"] = per
        rec["host_pairs_timed"] = host_pairs
        rec["host_ms_scaled_16_threads"] = round(per * pairs / 16 * 1e3, 1)
    if similarity:
        idx = np.random.default_rng(1).integers(0, N, similarity)
        timed(run, similarity_of=idx, **kw)
        sim_ms, _, _ = timed(run, similarity_of=idx, **kw)
        rec["similarity_M"] = similarity
        rec["similarity_ms"] = round(sim_ms - with_ms, 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--host-pairs", type=int, default=12)
    a = ap.parse_args()
    jobs = {"ns": lambda: shape("ns_S200_stride1", "ns", 200, 1, a.host_pairs),
            "ns10": lambda: shape("ns_S200_stride10", "ns", 200, 10, 0),
            "nsvi": lambda: shape("ns_S200_stride1_vi", "ns", 200, 1, 0, crit="vi"),
            "c2": lambda: shape("c2_S1000", "c2", 1000, 1, a.host_pairs),
            "c3": lambda: shape("c3_dp_S200", "c3", 200, 1, a.host_pairs),
            "psm": lambda: shape("ns_S200_stride10_psm8192", "ns", 200, 10, 0, similarity=8192)}
    res = [jobs[k]() for k in jobs if a.only in (None, k)]
    print(json.dumps({"partition_probe": res}))


if __name__ == "__main__":
    main()
