"""Cost of relabel="ecr" (DESIGN.md section 19): host clock around whole, synchronised calls -- each shape is run
without relabelling, with relabel="ecr" for both pivot kinds (the partition pivot against the same run with
partition= alone, so that the summary is not counted as relabelling), and with stephens="device" (burnin 12,
burnrelabel 10, the figures of section 11's table), all warm and from one session; a cost is the difference of two
calls.  Phases [3] and [4] of bmm_last_run_phases are printed beside them: the post-pass and the second label trace
out fall there.  Writes profiles/ecr_probe.json and prints it as one JSON line.

    python tools/ecr_probe.py [--only ns|c2]
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


def timed(fn, **kw):
    best = None
    for _ in range(5):
        t = time.perf_counter()
        out = fn(**kw)
        ms = (time.perf_counter() - t) * 1e3
        if best is None or ms < best[0]:
            best = (ms, out, phases())
    return best


def shape(name, workload, S):
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[workload]
    X = synth.host_matrix(N, P, K_true, dseed)[0]
    run = lambda **kw: bm.gibbs_collapsed(X, S + BURNIN, K, burnin=BURNIN, seed=3, **kw)
    run()                                                  # warm: code objects, pools
    plain_ms, out, ph_plain = timed(run)
    it_ms, oi, ph_it = timed(run, relabel="ecr")
    part_ms, _, ph_part = timed(run, partition="binder", partition_stride=10)
    pp_ms, op, ph_pp = timed(run, partition="binder", partition_stride=10, relabel="ecr", ecr_pivot="partition")
    st_ms, _, ph_st = timed(run, relabel=True, burnrelabel=10, stephens="device")
    assert np.array_equal(out["z"], oi["z_original"]) and np.array_equal(out["z"], op["z_original"])
    sweeps_ms = ph_plain[2] + ph_plain[3]
    return {"shape": name, "sampler": sampler, "K": K, "N": N, "S": S, "burnin": BURNIN,
            "run_ms": round(plain_ms, 2), "sweeps_ms_phases_2_3": round(sweeps_ms, 2),
            "kept_sweeps_ms": round(sweeps_ms * S / (S + BURNIN - 1), 2), "trace_out_ms_phase_4": ph_plain[4],
            "ecr_iterative_ms": round(it_ms - plain_ms, 2), "ecr_iterations": oi["ecr"]["iterations"],
            "ecr_converged": oi["ecr"]["converged"], "phases_ecr_iterative_ms": ph_it,
            "ecr_partition_pivot_ms": round(pp_ms - part_ms, 2), "partition_summary_ms": round(part_ms - plain_ms, 2),
            "phases_ecr_partition_ms": ph_pp, "phases_partition_ms": ph_part,
            "stephens_device_ms": round(st_ms - plain_ms, 2), "phases_stephens_ms": ph_st, "phases_plain_ms": ph_plain,
            "label_bytes_read_per_pass": 4 * S * N, "plan": bm.ecr_plan(S, N, K)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    jobs = {"ns": lambda: shape("ns_S200", "ns", 200), "c2": lambda: shape("c2_S1000", "c2", 1000)}
    res = {"ecr_probe": [jobs[k]() for k in jobs if a.only in (None, k)]}
    line = json.dumps(res)
    if a.only is None:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "ecr_probe.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
