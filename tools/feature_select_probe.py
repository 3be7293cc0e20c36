#!/usr/bin/env python3
"""What feature selection costs a sweep, at the C5 and north-star shapes:
  sweeps   armed against unarmed sweeps/s of a resident chain: host clock around whole synchronised calls after a
           warm-up, best of three, alternating;
  kernel   microseconds per k_fs_gamma launch from a `rocprofv3 --kernel-trace --stats` run of this script's child mode
           (a fresh process under the profiler; skipped, and said so, where rocprofv3 is not installed).
Usage: python tools/feature_select_probe.py [sweeps]        (default 100)
Writes profiles/feature_select_probe.json and prints it."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def chain_for(name, armed):
    import torch  # its HIP runtime must be the first one in the process (as in bench.py)
    torch.cuda.init()
    import bmm_mcmc_amd as bm
    from bmm_mcmc_amd import synth
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[name]
    X, labels = synth.device_matrix(N, P, K_true, dseed, "cuda")  # built in HBM: nothing crosses PCIe
    c = bm.Chain(sampler, N, P, K, seed=3)
    c.set_data_device(X.data_ptr())  # packed into bit planes and not read again
    c.set_initial_labels((labels % K + 1).to(torch.int32).cpu().numpy())
    del X
    if armed:
        c.set_feature_select(True, 0.5)
    c.sweeps(10)
    c.sync()
    return c


def rate(c, n):
    t0 = time.perf_counter()
    c.sweeps(n)
    c.sync()
    return n / (time.perf_counter() - t0)


def child(name, n):
    c = chain_for(name, True)
    c.sweeps(n)
    c.sync()
    c.close()


def kernel_us(name, n):
    exe = shutil.which("rocprofv3")
    if not exe:
        return {"skipped": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", name, str(n)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"skipped": "rocprofv3 exited with %d" % r.returncode, "stderr": r.stderr[-400:]}
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    kname = row.get("Name", "")
                    for key in ("k_fs_gamma", "k_count_sweep_end", "k_count_tables", "k_resample"):
                        if key in kname:
                            e = out.setdefault(key, {"calls": 0, "total_ns": 0.0})
                            e["calls"] += int(row["Calls"])
                            e["total_ns"] += float(row["TotalDurationNs"])
        for e in out.values():
            e["us_per_launch"] = round(e["total_ns"] / max(e["calls"], 1) / 1e3, 3)
        return out or {"skipped": "no kernel statistics in the profiler's output"}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]))
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    out = {"sweeps": n, "shapes": []}
    for name in ("c5", "ns"):
        plain, armed = chain_for(name, False), chain_for(name, True)
        r = {"plain": [], "armed": []}
        for _ in range(3):
            r["plain"].append(round(rate(plain, n), 1))
            r["armed"].append(round(rate(armed, n), 1))
        row = {"shape": name, "sweeps_per_s_unarmed": r["plain"], "sweeps_per_s_armed": r["armed"],
               "best_unarmed": max(r["plain"]), "best_armed": max(r["armed"]), "form_unarmed": plain.kernel_shape(),
               "form_armed": armed.kernel_shape(), "inclusion_rb_min_max": [float(v) for v in
                                                                           (armed.feature_summary()["inclusion_rb"].min(),
                                                                            armed.feature_summary()["inclusion_rb"].max())]}
        row["us_per_sweep_added"] = round(1e6 / row["best_armed"] - 1e6 / row["best_unarmed"], 2)
        plain.close()
        armed.close()
        row["kernels"] = kernel_us(name, n)
        out["shapes"].append(row)
        print(row, file=sys.stderr)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "feature_select_probe.json"), "w") as f:
        json.dump({"feature_select_probe": out}, f, indent=1)
        f.write("\n")
    print(json.dumps({"feature_select_probe": out}))


if __name__ == "__main__":
    main()
