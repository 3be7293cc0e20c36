#!/usr/bin/env python3
"""What the k-modes++ start costs and what it buys, on one MI355X.

  tools/init_probe.py time ns|c5        HIP-event time of one initialisation (iters 0 and 10) beside one sweep of the
                                        same chain in the same process: warm-up, repeats, median and spread
  tools/init_probe.py trap N seeds      from a random start and from init="kmodes", how many of `seeds` chains end in the
                                        generating mode (every generating component held by exactly one cluster), on
                                        synth.host_matrix(N, 50, 20, 22), the data and criterion of
                                        tests/tools/mode_trap_scan.py, default batch, 140 sweeps
Each call prints one JSON line; tools/init_probe.py merge FILE... gathers them into profiles/init_probe.json.
tools/init_probe.sh is the driver: every step under its own time limit, chained so that a failure ends the script."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 20
# "the same number of sweeps" as the recorded scan of tests/tools/mode_trap_scan.py this probe is read beside
with open(os.path.join(ROOT, "profiles", "r03", "mode_trap_scan_N1e5_96seeds.json")) as _f:
    SWEEPS = int(json.load(_f)["sweeps"])


def spread(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1]), "n": int(len(v))}


def time_shape(name):
    import torch
    import bmm_mcmc_amd as bm
    from bmm_mcmc_amd import synth
    sampler, k, k_true, N, P, seed = synth.WORKLOADS[name]
    X, _ = synth.device_matrix(N, P, k_true, seed, "cuda:0")
    torch.cuda.synchronize()
    out = {"shape": name, "N": N, "P": P, "K": k, "warmup": 2, "repeats": 7}
    with bm.Chain("collapsed", N, P, k, seed=1) as ch:
        ch.set_data_device(X.data_ptr(), keepalive=X)
        del X
        for iters in (0, 10):
            ms, rounds = [], []
            for rep in range(2 + 7):  # the initialisation may be repeated until the chain starts
                info = ch.init_labels("kmodes", iters=iters)
                if rep >= 2:
                    ms.append(info["device_ms"])
                    rounds.append(info["rounds_run"])
            out["init_ms_iters%d" % iters] = spread(ms)
            out["rounds_run_iters%d" % iters] = rounds[0]
            out["cost_iters%d" % iters] = info["cost"]
        # one sweep, measured as the initialisation is: HIP events on the chain's own stream around 10 sweeps
        ext = torch.cuda.ExternalStream(ch.stream(), device="cuda:0")
        ch.sweeps(3)
        ch.sync()
        per = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ext)
            ch.sweeps(10)
            e1.record(ext)
            e1.synchronize()
            per.append(e0.elapsed_time(e1) / 10.0)
        out["sweep_ms"] = spread(per)
    return out


def in_mode(z1, labels, N):
    tab = np.zeros((K, K), dtype=np.int64)
    np.add.at(tab, (z1 - 1, labels), 1)
    owner = tab.argmax(axis=1)
    big = tab.sum(axis=1) > N // 1000
    per = [int((big & (owner == c)).sum()) for c in range(K)]
    return all(v == 1 for v in per), float(tab.max(axis=1).sum() / N)


def trap(N, nseeds):
    import bmm_mcmc_amd as bm
    from bmm_mcmc_amd import synth
    P = 50
    X, labels, _, _ = synth.host_matrix(N, P, K, 22)
    out = {"N": N, "K": K, "P": P, "sweeps": SWEEPS, "seeds": nseeds, "batch": int(bm.default_batch("collapsed", N))}
    for init in ("random", "kmodes"):
        whole, agree, rounds = [], [], []
        for s in range(nseeds):
            seed = 2000 + s
            with bm.Chain("collapsed", N, P, K, seed=seed) as ch:
                ch.set_data(X)
                if init == "random":
                    ch.set_initial_labels(np.random.default_rng(seed).integers(1, K + 1, N).astype(np.int32))
                else:
                    rounds.append(ch.init_labels("kmodes")["rounds_run"])
                ch.sweeps(SWEEPS)
                w, a = in_mode(ch.labels(), labels, N)
            whole.append(w)
            agree.append(a)
        out[init] = {"in_generating_mode": int(sum(whole)), "of": nseeds, "mean_final_agreement": float(np.mean(agree))}
        if rounds:
            out[init]["rounds_run"] = spread(rounds)
    return out


if __name__ == "__main__":
    if sys.argv[1] == "time":
        print(json.dumps(time_shape(sys.argv[2])))
    elif sys.argv[1] == "trap":
        print(json.dumps(trap(int(float(sys.argv[2])), int(sys.argv[3]))))
    elif sys.argv[1] == "merge":
        parts = [json.loads(open(f).read().strip().splitlines()[-1]) for f in sys.argv[2:]]
        with open(os.path.join(ROOT, "profiles", "init_probe.json"), "w") as f:
            json.dump({"timing": [p for p in parts if "shape" in p], "mode_trapping": [p for p in parts if "seeds" in p]}, f, indent=1)
            f.write("\n")
