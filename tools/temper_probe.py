#!/usr/bin/env python3
"""What parallel tempering costs and what it buys, on the device.
(a) sweeps/s of a ladder of 4 at the north-star shape (ns) and at C2 -- every rung counted, as four chains are -- against
    four independent chains over shared planes advanced by bm.sweep_chains: the difference is the price of the exchange
    points (and of the tempered table kernel and the plainer kernel plan of the helpers).  --baseline-only measures the
    independent chains alone and calls nothing this feature added, so that it runs against a build of the parent commit
    (BMM_LIB_PATH) on the same box.
(b) the criterion of tests/tools/mode_trap_scan.py -- every generating component held by exactly one cluster above
    N/1000 rows in the final allocation -- for a plain chain and for the cold chain of ladders of 4 and 8, on the K = 20,
    P = 50 mixture at N = 1e3, 1e4 and 1e5 from uniformly random starts, at equal numbers of cold sweeps, with the
    exchange rates per pair.
Host clock around whole synchronised calls after a warm-up.  Prints one JSON line."""
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

SWEEPS = {"ns": (20, 120), "c2": (100, 1100)}
HOTTEST = 0.7               # the ladder of (a): geometric from 1 down to this
TRAP_HOTTEST = (0.7, 0.95)  # the ladders of (b): a wide one and a narrow one


def rate(step, sync, n1, n2, reps=3):
    """sweeps per second and chain: n2 - n1 sweeps over the difference of the two calls' times, best of `reps`"""
    best = 0.0
    for _ in range(reps):
        t = []
        for n in (n1, n2):
            t0 = time.perf_counter()
            step(n)
            sync()
            t.append(time.perf_counter() - t0)
        best = max(best, (n2 - n1) / (t[1] - t[0]))
    return best


def four_chains(wl, tempered):
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS[wl]
    X, _ = synth.device_matrix(N, P, K_true, dseed, torch.device("cuda", 0))
    z0 = np.random.default_rng(1).integers(1, K + 1, N).astype(np.int32)
    powers = bm.temper_ladder(4, HOTTEST) if tempered else [1.0] * 4
    chains = []
    for r in range(4):
        c = bm.Chain(sampler, N, P, K, alpha=1.0, seed=3 + r)
        if r == 0:
            c.set_data_device(X.data_ptr(), keepalive=X)
        else:
            c.share_data(chains[0])
        c.set_initial_labels(z0)
        if tempered and r > 0:
            c.set_temper(powers[r])
        chains.append(c)
    return chains


def throughput(wl, baseline_only):
    n1, n2 = SWEEPS[wl]
    out = {"shape": wl}

    def sync_all(chains):
        for c in chains:
            c.sync()
    chains = four_chains(wl, False)
    bm.sweep_chains(chains, 30)
    sync_all(chains)
    out["independent_x4_sweeps_per_s"] = round(4 * rate(lambda n: bm.sweep_chains(chains, n), lambda: sync_all(chains), n1, n2), 1)
    for c in chains[::-1]:
        c.close()
    if baseline_only:
        return out
    for swap_every in (1, 10):
        chains = four_chains(wl, True)
        with bm.Ladder(chains, seed=9) as lad:
            lad.sweeps(30, swap_every)
            sync_all(chains)
            out["ladder_x4_swap_every_%d_sweeps_per_s" % swap_every] = round(
                4 * rate(lambda n: lad.sweeps(n, swap_every), lambda: sync_all(chains), n1, n2), 1)
            st = lad.stats()
            out["ladder_x4_swap_every_%d_rates" % swap_every] = (st["accepted"] / np.maximum(st["proposed"], 1)).round(4).tolist()
        for c in chains[::-1]:
            c.close()
    out["exchange_price"] = round(1.0 - out["ladder_x4_swap_every_1_sweeps_per_s"] / out["independent_x4_sweeps_per_s"], 4)
    return out


def in_generating_mode(z1, labels, K, K_true, N):
    tab = np.zeros((K, K_true), dtype=np.int64)
    np.add.at(tab, (z1 - 1, labels), 1)
    owner, big = tab.argmax(axis=1), tab.sum(axis=1) > N // 1000
    return all(int((big & (owner == c)).sum()) == 1 for c in range(K_true))


def mode_trap(N, seeds, sweeps):
    K, P = 20, 50
    X, labels, _, _ = synth.host_matrix(N, P, K, 22)
    out = {"N": N, "K": K, "P": P, "cold_sweeps": sweeps, "seeds": seeds}
    for R, hottest in [(1, None)] + [(R, h) for h in TRAP_HOTTEST for R in (4, 8)]:
        hits, rates = 0, []
        t0 = time.perf_counter()
        for s in range(seeds):
            r = bm.gibbs_collapsed(X, sweeps + 1, K, burnin=sweeps, seed=2000 + s, temper=None if R == 1 else R,
                                   temper_hottest=hottest or 0.5)
            hits += int(in_generating_mode(r["z"][-1], labels, K, K, N))
            if R > 1:
                rates.append(r["temper"]["rate"])
        key = "plain" if R == 1 else "ladder_%d_hottest_%g" % (R, hottest)
        out[key] = {"in_generating_mode": hits, "of": seeds, "seconds": round(time.perf_counter() - t0, 2)}
        if R > 1:
            out[key]["inv_temp"] = bm.temper_ladder(R, hottest).round(4).tolist()
            out[key]["mean_rate_per_pair"] = np.nanmean(np.array(rates), axis=0).round(4).tolist()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ns,c2")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--trap", default="1000:24:300,10000:24:300,100000:12:300", help="N:seeds:sweeps,... ('' skips part (b))")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    out = {"tag": args.tag, "throughput": [throughput(wl, args.baseline_only) for wl in args.shapes.split(",") if wl]}
    if not args.baseline_only and args.trap:
        out["mode_trap"] = [mode_trap(*(int(float(v)) for v in job.split(":"))) for job in args.trap.split(",")]
    print(json.dumps({"temper_probe": out}))


if __name__ == "__main__":
    main()
