#!/usr/bin/env python3
"""What the split-merge moves of the DP chain cost and what they buy.
  time    per move at c3 (gibbs_dp, N = 1e6) and at N = 4e5, beside the sweep time of the same run: host clock around
          whole synchronised calls after a warm-up, a per-unit figure being the difference of two calls that differ only
          in the number of units (best of three), as tools/loo_probe.py does;
  seeds   for the ten seeds of tools/dp_seed_scan.py (N = 4e5, five generating components): the clusters above N/1000
          at the end of the run, without moves and with `moves` moves per sweep, for each number of scans given.
Usage: python tools/split_merge_probe.py [moves_per_sweep [scans ...]]      (default 4 moves; scans 0 2 5)
Writes profiles/split_merge_probe.json and prints it."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bmm_mcmc_amd as bm  # noqa: E402
from bmm_mcmc_amd import synth  # noqa: E402


def per_unit(step, n1, n2, reps=3):
    vals = []
    for _ in range(reps):
        t = []
        for n in (n1, n2):
            t0 = time.perf_counter()
            step(n)
            t.append((time.perf_counter() - t0) * 1e3)
        vals.append((t[1] - t[0]) / (n2 - n1))
    return min(vals)


def timing(name, N, P, K, K_true, dseed, scans_list):
    X = synth.host_matrix(N, P, K_true, dseed)[0]
    out = {"shape": name, "N": N, "P": P, "maxK": K}
    with bm.Chain("dp", N, P, K, seed=3) as c:
        c.set_data(X)
        c.sweeps(30)
        c.sync()

        def sweeps(n):
            c.sweeps(n)
            c.sync()

        def moves(n):
            c.split_merge(n)
            c.sync()
        sweeps(5)
        out["ms_sweep"] = round(per_unit(sweeps, 5, 25), 4)
        out["ms_move"] = {}
        for scans in scans_list:
            c.set_split_merge(1, scans)
            c.set_split_merge(0, scans)
            moves(5)
            out["ms_move"][str(scans)] = round(per_unit(moves, 5, 45), 4)
        out["stats"] = c.split_merge_stats()
    return out


def seeds(moves, scans_list, first=11, n=10):
    K, K_true, N, P = 30, 5, 400_000, 50
    X = synth.host_matrix(N, P, K_true, 77)[0]
    rows = []
    for seed in range(first, first + n):
        row = {"seed": seed}
        for scans in [None] + list(scans_list):
            with bm.Chain("dp", N, P, K, seed=seed) as c:
                c.set_data(X)
                if scans is not None:
                    c.set_split_merge(moves, scans)
                c.sweeps(150)
                counts = c.sweeps_counts(60)
                key = "none" if scans is None else "scans_%d" % scans
                row[key] = int((counts[-1] > N / 1000).sum())
                if scans is not None:
                    row[key + "_stats"] = c.split_merge_stats()
        rows.append(row)
        print(row, file=sys.stderr)
    return rows


def main():
    moves = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    scans_list = [int(v) for v in sys.argv[2:]] or [0, 2, 5]
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS["c3"]
    assert sampler == "dp"
    out = {"moves_per_sweep": moves, "scans": scans_list,
           "timing": [timing("c3", N, P, K, K_true, dseed, scans_list), timing("N4e5", 400_000, 50, 30, 5, 77, scans_list)],
           "seeds": seeds(moves, scans_list)}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "split_merge_probe.json"), "w") as f:
        json.dump({"split_merge_probe": out}, f, indent=1)
        f.write("\n")
    print(json.dumps({"split_merge_probe": out}))


if __name__ == "__main__":
    main()
