#!/usr/bin/env python3
"""What the split-merge moves of the allocation sampler cost and whether K is found with them.
  time    per move at c2 (K = 3, N = 1e5, P = 20; maxK = 3) and at the north-star shape (N = 1e6, P = 50, 20 generating
          components) with maxK = 30, beside the sweep and the eject / absorb move of the same armed chain: host clock
          around whole synchronised calls after a warm-up, a per-unit figure being the difference of two calls that
          differ only in the number of units (best of three), as tools/alloc_probe.py does; and the counts of the moves;
  seeds   section 18's experiment with the moves on: for ten seeds on planted data (five generating components, P = 50)
          at each N given, from K0 = 2 and uniform labels, 150 + 150 sweeps: the posterior mode of K and of the number
          of non-empty labels over the kept sweeps, and the counts of both kinds of move.
Usage: python tools/alloc_split_probe.py [--out FILE] [split_merge_per_sweep [N ...]]     (default 2 moves; N 2000 400000)
Writes profiles/alloc_split_probe.json (or FILE) and prints it."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bmm_mcmc_amd as bm  # noqa: E402
from bmm_mcmc_amd import synth  # noqa: E402

A, BURN, KEPT, K_TRUE, EA_MOVES = 1.0, 150, 150, 5, 4
SCANS = bm.SPLIT_MERGE_SCANS


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


def rates(st):
    out = dict(st)
    for kind in ("splits", "merges"):
        n = st["proposed_" + kind]
        out[kind + "_rate"] = round(st["accepted_" + kind] / n, 4) if n else None
    return out


def timing(name, N, P, maxK, K_true, dseed):
    X = synth.host_matrix(N, P, K_true, dseed)[0]
    out = {"shape": name, "N": N, "P": P, "maxK": maxK, "K0": K_true, "scans": SCANS}
    with bm.Chain("collapsed", N, P, maxK, alpha=A, seed=3) as c:
        c.set_data(X)
        c.set_initial_labels(np.random.default_rng(3).integers(1, K_true + 1, N).astype(np.int32))
        c.set_alloc("poisson", 0)
        c.set_k(K_true)
        c.set_alloc_split_merge(0, SCANS)
        c.sweeps(30)
        c.sync()

        def sweeps(n):
            c.sweeps(n)
            c.sync()

        def ea(n):
            c.alloc(n)
            c.sync()

        def moves(n):
            c.alloc_split_merge(n)
            c.sync()
        sweeps(5)
        out["ms_sweep"] = round(per_unit(sweeps, 5, 25), 4)
        ea(5)
        out["ms_eject_absorb"] = round(per_unit(ea, 5, 45), 4)
        moves(5)
        out["ms_move"] = round(per_unit(moves, 5, 45), 4)
        out["K_end"] = c.k()
        out["stats"] = rates(c.alloc_split_merge_stats())
    return out


def mode(v, n):
    return int(np.bincount(np.asarray(v), minlength=n + 1).argmax())


def seeds(N, moves, maxK=30, P=50, first=11, n=10):
    X = synth.host_matrix(N, P, K_TRUE, 77)[0]
    rows = []
    for seed in range(first, first + n):
        with bm.Chain("collapsed", N, P, maxK, alpha=A, seed=seed) as c:
            c.set_data(X)
            c.set_initial_labels(np.random.default_rng(seed).integers(1, 3, N).astype(np.int32))
            c.set_alloc("poisson", EA_MOVES)
            c.set_k(2)
            c.set_alloc_split_merge(moves, SCANS)
            c.sweeps(BURN)
            Ks, used = [], []
            for _ in range(KEPT):
                c.sweeps(1)
                Ks.append(c.k())
                used.append(int((c.counts()[0] > 0).sum()))
            row = {"seed": seed, "K_mode": mode(Ks, maxK), "K_min": min(Ks), "K_max": max(Ks),
                   "used_mode": mode(used, maxK), "split_merge": rates(c.alloc_split_merge_stats()), "eject_absorb": c.alloc_stats()}
        rows.append(row)
        print(row, file=sys.stderr)
    return {"N": N, "P": P, "maxK": maxK, "K_generating": K_TRUE, "burn": BURN, "kept": KEPT,
            "K_mode_equals_generating": sum(r["K_mode"] == K_TRUE for r in rows),
            "used_mode_equals_generating": sum(r["used_mode"] == K_TRUE for r in rows), "rows": rows}


def main():
    argv = sys.argv[1:]
    dest = os.path.join(ROOT, "profiles", "alloc_split_probe.json")
    if argv[:1] == ["--out"]:
        dest, argv = argv[1], argv[2:]
    moves = int(argv[0]) if argv else 2
    Ns = [int(v) for v in argv[1:]] or [2000, 400_000]
    sampler, K, K_true, N, P, dseed = synth.WORKLOADS["c2"]
    assert sampler == "collapsed"
    _, _, ns_true, ns_N, ns_P, ns_seed = synth.WORKLOADS["ns"]
    out = {"a": A, "prior_k": "poisson", "eject_absorb_per_sweep": EA_MOVES, "split_merge_per_sweep": moves, "scans": SCANS,
           # (at c2 every label is open, K = maxK = 3: a split there is skipped, which the counts show; the second row
           # gives the same shape one label of room)
           "timing": [timing("c2", N, P, K, K_true, dseed), timing("c2-maxK4", N, P, K + 1, K_true, dseed),
                      timing("ns", ns_N, ns_P, 30, ns_true, ns_seed)],
           "seeds": [seeds(n, moves) for n in Ns]}
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    with open(dest, "w") as f:
        json.dump({"alloc_split_probe": out}, f, indent=1)
        f.write("\n")
    print(json.dumps({"alloc_split_probe": out}))


if __name__ == "__main__":
    main()
