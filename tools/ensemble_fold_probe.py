"""What the folds on ensemble chains cost, and that a run without them costs what it did.

Folds: chain-sweeps per second of bm.gibbs_ensemble at 256 chains with nothing asked, with loo=True and with newdata= (M = N
rows) on the bundled K3_N1000_P5 (K = 3) and on the K = 20, P = 50, N = 4096 mixture of section 31; the host clock around
two calls that differ in their sweeps only, so start-up, packing and the copies of the results cancel.

Unarmed (`--parent-lib PATH`, a build of the commit before the feature): tools/ensemble_probe.py --only speed run as a
child process on that library and on this tree's, alternating, `--rounds` times each; both series of chain-sweeps/s are
kept, with the parent's own run-to-run spread and whether this tree's rates lie inside it.

Writes profiles/ensemble_fold_probe.json (or --out), merging the part that ran into what is there, and prints it as one
JSON line.

    python tools/ensemble_fold_probe.py [--only folds|unarmed] [--parent-lib PATH] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "ensemble_fold_probe.json")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CHAINS = 256


def bundled(name):
    with open(os.path.join(GOLDEN, name + ".txt")) as f:
        return np.asfortranarray(np.array([[int(c) for c in line.strip()] for line in f if line.strip()], dtype=np.int32))


def mixture(N, P, K, seed):
    rng = np.random.default_rng(seed)
    theta = 0.1 + 0.8 * rng.random((K, P))
    lab = rng.integers(0, K, N)
    return np.asfortranarray((rng.random((N, P)) < theta[lab]).astype(np.int32))


def wall(fn, reps=3):
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        s = time.perf_counter() - t
        best = s if best is None or s < best else best
    return best


def fold_shape(bm, name, X, K, n1, n2):
    """every sweep of the timed calls is a kept one (burnin = 1), so every sweep is followed by its folds"""
    N, P = X.shape
    Xn = np.asfortranarray(1 - X)  # M = N rows over the same columns
    rows = {}
    for what, opts in (("nothing", {}), ("loo", dict(loo=True)), ("newdata_M_eq_N", dict(newdata=Xn))):
        def run(n):
            bm.gibbs_ensemble(X, n + 1, K, chains=CHAINS, burnin=1, seed=7, keep_trace=False, **opts)
        run(2)  # warm
        s = (wall(lambda: run(n2)) - wall(lambda: run(n1))) / (n2 - n1)
        rows[what] = {"ms_per_sweep_of_the_ensemble": round(s * 1e3, 4), "chain_sweeps_per_s": round(CHAINS / s, 1)}
    base = rows["nothing"]["ms_per_sweep_of_the_ensemble"]
    plan = bm.ensemble_plan("collapsed", N, P, K, CHAINS)
    for what in ("loo", "newdata_M_eq_N"):
        ms = rows[what]["ms_per_sweep_of_the_ensemble"] - base
        rows[what]["ms_of_the_fold"] = round(ms, 4)
        rows[what]["fold_over_one_sweep_launch"] = round(ms / (base / plan["launches_per_sweep"]), 4)
    return {"data": name, "N": N, "P": P, "K": K, "chains": CHAINS, "sweeps_timed": [n1, n2],
            "launches_per_sweep": plan["launches_per_sweep"], "rates": rows,
            "fold_plan_loo": bm.ensemble_fold_plan("collapsed", N, P, K, CHAINS, loo=True),
            "fold_plan_newdata": bm.ensemble_fold_plan("collapsed", N, P, K, CHAINS, M=N)}


def folds():
    import bmm_mcmc_amd as bm
    return [fold_shape(bm, "K3_N1000_P5", bundled("K3_N1000_P5"), 3, 20, 80),
            fold_shape(bm, "mixture K20 P50 N4096, data seed 11", mixture(4096, 50, 20, 11), 20, 4, 16)]


def probe_speed(lib):
    """the `speed` part of tools/ensemble_probe.py in a child process on one build of the library"""
    env = dict(os.environ)
    if lib:
        env["BMM_LIB_PATH"] = lib
    else:
        env.pop("BMM_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ensemble_probe.py"), "--only", "speed"], env=env, capture_output=True,
                       text=True, check=True)
    speed = json.loads(r.stdout.strip().splitlines()[-1])["ensemble_probe"]["speed"]
    return {"%s chains=%d" % (s["data"], e["chains"]): e["chain_sweeps_per_s"] for s in speed for e in s["ensemble"]}


def unarmed(parent_lib, rounds):
    saved = os.path.join(ROOT, "profiles", "ensemble_probe.json")
    with open(saved) as f:
        keep = f.read()  # (the child writes its own record there: put back afterwards)
    series = {"parent": [], "this_tree": []}
    try:
        for _ in range(rounds):
            series["parent"].append(probe_speed(parent_lib))
            series["this_tree"].append(probe_speed(None))
    finally:
        with open(saved, "w") as f:
            f.write(keep)
    verdict = {}
    for key in series["parent"][0]:
        p = [r[key] for r in series["parent"]]
        t = [r[key] for r in series["this_tree"]]
        verdict[key] = {"parent": p, "this_tree": t, "parent_min": min(p), "parent_max": max(p),
                        "this_tree_inside_the_parents_spread": [min(p) <= v <= max(p) for v in t],
                        "this_tree_median_over_parent_median": round(float(np.median(t) / np.median(p)), 4)}
    return {"what": "chain-sweeps/s of tools/ensemble_probe.py --only speed, no fold asked, alternating parent, this tree",
            "rounds": rounds, "rates": verdict}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    res = {}
    for path in (a.out, OUT):
        if os.path.exists(path):
            with open(path) as f:
                res = json.load(f).get("ensemble_fold_probe", {})
            break
    if a.only in (None, "folds"):
        res["folds"] = folds()
    if a.only in (None, "unarmed") and a.parent_lib:
        res["unarmed"] = unarmed(os.path.abspath(a.parent_lib), a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps({"ensemble_fold_probe": res}, indent=1) + "\n")
    print(json.dumps({"ensemble_fold_probe": res}))


if __name__ == "__main__":
    main()
