"""Cases and digests that pin what the count-table builds and the stored-state scorers compute, bit for bit.

The table image of a counting chain (kernels.hip.h: the sweep's build, the allocation sampler's, the one the resample
workgroups make for themselves, the predictive's and the leave-one-out's) decides every label drawn and every
predictive value, so SHA-256 digests of the raw bytes of labels, counts, hand-off probabilities, predictive and
leave-one-out values show a reordered sum or a moved guard that a tolerance would let through.  The digests in
tests/golden/state_score_pins.json were recorded from the commit before the builds were folded into one statement of
the rules (bmm_spec.h "count-table rules"); tests/test_gpu_state_score_pins.py holds every later build to them.

Record (from a tree that has been built, on the device):
    python tests/state_score_pins.py --root TREE --record FILE
imports the library from TREE, so an exported copy of another commit can be recorded with this module's cases.  Two
recordings of one tree must be byte-equal before a file is worth committing.

Shapes are the smallest at which each copy of the rules could go wrong; see the comment at each group."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "golden", "state_score_pins.json")
ENV = {"CUS": "BMM_DEBUG_CUS", "NOSELF": "BMM_DEBUG_NOSELF"}   # the test variant's switches the cases use
BETA_GAMMA = {"collapsed": (0.7, 0.4), "dp": (0.5, 0.5), "stickbreaking": (0.3, 1.1), "full": (0.7, 0.4)}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def data(N, P, seed):
    """three planted components, rates 0.1 + 0.8 U (tests/util.py synth, restated so that the recorder needs no path).
    From 100 features on the rates are 0.42 + 0.16 U: with crisp rates that many features fix every row's label after
    a sweep or two, and a chain that stands still pins nothing past its first state."""
    rng = np.random.Generator(np.random.PCG64(seed))
    theta = 0.1 + 0.8 * rng.random((3, P)) if P < 100 else 0.42 + 0.16 * rng.random((3, P))
    lab = rng.integers(3, size=N)
    return np.asfortranarray((rng.random((N, P)) < theta[lab]).astype(np.int32))


def edge_labels(N, K, seed):
    """labels 1, 2 and 4 hold the rows but for one row on label 3: label 3 has a single row (the n > 1 edge), label 5
    and every later one none (the n > 0 edge)"""
    z = np.random.default_rng(seed).choice([1, 2, 4], N).astype(np.int32)
    z[N // 2] = 3
    assert K >= 5
    return z


# ------------------------------------------------------------------------------------------------ the cases
# name -> spec.  kind "sweep": labels after every sweep, counts, the hand-off probabilities of one more sweep.
# kind "score": one sweep, then predict_state / loo_state, three sweeps folded into the predictive, three into the
# leave-one-out summary.  env: the test variant's switches.  kt, packed: the accumulator count and the packed kernel,
# asserted through the test variant's bmm_dbg_kernel_key / bmm_dbg_kernel_packed.  A case with any of the three runs on
# the -DBMM_DEBUG_HOOKS library (same kernels, compiled from the same source).  still: a chain that cannot move.
def _cases():
    c = {}

    def sweep(name, sampler, N, P, K, **kw):
        c[name] = dict(kind="sweep", sampler=sampler, N=N, P=P, K=K, sweeps=kw.pop("sweeps", 5), **kw)

    def score(name, sampler, N, P, K, M, **kw):
        c[name] = dict(kind="score", sampler=sampler, N=N, P=P, K=K, M=M, **kw)

    # the sweep's builds.  K = 3, P = 20: 255 logs, the workgroups build their own image (SELF) -- and not, under NOSELF
    sweep("sweep-fin-K3-P20-self", "collapsed", 600, 20, 3, own=True)
    sweep("sweep-fin-K3-P20-noself", "collapsed", 600, 20, 3, env={"NOSELF": 1}, own=False)
    sweep("sweep-fin-K5-P33", "collapsed", 600, 33, 5)
    # P = 125: a second trip of the 120-feature chunk loop, groups that cross a word
    sweep("sweep-fin-K4-P125", "collapsed", 500, 125, 4)
    sweep("sweep-dp-K6-P125", "dp", 500, 125, 6)
    sweep("sweep-fin-K20-P112-width4", "collapsed", 700, 112, 20, width=4)
    sweep("sweep-fin-K3-P130-generic", "collapsed", 400, 130, 3)
    sweep("sweep-sb-K70-generic", "stickbreaking", 400, 10, 70)
    # a start with an empty label and a single-row label
    sweep("sweep-fin-K7-edges", "collapsed", 500, 20, 7, edges=True)
    sweep("sweep-dp-K9-edges", "dp", 500, 20, 9, edges=True)
    # a mask that excludes features in both words of P = 40 (p_in of the DP's new cluster)
    sweep("sweep-fin-K4-P40-mask", "collapsed", 500, 40, 4, mask=(3, 17, 35, 39))
    sweep("sweep-dp-K6-P40-mask", "dp", 500, 40, 6, mask=(3, 17, 35, 39))
    # one CU and 4500 rows: more than four chunks per wave, so the packed kernel runs and the packed image is written
    sweep("sweep-fin-K3-P20-packed", "collapsed", 4500, 20, 3, env={"CUS": 1}, sweeps=4, batch=4500, packed=True, kt=4)
    # the allocation sampler, maxK = 8: planted data of tests/alloc_sweep_cases.py (comps, loners, per, coins, crowd)
    sweep("alloc-open1", "collapsed", 300, 33, 8, alloc=dict(K_open=1, plant=(1, 0, 1, 4, 0)), batch=64, still=True)  # (one open label: every row stays)
    sweep("alloc-open3", "collapsed", 300, 33, 8, alloc=dict(K_open=3, plant=(1, 1, 2, 2, 0)), batch=64)
    sweep("alloc-open8", "collapsed", 300, 33, 8, alloc=dict(K_open=8, plant=(3, 3, 1, 3, 4)), batch=64)
    sweep("alloc-set-k", "collapsed", 0, 0, 8, alloc=dict(schedule=True), sweeps=6)
    # the stored-state scorers: every sampler at 4, 32 and 40 accumulators (at 40 a counting chain's own-label rows
    # go to the generic leave-one-out kernel: lookup_score has no own-label form above 32); 700 fitted and 530 new
    # rows: no multiple of 512
    for kt in (4, 32, 40):
        score("score-fin-KT%d" % kt, "collapsed", 700, 20, kt - 2 if kt > 4 else 3, 530, kt=kt)
        score("score-dp-KT%d" % kt, "dp", 700, 20, kt - 1, 530, kt=kt)
        score("score-sb-KT%d" % kt, "stickbreaking", 700, 20, kt, 530, kt=kt)
        score("score-full-KT%d" % kt, "full", 700, 20, kt, 530, kt=kt)
    score("score-fin-K20-P112-width4", "collapsed", 700, 112, 20, 530, width=4)
    score("score-fin-K3-P130-generic", "collapsed", 400, 130, 3, 300)
    score("score-fin-K3-P130-generic-int32", "collapsed", 400, 130, 3, 300, layout="int32")
    # one CU: more tiles than workgroups, the next tile's words are prefetched
    score("score-fin-K5-P33-tiles", "collapsed", 3000, 33, 5, 2700, env={"CUS": 1})
    score("score-dp-K6-P33-tiles", "dp", 3000, 33, 6, 2700, env={"CUS": 1})
    score("score-fin-K7-edges", "collapsed", 500, 20, 7, 300, edges=True)
    score("score-dp-K9-edges", "dp", 500, 20, 9, 300, edges=True)
    # theta-hat of short runs
    for s in ("collapsed", "dp", "stickbreaking", "full", "allocation"):
        c["run-" + s] = dict(kind="run", sampler=s)
    return c


CASES = _cases()


def uses_test_variant(s):
    return bool(s.get("env")) or "kt" in s or "packed" in s


PRODUCT_CASES = [n for n, s in CASES.items() if not uses_test_variant(s)]
SWITCHED_CASES = [n for n, s in CASES.items() if uses_test_variant(s)]


# ------------------------------------------------------------------------------------------------ running one
def _start(bm, s, seed):
    sampler, N, P, K = s["sampler"], s["N"], s["P"], s["K"]
    beta, gamma = BETA_GAMMA[sampler]
    al = s.get("alloc")
    z0 = None
    if al:
        import alloc_sweep_cases as ac
        beta, gamma = 0.5, 0.5
        if al.get("schedule"):
            X, z0 = ac.k_start()
            N, P, s = ac.K_N, ac.K_P, dict(s, batch=ac.K_BATCH)
        else:
            comps, loners, per, coins, crowd = al["plant"]
            X, z0 = ac.planted(N, P, comps, loners, per, coins, s["batch"], 5, crowd)
    else:
        X = data(N, P, seed)
    c = bm.Chain(sampler, N, P, K, alpha=1.0 if al else 1.3, beta=beta, gamma=gamma, batch=s.get("batch"), seed=seed,
                 x_layout=s.get("layout"))
    if "width" in s:
        from bmm_mcmc_amd import _capi
        assert _capi.lib().bmm_spec_group_width_for(_capi.SAMPLER_CODE[sampler], K, P) == s["width"]
    c.set_data(X)
    rng = np.random.default_rng(seed)
    if sampler == "collapsed":
        if z0 is None:
            z0 = edge_labels(N, K, seed) if s.get("edges") else rng.integers(1, K + 1, N).astype(np.int32)
        c.set_initial_labels(z0)
    elif sampler in ("stickbreaking", "full"):
        c.set_initial_params(rng.dirichlet(np.ones(K)), np.asfortranarray(0.05 + 0.9 * rng.random((K, P))))
    if s.get("mask"):
        g = np.ones(P, dtype=np.uint8)
        g[list(s["mask"])] = 0
        c.set_features(g)
    if al:
        c.set_alloc("uniform", 0)
        if "K_open" in al:
            c.set_k(al["K_open"])
    return c, X


def _check_path(c, s):
    """the kernel the chain chose is the one the case is for"""
    import ctypes
    from bmm_mcmc_amd import _capi
    if "kt" in s:
        key = (ctypes.c_int * 10)()
        _capi.check(_capi.lib().bmm_dbg_kernel_key(c._h, key))
        assert key[0] == s["kt"], (tuple(key), s["kt"])
    if s.get("packed"):
        assert _capi.lib().bmm_dbg_kernel_packed(c._h) == 1


def _moved(out, keys, s):
    """the states a case pins differ from one another, unless the chain cannot move"""
    assert s.get("still") or len({out[k] for k in keys}) > 1, keys


def _seat_edges(c, s, seed):
    """the DP chain is seated by its first sweep; the edge labels replace that allocation"""
    if s.get("edges") and s["sampler"] == "dp":
        c.set_labels(edge_labels(s["N"], s["K"], seed))


def _run_sweep(bm, s, seed, out):
    c, X = _start(bm, s, seed)
    with c:
        shape = c.kernel_shape()
        if "own" in s:
            assert shape["builds_own_tables"] == s["own"], shape
        al = s.get("alloc") or {}
        for j in range(s["sweeps"]):
            if al.get("schedule"):
                import alloc_sweep_cases as ac
                c.set_k(ac.k_schedule(j, c.labels(), c.k()))
                out["K%d" % j] = str(c.k())
            c.sweeps(1)
            if j == 0:
                _seat_edges(c, s, seed)
            out["z%d" % (j + 1)] = sha(c.labels())
        _check_path(c, s)
        _moved(out, ["z%d" % (j + 1) for j in range(2, s["sweeps"])], s)   # still moving from the third sweep on
        Nk, S = c.counts()
        out["Nk"], out["S"] = sha(Nk), sha(S)
        if not al:
            out["probs"] = sha(c.sweep_probs())
            out["z_after_probs"] = sha(c.labels())


def _run_score(bm, s, seed, out):
    c, X = _start(bm, s, seed)
    Xnew = data(s["M"], s["P"], seed + 1000)
    with c:
        c.set_newdata(Xnew, responsibilities=True)
        c.set_loo()
        # (the finite sampler's edge labels are its start: scored before a sweep moves the single row)
        c.sweeps(0 if s.get("edges") and s["sampler"] == "collapsed" else 1)
        _seat_edges(c, s, seed)
        _check_path(c, s)
        if s.get("edges"):
            Nk = c.counts()[0]
            assert (Nk == 0).any() and (Nk == 1).any(), Nk
        ld, rp = c.predict_state(responsibilities=True)
        out["predict_state"], out["predict_state_resp"] = sha(ld), sha(rp)
        out["loo_state"] = sha(c.loo_state())
        for j in range(3):
            out["predict_trace%d" % j] = sha(c.sweeps_predict(1, trace=True))
            out["z_p%d" % j] = sha(c.labels())
        pr = c.predictive(responsibilities=True)
        assert pr["n"] == 3
        out["predictive_lppd"], out["predictive_resp"] = sha(pr["lppd"]), sha(pr["resp"])
        for j in range(3):
            out["loo_trace%d" % j] = sha(c.sweeps_loo(1, trace=True))
            out["z_l%d" % j] = sha(c.labels())
        _moved(out, ["predict_trace%d" % j for j in range(3)], s)
        _moved(out, ["loo_trace%d" % j for j in range(3)], s)
        lo = c.loo()
        assert lo["n_folded"] == 3
        for k in sorted(lo):
            if k != "n_folded":
                out["loo_" + k] = sha(np.asarray(lo[k], dtype=np.float64))
        Nk, S = c.counts()
        out["Nk"], out["S"] = sha(Nk), sha(S)


def _run_run(bm, s, seed, out):
    X = data(600, 20, seed)
    z0 = np.random.default_rng(seed).integers(1, 4, 600).astype(np.int32)
    sampler = s["sampler"]
    if sampler == "collapsed":
        r = bm.gibbs_collapsed(X, 6, 3, burnin=1, seed=seed, batch=256, initial_K=z0)
    elif sampler == "dp":
        r = bm.gibbs_dp(X, 6, burnin=1, seed=seed, maxK=10)
    elif sampler == "stickbreaking":
        r = bm.gibbs_stickbreaking(X, 6, 10, burnin=1, seed=seed)
    elif sampler == "full":
        r = bm.gibbs_full(X, 6, 4, burnin=1, seed=seed)
    else:
        r = bm.gibbs_allocation(X, 6, 8, a=1.0, prior_k="uniform", K0=4, moves=1, burnin=1, seed=seed, batch=256, initial_K=z0)
    out["theta"], out["z"] = sha(r["theta"]), sha(r["z"])


def digests(bm, name):
    """{what: sha256 hex (or a short plain value)} of one case, on whatever library `bm` has loaded"""
    s = CASES[name]
    seed = 100 + sorted(CASES).index(name)
    out = {}
    {"sweep": _run_sweep, "score": _run_score, "run": _run_run}[s["kind"]](bm, s, seed, out)
    return out


def set_switches(env, setenv, delenv):
    for k, var in ENV.items():
        if env and env.get(k):
            setenv(var, str(int(env[k])))
        else:
            delenv(var)


def load_pins():
    with open(PINS) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ the recorder
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True, help="the tree whose library is recorded")
    ap.add_argument("--record", required=True, help="the JSON file to write")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(1, HERE)
    import bmm_mcmc_amd as bm
    from bmm_mcmc_amd import _capi, build
    assert os.path.abspath(bm.__file__).startswith(root + os.sep), bm.__file__
    product, switched = _capi.load(build.LIB), _capi.load(build.LIB_DBG)
    rec = {}
    for name in sorted(CASES):
        env = CASES[name].get("env")
        _capi._LIB = switched if uses_test_variant(CASES[name]) else product
        set_switches(env, os.environ.__setitem__, lambda v: os.environ.pop(v, None))
        rec[name] = digests(bm, name)
        print(name, len(rec[name]), flush=True)
    with open(a.record, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
