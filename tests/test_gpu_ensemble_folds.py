"""Leave-one-out and held-out predictive on every chain of an ensemble (include/bmm_mcmc.h): chain c
of bm.gibbs_ensemble(..., loo=..., newdata=...) against the batch = 1 run of gibbs_collapsed / gibbs_dp under seed + c with
the same option, as raw bytes -- both sides are bmm_spec.h's arithmetic in k_score's order, so equality is the requirement
-- on the shapes where k_ens_score can go wrong; an independent pin against the NumPy restatements; and that a fold
changes nothing of the chains themselves."""
import numpy as np
import pytest

import bmm_mcmc_amd as bm
import loo_ref as lref
import predictive_ref as pref
from util import synth

pytestmark = pytest.mark.gpu

BETA = GAMMA = 0.5
RTOL = 1e-12  # tests/test_gpu_loo.py, tests/test_gpu_predict.py: 1-ulp log / exp and the order of the sums
LOO_KEYS = ("log_cpo", "ess", "lppd", "mean", "var")


def _same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes(), what


def _starts(seed, chains, K, N):
    return [np.ascontiguousarray(np.random.default_rng(seed + c).integers(1, K + 1, N), dtype=np.int32) for c in range(chains)]


def _three_label_starts(seed, chains, N):
    """starts that use labels 1, 2 and 4 of 5 only: labels 3 and 5 stay empty for ever"""
    return [np.ascontiguousarray(np.array([1, 2, 4], dtype=np.int32)[np.random.default_rng(seed + c).integers(0, 3, N)]) for c in range(chains)]


def _new_rows(X, M, seed):
    """M rows over X's columns, none of them a row of X"""
    rng = np.random.default_rng(seed)
    have = {r.tobytes() for r in np.ascontiguousarray(X)}
    assert len(have) < 2 ** min(X.shape[1], 30), "the rows of X cover the cube: no row is new"
    out = []
    while len(out) < M:
        r = (rng.random(X.shape[1]) < 0.5).astype(np.int32)
        if r.tobytes() not in have:
            out.append(r)
    return np.asfortranarray(np.array(out, dtype=np.int32))


def _any_rows(P, M, seed):
    """M rows over P columns, whether rows of the data or not"""
    return np.asfortranarray((np.random.default_rng(seed).random((M, P)) < 0.5).astype(np.int32))


def _single(sampler, X, nsamples, K, alpha, burnin, seed, z0, **opts):
    if sampler == "collapsed":
        return bm.gibbs_collapsed(X, nsamples, K, alpha=alpha, beta=BETA, gamma=GAMMA, burnin=burnin, seed=seed, batch=1, initial_K=z0, **opts)
    return bm.gibbs_dp(X, nsamples, alpha=alpha, beta=BETA, gamma=GAMMA, burnin=burnin, maxK=K, seed=seed, batch=1, **opts)


def _compare(got, want, what, loo, pred, trace=True):
    if loo:
        g, w = got["loo"], want["loo"]
        for key in LOO_KEYS + (("ell",) if trace else ()):
            _same_bytes(g[key], w[key], "%s loo %s" % (what, key))
        for key in ("lpml", "min_ess"):
            _same_bytes(np.float64(g[key]), np.float64(w[key]), "%s loo %s" % (what, key))
        assert g["n_folded"] == w["n_folded"], what
    if pred:
        g, w = got["predictive"], want["predictive"]
        _same_bytes(g["lppd"], w["lppd"], what + " predictive lppd")
        if trace:
            _same_bytes(g["logdens"], w["logdens"], what + " logdens")


def _ensemble_against_single(sampler, X, K, nsamples, chains, alpha, burnin, seed, Xn, initial_K=None):
    """the folds together, then each alone; every chain against the single run with the same option"""
    N = X.shape[0]
    z0s = None
    if sampler == "collapsed":
        z0s = initial_K if initial_K is not None else _starts(seed, chains, K, N)
    both = None
    for opts in (dict(loo="trace", newdata=Xn, predictive_trace=True), dict(loo="trace"), dict(newdata=Xn, predictive_trace=True)):
        outs = bm.gibbs_ensemble(X, nsamples, K, sampler=sampler, chains=chains, alpha=alpha, burnin=burnin, seed=seed,
                                 initial_K=initial_K, **opts)
        assert len(outs) == chains
        for c, got in enumerate(outs):
            assert ("loo" in got) == ("loo" in opts) and ("predictive" in got) == ("newdata" in opts)
            want = _single(sampler, X, nsamples, K, alpha, burnin, seed + c, None if z0s is None else z0s[c], **opts)
            _compare(got, want, "%s chain %d %s" % (sampler, c, sorted(opts)), "loo" in opts, "newdata" in opts)
            for key in ("z", "theta", "alpha"):
                _same_bytes(got[key], want[key], "%s chain %d %s" % (sampler, c, key))
            S = nsamples - burnin
            folded = S if burnin > 0 else S - 1
            for fold, tr in (("loo", "ell"), ("predictive", "logdens")):
                if fold in got:
                    assert got[fold]["n_folded"] == folded
                    assert got[fold][tr].shape[0] == S
                    assert np.isnan(got[fold][tr][0]).all() == (burnin == 0)  # row 0 of a run without burn-in is the start
                    assert np.isfinite(got[fold][tr][1 if burnin == 0 else 0:]).all()
        both = both or outs
    return both


# the DP shape of section 14's quirk: some kept state holds a cluster of one row.  The seed was chosen on the CPU with the
# oracle's batch = 1 chain (oracle_dp_run) before any device ran it: chain 0 under this seed has such a state with
# burn-in 0 and 3, the concentration sampled and fixed at 1.7, in all four pairings
SINGLETON_SEED = 1100

# (sampler, data, K or maxK, sweeps, new rows)
SHAPES = {
    "K2_P5_N130": ("collapsed", lambda: synth(130, 5, 2, 1)[0], 2, 10, 65),               # N no multiple of 64
    "K3_P7": ("collapsed", lambda: synth(200, 7, 3, 2)[0], 3, 8, 1),                      # a partial group; own groups 3 + 3 + 1
    "K5_P33_three_labels": ("collapsed", lambda: synth(257, 33, 3, 3)[0], 5, 6, 200),     # second plane word; empty labels
    "K20_P112": ("collapsed", lambda: synth(150, 112, 6, 4)[0], 20, 5, 65),               # group width 4; two launches a sweep
    "K64_P9": ("collapsed", lambda: synth(400, 9, 8, 5)[0], 64, 5, 200),                  # the single run's generic scorer
    "DP63_P12": ("dp", lambda: synth(200, 12, 5, 6)[0], 63, 6, 1),                        # Kc = 64
    "DP12_singleton": ("dp", lambda: synth(120, 10, 4, 21)[0], 12, 8, 65),                # a row that sits alone
}
# the concentration sampled and fixed, each with burn-in 0 and five chains and with burn-in 3 and one chain
VARIANTS = {
    "sampled_burn0_5chains": dict(alpha=None, burnin=0, chains=5),
    "fixed_burn3_1chain": dict(alpha=1.7, burnin=3, chains=1),
    "fixed_burn0_5chains": dict(alpha=1.7, burnin=0, chains=5),
    "sampled_burn3_1chain": dict(alpha=None, burnin=3, chains=1),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_chain_is_the_single_run_with_the_same_option(shape, variant):
    sampler, data, K, sweeps, M = SHAPES[shape]
    v = VARIANTS[variant]
    X = data()
    N, P = X.shape
    seed = SINGLETON_SEED if shape == "DP12_singleton" else 3000 + 17 * sorted(SHAPES).index(shape)
    nsamples = sweeps + 1 + v["burnin"]
    initial_K = _three_label_starts(seed, v["chains"], N) if shape == "K5_P33_three_labels" else None
    Xn = _new_rows(X, M, seed)
    outs = _ensemble_against_single(sampler, X, K, nsamples, v["chains"], v["alpha"], v["burnin"], seed, Xn, initial_K)
    plan = bm.ensemble_plan(sampler, N, P, K, v["chains"])
    if shape == "K20_P112":
        assert plan["group_width"] == 4 and plan["launches_per_sweep"] == 2
    if shape == "K5_P33_three_labels":  # finite labels that stay empty keep their prior weight
        for o in outs:
            assert (o["sizes"][:, [2, 4]] == 0).all()
    if shape == "DP12_singleton":
        kept = outs[0]["sizes"][1 if v["burnin"] == 0 else 0:]
        assert (kept == 1).any(), "no kept state holds a cluster of one row"


def test_a_sweep_over_several_launches():
    X = synth(2100, 5, 2, 9)[0]
    assert bm.ensemble_plan("collapsed", 2100, 5, 2, 2)["launches_per_sweep"] == 2
    Xn = _any_rows(5, 65, 4)  # (2100 rows cover all 32 patterns of P = 5)
    for sampler, K, chains, burnin, seed in (("collapsed", 2, 2, 1, 77), ("dp", 6, 1, 0, 78)):
        z0s = _starts(seed, chains, K, 2100) if sampler == "collapsed" else None
        opts = dict(loo="trace", newdata=Xn, predictive_trace=True)
        outs = bm.gibbs_ensemble(X, 4, K, sampler=sampler, chains=chains, burnin=burnin, seed=seed, **opts)
        for c, got in enumerate(outs):
            want = _single(sampler, X, 4, K, None, burnin, seed + c, None if z0s is None else z0s[c], **opts)
            _compare(got, want, "%s chain %d" % (sampler, c), True, True)


def test_three_hundred_chains_every_one_compared():
    X = synth(130, 5, 2, 1)[0]
    Xn = _new_rows(X, 65, 5)
    seed, chains = 5000, 300
    z0s = _starts(seed, chains, 2, 130)
    outs = bm.gibbs_ensemble(X, 4, 2, chains=chains, burnin=1, seed=seed, keep_trace=False, loo=True, newdata=Xn)
    assert bm.ensemble_plan("collapsed", 130, 5, 2, chains)["workgroups"] == 75
    for c, got in enumerate(outs):
        want = bm.gibbs_collapsed(X, 4, 2, beta=BETA, gamma=GAMMA, burnin=1, seed=seed + c, batch=1, initial_K=z0s[c], loo=True, newdata=Xn)
        _same_bytes(np.float64(got["loo"]["lpml"]), np.float64(want["loo"]["lpml"]), "chain %d lpml" % c)
        _same_bytes(got["predictive"]["lppd"], want["predictive"]["lppd"], "chain %d lppd" % c)
    pool = bm.ensemble_pool(outs)
    assert pool["loo"]["n_folded"] == 300 * 3 and pool["loo"]["lpml_chains"].shape == (300,) and pool["loo"]["lpml_sd"] > 0


@pytest.mark.parametrize("sampler,K,shape", [("collapsed", 3, "K3_P7"), ("dp", 12, "DP12_singleton")])
def test_an_independent_pin(sampler, K, shape):
    """ell and logdens recomputed from the returned z and alpha and a recount, by the NumPy restatements"""
    X = SHAPES[shape][1]()
    N = X.shape[0]
    Xn = _new_rows(X, 65, 11)
    seed = SINGLETON_SEED if shape == "DP12_singleton" else 41
    outs = bm.gibbs_ensemble(X, 6, K, sampler=sampler, chains=2, burnin=2, seed=seed, loo="trace", newdata=Xn, predictive_trace=True)
    terms = pref.collapsed_terms if sampler == "collapsed" else pref.dp_terms
    rows = range(0, N, 7)  # (recount_ell recounts the whole state per row)
    for c, o in enumerate(outs):
        for s in (0, 3):
            z, alpha = o["z"][s], float(o["alpha"][s, 0])
            want = lref.recount_ell(X, z, K, alpha, BETA, GAMMA, sampler, rows=rows)
            got = o["loo"]["ell"][s][list(rows)]
            print(shape, c, s, "largest relative difference of ell", np.max(np.abs(got - want) / np.abs(want)))
            np.testing.assert_allclose(got, want, rtol=RTOL)
            Nk, S = pref.counts_from_labels(X, z, K)
            want = pref.logdens(terms(Xn, Nk, S, alpha, N, BETA, GAMMA))
            got = o["predictive"]["logdens"][s]
            print(shape, c, s, "largest relative difference of logdens", np.max(np.abs(got - want) / np.abs(want)))
            np.testing.assert_allclose(got, want, rtol=RTOL)


@pytest.mark.parametrize("sampler,K", [("collapsed", 3), ("dp", 8)])
def test_the_densities_of_all_rows_sum_to_one(sampler, K):
    X = synth(150, 5, 3, 13)[0]
    outs = bm.gibbs_ensemble(X, 6, K, sampler=sampler, chains=3, burnin=1, seed=19, newdata=pref.all_rows(5), predictive_trace=True)
    for o in outs:
        ld = o["predictive"]["logdens"]
        assert ld.shape == (5, 32)
        assert np.max(np.abs(np.exp(ld).sum(axis=1) - 1.0)) < 1e-12  # tests/test_gpu_predict.py: over all 2^P rows


def test_nothing_leaks():
    """a fold changes nothing of the chains; chain c of five with folds is the same chain alone"""
    X = synth(200, 7, 3, 2)[0]
    Xn = _new_rows(X, 65, 3)
    for sampler, K in (("collapsed", 3), ("dp", 8)):
        seed = 900
        opts = dict(loo="trace", newdata=Xn, predictive_trace=True)
        plain = bm.gibbs_ensemble(X, 9, K, sampler=sampler, chains=5, burnin=0, seed=seed)
        five = bm.gibbs_ensemble(X, 9, K, sampler=sampler, chains=5, burnin=0, seed=seed, **opts)
        z0s = _starts(seed, 5, K, 200)
        for c in range(5):
            for key in ("z", "theta", "alpha", "sizes", "z_last"):
                _same_bytes(five[c][key], plain[c][key], "%s chain %d %s" % (sampler, c, key))
            alone = bm.gibbs_ensemble(X, 9, K, sampler=sampler, chains=1, burnin=0, seed=seed + c,
                                      initial_K=[z0s[c]] if sampler == "collapsed" else None, **opts)[0]
            _compare(five[c], alone, "%s chain %d alone" % (sampler, c), True, True)
