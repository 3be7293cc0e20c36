"""The posterior predictive density of new rows on the device (include/bmm_mcmc.h) against
tests/predictive_ref.py, the NumPy restatement that tests/test_predictive_ref.py pins to the oracle's conditionals
and to exact enumeration.  The restatement is fed with the state read from the same chain (Chain.counts / alpha /
params), so the two differ only in 1-ulp log / exp and the order of the sums: rtol 1e-12 on log p(x | state),
responsibilities summing to 1 within 1e-14."""
import ctypes as C

import numpy as np
import pytest
from scipy.special import logsumexp

import bmm_mcmc_amd as bm
import predictive_ref as pref
from bmm_mcmc_amd import _capi
from util import load_dataset, synth

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def _chain(sampler, X, K, seed=3, alpha=1.3, beta=0.5, gamma=0.5, batch=None, z0=None):
    N, P = X.shape
    c = bm.Chain(sampler, N, P, K, alpha=alpha, beta=beta, gamma=gamma, batch=batch, seed=seed)
    c.set_data(X)
    rng = np.random.default_rng(seed)
    if sampler == "collapsed":
        c.set_initial_labels(rng.integers(1, K + 1, N).astype(np.int32) if z0 is None else z0)
    elif sampler in ("stickbreaking", "full"):
        c.set_initial_params(rng.dirichlet(np.ones(K)), np.asfortranarray(0.05 + 0.9 * rng.random((K, P))))
    return c


def _want_terms(c, Xnew, beta, gamma):
    """the restatement's log category terms from the state read off the chain"""
    if c.sampler in ("stickbreaking", "full"):
        pi, theta = c.params()
        return pref.explicit_terms(Xnew, pi, theta)
    Nk, S = c.counts()
    fn = pref.collapsed_terms if c.sampler == "collapsed" else pref.dp_terms
    return fn(Xnew, Nk, S, c.alpha(), c.N, beta, gamma)


def _check_state(c, Xnew, beta, gamma, tag):
    ld, rp = c.predict_state(responsibilities=True)
    t = _want_terms(c, Xnew, beta, gamma)
    want = pref.logdens(t)
    print(tag, "largest relative difference of logdens", np.max(np.abs(ld - want) / np.abs(want)),
          "largest |sum resp - 1|", np.max(np.abs(rp.sum(axis=1) - 1.0)))
    np.testing.assert_allclose(ld, want, rtol=RTOL)
    assert np.array_equal(c.predict_state(), ld)
    assert rp.shape == (Xnew.shape[0], t.shape[1])
    assert np.max(np.abs(rp.sum(axis=1) - 1.0)) < 1e-14
    np.testing.assert_allclose(rp, pref.resp(t), rtol=0, atol=1e-11)


def _newrows(rng, M, P):
    return np.asfortranarray((rng.random((M, P)) < 0.1 + 0.8 * rng.random(P)).astype(np.int32))


# sampler, K (or maxK), P, beta, gamma, accumulators, group width
SHAPES = [
    ("collapsed", 3, 5, 0.7, 0.4, 4, 5),
    ("collapsed", 2, 1, 0.5, 0.5, 4, 5),
    ("collapsed", 20, 50, 0.5, 0.5, 20, 5),
    ("collapsed", 32, 100, 0.7, 0.4, 32, 4),
    ("collapsed", 64, 50, 0.5, 0.5, 64, 4),
    ("collapsed", 4, 128, 0.6, 0.9, 4, 5),
    ("dp", 19, 50, 0.5, 0.5, 20, 5),
    ("stickbreaking", 50, 50, 0.3, 1.1, 52, 5),
    ("full", 8, 100, 0.7, 0.4, 8, 5),
    ("full", 3, 5, 0.5, 0.5, 4, 5),
]


@pytest.mark.parametrize("sampler,K,P,beta,gamma,kt,gw", SHAPES)
def test_predict_state_equals_the_restatement(sampler, K, P, beta, gamma, kt, gw):
    code = _capi.SAMPLER_CODE[sampler]
    assert _capi.lib().bmm_spec_group_width_for(code, K, P) == gw
    assert kt >= (K + 1 if sampler == "dp" else K)
    X, _, _, _ = synth(3000, P, 3, seed=K + P)
    rng = np.random.default_rng(K * 1000 + P)
    Xnew = _newrows(rng, 1300, P)  # three workgroups of 512 rows, the last one partly filled
    with _chain(sampler, X, K, beta=beta, gamma=gamma) as c:
        c.set_newdata(Xnew)
        _check_state(c, Xnew, beta, gamma, "%s K=%d P=%d sweep 0" % (sampler, K, P))
        c.sweeps(1)
        _check_state(c, Xnew, beta, gamma, "%s K=%d P=%d sweep 1" % (sampler, K, P))
        c.sweeps(3)
        _check_state(c, Xnew, beta, gamma, "%s K=%d P=%d sweep 4" % (sampler, K, P))


@pytest.mark.parametrize("sampler,K,P", [("collapsed", 3, 150), ("stickbreaking", 70, 10), ("dp", 70, 10)])
def test_predict_state_on_the_generic_path(sampler, K, P):
    """shapes k_resample_generic takes: P > 128, or more than 64 categories"""
    X, _, _, _ = synth(1500, P, 3, seed=9)
    rng = np.random.default_rng(K + P)
    Xnew = _newrows(rng, 777, P)
    with _chain(sampler, X, K) as c:
        c.set_newdata(Xnew)
        for n in (0, 1, 2):
            c.sweeps(n)
            _check_state(c, Xnew, 0.5, 0.5, "generic %s K=%d P=%d after %d more" % (sampler, K, P, n))


@pytest.mark.parametrize("M", [1, 63, 64, 65, 1300])
@pytest.mark.parametrize("sampler,K,P", [("collapsed", 3, 5), ("stickbreaking", 12, 40), ("collapsed", 3, 150)])
def test_every_number_of_new_rows(sampler, K, P, M):
    X, _, _, _ = synth(1000, P, 3, seed=4)
    Xnew = _newrows(np.random.default_rng(M), M, P)
    with _chain(sampler, X, K) as c:
        c.set_newdata(Xnew)
        c.sweeps(2)
        _check_state(c, Xnew, 0.5, 0.5, "%s M=%d" % (sampler, M))


def test_a_state_with_empty_labels():
    """labels 3, 5 and 6 of 6 start empty and stay so (the finite sampler never refills a label): the predictive
    keeps their prior weight"""
    X, _, _, _ = synth(2000, 20, 3, seed=2)
    z0 = np.random.default_rng(0).choice([1, 2, 4], X.shape[0]).astype(np.int32)
    Xnew = _newrows(np.random.default_rng(1), 300, 20)
    with _chain("collapsed", X, 6, z0=z0, beta=0.7, gamma=0.4) as c:
        c.set_newdata(Xnew)
        for n in (0, 1, 3):
            c.sweeps(n)
            assert np.all(c.counts()[0][[2, 4, 5]] == 0)
            _check_state(c, Xnew, 0.7, 0.4, "empty labels, %d more" % n)


def test_a_dp_state_at_maxk():
    """The DP sampler opens a label only while fewer than maxK - 1 are in use (k_resample: Kused < K - 1), so a chain
    "at maxK" holds maxK - 1 clusters and one label that stays free: three generating components and maxK = 3."""
    X, _, _, _ = synth(2000, 30, 3, seed=6)
    Xnew = _newrows(np.random.default_rng(3), 300, 30)
    with _chain("dp", X, 3) as c:
        c.set_newdata(Xnew)
        c.sweeps(5)
        assert (c.counts()[0] > 0).sum() == 2
        _check_state(c, Xnew, 0.5, 0.5, "dp at maxK")


def test_the_dp_predictive_is_a_density_on_the_device():
    X = load_dataset("K3_N1000_P5")
    Xnew = pref.all_rows(5)
    with _chain("dp", X, 6) as c:
        c.set_newdata(Xnew)
        # (before the first sweep nobody is seated: the N fitted observations carry no weight yet, only the new cluster's)
        _check_state(c, Xnew, 0.5, 0.5, "dp before the first sweep (new cluster only)")
        c.sweeps(5)
        _check_state(c, Xnew, 0.5, 0.5, "dp after five sweeps")
        assert abs(np.exp(c.predict_state()).sum() - 1.0) < 1e-12  # over all 2^P rows


def _check_fold_lppd(sampler, trace, lppd, n, M):
    """lppd of a fold over the n kept sweeps whose log densities are `trace` (n x M)
    (tests/test_gpu_split_merge_routes.py holds a run with split-merge moves to the same)"""
    assert trace.shape == (n, M) and lppd.shape == (M,)
    want = logsumexp(trace, axis=0) - np.log(n)
    print(sampler, "largest |lppd - logsumexp(trace) + log n|", np.max(np.abs(lppd - want)))
    assert np.max(np.abs(lppd - want)) < 1e-12


@pytest.mark.parametrize("sampler,K", [("collapsed", 5), ("dp", 9), ("stickbreaking", 6), ("full", 4)])
def test_the_fold(sampler, K):
    X, _, _, _ = synth(4000, 30, 3, seed=8)
    Xnew = _newrows(np.random.default_rng(5), 700, 30)
    n = 7

    def run():
        with _chain(sampler, X, K, alpha=None) as c:
            c.set_newdata(Xnew, responsibilities=True)
            c.sweeps(2)
            trace = c.sweeps_predict(n, trace=True)
            return trace, c.predictive(responsibilities=True)

    trace, pr = run()
    assert pr["n"] == n
    _check_fold_lppd(sampler, trace, pr["lppd"], n, 700)
    assert np.max(np.abs(pr["resp"].sum(axis=1) - 1.0)) < 1e-13  # a mean of n rows that each sum to 1 within 1e-14
    with _chain(sampler, X, K, alpha=None) as c:  # the same chain stepped by hand
        c.set_newdata(Xnew)
        c.sweeps(2)
        for s in range(n):
            c.sweeps(1)
            assert np.array_equal(c.predict_state(), trace[s]), s
        with pytest.raises(bm.BmmError):
            c.predictive()  # predict_state folds nothing
        c.sweeps_predict(2)
        c.predict_reset()
        c.sweeps_predict(3)
        assert c.predictive()["n"] == 3
    trace2, pr2 = run()
    assert np.array_equal(trace2, trace)
    assert np.array_equal(pr2["lppd"], pr["lppd"]) and np.array_equal(pr2["resp"], pr["resp"])


def _call(sampler, X, K, **kw):
    rng = np.random.default_rng(17)
    if sampler == "collapsed":
        return bm.gibbs_collapsed(X, 14, K, burnin=6, seed=21, initial_K=rng.integers(1, K + 1, X.shape[0]).astype(np.int32), **kw)
    if sampler == "dp":
        return bm.gibbs_dp(X, 14, burnin=6, maxK=K, seed=21, **kw)
    fn = bm.gibbs_stickbreaking if sampler == "stickbreaking" else bm.gibbs_full
    return fn(X, 14, K, burnin=6, seed=21, initial_pi=np.ones(K) / K,
              initial_theta=np.asfortranarray(0.1 + 0.8 * rng.random((K, X.shape[1]))), **kw)


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("sampler", ["collapsed", "dp", "stickbreaking", "full"])
def test_newdata_changes_nothing_of_the_chain(sampler, relabel):
    X = load_dataset("K3_N1000_P5")
    fit, Xnew = X[:800], X[800:]
    kw = dict(relabel=True, burnrelabel=3, stephens="device") if relabel else {}
    plain = _call(sampler, fit, 4, **kw)
    assert "predictive" not in plain
    with_new = _call(sampler, fit, 4, newdata=Xnew, predictive_trace=True, responsibilities=True, **kw)
    for key in plain:
        assert np.array_equal(plain[key], with_new[key], equal_nan=True), key
    pr = with_new["predictive"]
    assert pr["lppd"].shape == (200,) and pr["logdens"].shape == (8, 200)
    assert pr["resp"].shape == (200, 5 if sampler == "dp" else 4)
    assert np.max(np.abs(pr["lppd"] - (logsumexp(pr["logdens"], axis=0) - np.log(8)))) < 1e-12
    assert set(_call(sampler, fit, 4, newdata=Xnew, **kw)["predictive"]) == {"lppd"}


@pytest.mark.parametrize("sampler", ["collapsed", "dp", "stickbreaking", "full"])
def test_one_call_equals_the_resident_chain(sampler):
    X = load_dataset("K3_N1000_P5")
    fit, Xnew = np.asfortranarray(X[:800]), np.asfortranarray(X[800:])
    K, ns, burnin = 4, 14, 6
    got = _call(sampler, fit, K, newdata=Xnew)["predictive"]["lppd"]
    rng = np.random.default_rng(17)
    with bm.Chain(sampler, 800, 5, K, seed=21) as c:
        c.set_data(fit)
        if sampler == "collapsed":
            c.set_initial_labels(rng.integers(1, K + 1, 800).astype(np.int32))
        elif sampler != "dp":
            c.set_initial_params(np.ones(K) / K, np.asfortranarray(0.1 + 0.8 * rng.random((K, 5))))
        c.set_newdata(Xnew)
        c.sweeps(burnin - 1)               # sweeps j = 1 .. burnin - 1 are not kept
        c.sweeps_predict(ns - burnin)      # j = burnin .. nsamples - 1
        want = c.predictive()
    assert want["n"] == ns - burnin
    assert np.array_equal(got, want["lppd"])


def test_held_out_rows_prefer_three_components_to_one():
    X = load_dataset("K3_N1000_P5")
    fit, Xnew = X[:800], X[800:]
    z3 = np.random.default_rng(1).integers(1, 4, 800).astype(np.int32)
    l3 = bm.gibbs_collapsed(fit, 120, 3, alpha=1.0, burnin=20, seed=5, initial_K=z3, newdata=Xnew)["predictive"]["lppd"]
    l1 = bm.gibbs_collapsed(fit, 120, 1, alpha=1.0, burnin=20, seed=5, initial_K=np.ones(800, dtype=np.int32),
                            newdata=Xnew)["predictive"]["lppd"]
    # one component: every state is the same, the product of the Beta-Bernoulli marginals
    s = fit.sum(axis=0).astype(np.float64)
    marg = (Xnew * np.log(0.5 + s) + (1 - Xnew) * np.log(0.5 + 800 - s) - np.log(1.0 + 800)).sum(axis=1)
    np.testing.assert_allclose(l1, marg, rtol=RTOL)
    print("mean lppd of 200 held-out rows: K = 3", l3.mean(), "K = 1", l1.mean())
    assert l3.mean() > l1.mean()


def test_refusals_leave_the_chain_usable():
    X, _, _, _ = synth(1000, 10, 3, seed=1)
    good = _newrows(np.random.default_rng(2), 100, 10)
    bad = good.copy()
    bad[17, 3] = 2
    with _chain("collapsed", X, 3) as c:
        c.set_newdata(good)
        c.sweeps(1)
        before = c.predict_state()
        with pytest.raises(bm.BmmError, match="binary"):
            c.set_newdata(bad)
        with pytest.raises(bm.BmmError):
            _capi.check(_capi.lib().bmm_chain_set_newdata_host(c._h, _capi.vp(good), C.c_int64(-1)))
        with pytest.raises(bm.BmmError):
            _capi.check(_capi.lib().bmm_chain_set_newdata_host(c._h, None, C.c_int64(5)))
        assert np.array_equal(c.predict_state(), before)  # the earlier set is still there
        c.sweeps_predict(2)
        assert c.predictive()["n"] == 2
        c.set_newdata(None)
        with pytest.raises(bm.BmmError):
            c.predict_state()
        c.sweeps(1)
    with _chain("stickbreaking", X, 4) as c:
        c.set_shard(2000, 0)
        with pytest.raises(bm.BmmError, match="sharded"):
            c.set_newdata(good)
    with pytest.raises(NotImplementedError):
        bm.gibbs_collapsed(X, 6, 3, chains=2, newdata=good)
    with pytest.raises(bm.BmmError, match="binary"):
        bm.gibbs_collapsed(X, 6, 3, seed=1, newdata=bad)
    assert "predictive" in bm.gibbs_collapsed(X, 6, 3, seed=1, newdata=good)
