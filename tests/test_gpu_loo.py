"""The leave-one-out predictive of the fitted rows on the device (include/bmm_mcmc.h) against
tests/loo_ref.py, the NumPy restatement that tests/test_loo_ref.py pins to the recount, to the oracle's conditionals
and to exact enumeration.  The restatement is fed with the state read from the same chain (Chain.counts / labels /
alpha / params), so the two differ only in 1-ulp log / exp and the order of the sums: rtol 1e-12 on ell, the project's
figure for logdens."""
import math

import numpy as np
import pytest
from scipy.special import logsumexp

import bmm_mcmc_amd as bm
import loo_ref as lref
from test_gpu_predict import SHAPES
from util import load_dataset, synth

pytestmark = pytest.mark.gpu

RTOL = 1e-12
EPS = 2.0 ** -52


def _chain(sampler, X, K, seed=3, alpha=1.3, beta=0.5, gamma=0.5, batch=None, z0=None):
    N, P = X.shape
    c = bm.Chain(sampler, N, P, K, alpha=alpha, beta=beta, gamma=gamma, batch=batch, seed=seed)
    c.set_data(X)
    rng = np.random.default_rng(seed)
    if sampler == "collapsed":
        c.set_initial_labels(rng.integers(1, K + 1, N).astype(np.int32) if z0 is None else z0)
    elif sampler in ("stickbreaking", "full"):
        c.set_initial_params(rng.dirichlet(np.ones(K)), np.asfortranarray(0.05 + 0.9 * rng.random((K, P))))
    c.set_loo()
    return c


def _want(c, X, beta, gamma):
    """the restatement's ell from the state read off the chain"""
    if c.sampler in ("stickbreaking", "full"):
        pi, theta = c.params()
        return lref.explicit_ell(X, pi, theta)
    Nk, S = c.counts()
    return lref.counting_ell(X, c.labels(), Nk, S, c.alpha(), beta, gamma, c.sampler)


def _check_state(c, X, beta, gamma, tag):
    got = c.loo_state()
    want = _want(c, X, beta, gamma)
    print(tag, "largest relative difference of ell", np.max(np.abs(got - want) / np.abs(want)))
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got, want, rtol=RTOL)
    assert np.array_equal(c.loo_state(), got)
    return got


def _check_sweeps(c, X, beta, gamma, tag, steps=(1, 3)):
    """sweep 0 where the state is seated (the finite collapsed sampler), then after 1 and 4 sweeps"""
    if c.sampler == "collapsed":
        _check_state(c, X, beta, gamma, tag + " sweep 0")
    done = 0
    for n in steps:
        c.sweeps(n)
        done += n
        _check_state(c, X, beta, gamma, tag + " sweep %d" % done)


@pytest.mark.parametrize("sampler,K,P,beta,gamma,kt,gw", SHAPES)
def test_loo_state_equals_the_restatement(sampler, K, P, beta, gamma, kt, gw):
    X, _, _, _ = synth(3000, P, 3, seed=K + P)  # six workgroups of 512 rows, the last one partly filled
    with _chain(sampler, X, K, beta=beta, gamma=gamma) as c:
        _check_sweeps(c, X, beta, gamma, "%s K=%d P=%d" % (sampler, K, P))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1300])
@pytest.mark.parametrize("sampler,K,P", [("collapsed", 3, 5), ("dp", 6, 12), ("stickbreaking", 12, 40), ("collapsed", 3, 150)])
def test_every_number_of_fitted_rows(sampler, K, P, N):
    rng = np.random.default_rng(N + P)
    X = np.asfortranarray((rng.random((N, P)) < 0.1 + 0.8 * rng.random(P)).astype(np.int32))
    with _chain(sampler, X, K) as c:
        _check_sweeps(c, X, 0.5, 0.5, "%s N=%d" % (sampler, N), steps=(1, 1))


@pytest.mark.parametrize("sampler,K", [("collapsed", 5), ("dp", 9)])
def test_pending_deltas_and_several_batches_per_sweep(sampler, K):
    """batch 700 of 3000: five launches per sweep; before the first sweep the finite sampler's statistics are all
    pending deltas (k_count_labels), and k_state_tables reads them without folding them"""
    X, _, _, _ = synth(3000, 20, 3, seed=12)
    beta, gamma = (0.7, 0.4) if sampler == "collapsed" else (0.5, 0.5)  # (the DP sampler takes beta == gamma only)
    with _chain(sampler, X, K, batch=700, beta=beta, gamma=gamma) as c:
        assert c.batch == 700
        _check_sweeps(c, X, beta, gamma, "%s batch 700" % sampler)
        z, (Nk, S), a = c.labels(), c.counts(), c.alpha()
        c.loo_state()
        assert np.array_equal(c.labels(), z) and np.array_equal(c.counts()[0], Nk) and np.array_equal(c.counts()[1], S)
        assert c.alpha() == a


@pytest.mark.parametrize("sampler,K,P", [("collapsed", 3, 150), ("stickbreaking", 70, 10), ("dp", 70, 10)])
def test_loo_state_on_the_generic_path(sampler, K, P):
    """shapes k_resample_generic takes: P > 128, or more than 64 categories"""
    X, _, _, _ = synth(1500, P, 3, seed=9)
    with _chain(sampler, X, K) as c:
        _check_sweeps(c, X, 0.5, 0.5, "generic %s K=%d P=%d" % (sampler, K, P), steps=(1, 2))


def test_loo_state_with_the_own_label_tables_in_global_memory():
    """K = 24, P = 128: the plain tables and the minus-self tables do not fit in LDS together (the second tier of
    k_resample, tests/test_gpu_relabel.py), so the own-label score is gathered from global memory"""
    X, _, _, _ = synth(1200, 128, 3, seed=5)
    with _chain("collapsed", X, 24, beta=0.6, gamma=0.9) as c:
        _check_sweeps(c, X, 0.6, 0.9, "second tier")


# ---------------------------------------------------------------- edge cases, hand-built
def test_finite_states_with_singleton_and_empty_labels():
    """labels 3 and 6 of 7 hold one row each, 5 and 7 none from the start: removing a singleton's row empties its label,
    which keeps its prior weight, as an empty one does"""
    X, _, _, _ = synth(2000, 20, 3, seed=2)
    z0 = np.random.default_rng(0).choice([1, 2, 4], X.shape[0]).astype(np.int32)
    z0[0], z0[1] = 3, 6
    with _chain("collapsed", X, 7, z0=z0, beta=0.7, gamma=0.4) as c:
        c.sweeps(0)  # (starts the chain: the statistics of the initial labels are counted)
        Nk = c.counts()[0]
        assert Nk[2] == 1 and Nk[5] == 1 and Nk[4] == 0 and Nk[6] == 0
        ell = _check_state(c, X, 0.7, 0.4, "singletons and empty labels, sweep 0")
        T = lref.counting_terms(X, z0, Nk, c.counts()[1], c.alpha(), 0.7, 0.4, "collapsed")
        prior = np.log(c.alpha() / 7) - np.log(1999 + c.alpha()) + (X[0] * np.log(0.7) + (1 - X[0]) * np.log(0.4) - np.log(1.1)).sum()
        assert T[0, 2] == pytest.approx(prior, rel=RTOL) and ell[0] == pytest.approx(logsumexp(T[0]), rel=RTOL)
        for n in (1, 3):
            c.sweeps(n)
            assert np.all(c.counts()[0][[4, 6]] == 0)
            _check_state(c, X, 0.7, 0.4, "singletons and empty labels, %d more" % n)


def test_a_dp_state_in_which_several_rows_sit_alone():
    """40 rows under a fixed concentration of 8: the sequential scan leaves several rows in clusters of their own.  Such
    a row's own label is unused without it: it is scored by the other used labels and the new cluster."""
    rng = np.random.default_rng(21)
    X = np.asfortranarray((rng.random((40, 8)) < 0.5).astype(np.int32))
    with _chain("dp", X, 30, alpha=8.0, batch=1) as c:
        seen = 0
        for s in range(4):
            c.sweeps(1)
            Nk, S = c.counts()
            alone = np.flatnonzero(Nk[c.labels() - 1] == 1)
            seen = max(seen, alone.size)
            ell = _check_state(c, X, 0.5, 0.5, "dp, %d rows alone" % alone.size)
            T = lref.counting_terms(X, c.labels(), Nk, S, c.alpha(), 0.5, 0.5, "dp")
            for i in alone:
                assert np.isneginf(T[i, c.labels()[i] - 1]) and ell[i] == pytest.approx(logsumexp(T[i]), rel=RTOL)
        assert seen >= 2, seen


def test_a_dp_state_at_maxk():
    """three generating components and maxK = 3: the chain holds maxK - 1 clusters and one label that stays free
    (tests/test_gpu_predict.py)"""
    X, _, _, _ = synth(2000, 30, 3, seed=6)
    with _chain("dp", X, 3) as c:
        c.sweeps(5)
        assert (c.counts()[0] > 0).sum() == 2
        _check_state(c, X, 0.5, 0.5, "dp at maxK")


@pytest.mark.parametrize("K,P", [(2, 1), (3, 5), (3, 6), (4, 128)])
def test_partly_used_last_groups(K, P):
    """P = 5 and 128: the last group of three is partly used (5 = 3 + 2, 128 = 42 * 3 + 2); P = 6 and 128: the last group
    of five (6 = 5 + 1, 128 = 25 * 5 + 3); K = 2, P = 1: one feature in either"""
    X, _, _, _ = synth(700, P, 2, seed=P)
    for sampler in ("collapsed", "dp", "full"):
        beta, gamma = (0.5, 0.5) if sampler == "dp" else (0.6, 0.9)  # (the DP sampler takes beta == gamma only)
        with _chain(sampler, X, K, beta=beta, gamma=gamma) as c:
            _check_sweeps(c, X, beta, gamma, "%s K=%d P=%d" % (sampler, K, P), steps=(1, 1))


# ---------------------------------------------------------------- the fold
def _check_fold(sampler, trace, got, n, N):
    """the summary `got` of a fold over the n kept sweeps whose ell is `trace` (n x N), against the restatement's
    (tests/test_gpu_split_merge_routes.py holds a run with split-merge moves to the same)"""
    assert trace.shape == (n, N) and got["n_folded"] == n
    want = lref.summary(trace, waic=sampler in ("stickbreaking", "full"))
    R = np.max(np.abs(trace))
    for key in ("log_cpo", "lppd"):
        print(sampler, key, "largest difference", np.max(np.abs(got[key] - want[key])))
        assert np.max(np.abs(got[key] - want[key])) < 1e-12  # as lppd of the predictive: a few ulp of a value of a few tens
    np.testing.assert_allclose(got["ess"], want["ess"], rtol=1e-12)  # a ratio of two sums of n terms, each a few ulp
    assert np.all(got["ess"] >= 1.0 - 1e-12) and np.all(got["ess"] <= n + 1e-12)
    # Welford's mean: n updates, each rounding a value of at most R = max |ell| a few times
    assert np.max(np.abs(got["mean"] - want["mean"])) <= 8 * n * EPS * R
    # Welford's M2: n updates of delta * (ell - mean'), |each factor| <= 2 R, a handful of roundings each, on a sum of
    # at most n (2 R)^2; divided by n - 1.  Bound 64 n eps R^2 (NumPy's two-pass value is well inside it too).
    print(sampler, "var: largest difference", np.max(np.abs(got["var"] - want["var"])), "bound", 64 * n * EPS * R * R)
    assert np.max(np.abs(got["var"] - want["var"])) <= 64 * n * EPS * R * R
    # the scalars: 1024 partial sums of ceil(N / 1024) rows each, then a 10-level tree
    depth = -(-N // 1024) + 10
    for key, rows in (("lpml", got["log_cpo"]),):
        assert abs(got[key] - math.fsum(rows)) <= depth * EPS * math.fsum(np.abs(rows))
    assert got["min_ess"] == got["ess"].min()
    if sampler in ("stickbreaking", "full"):
        assert abs(got["p_waic"] - math.fsum(got["var"])) <= depth * EPS * math.fsum(np.abs(got["var"]))
        lp = math.fsum(got["lppd"])
        assert abs(got["elpd_waic"] - (lp - got["p_waic"])) <= depth * EPS * math.fsum(np.abs(got["lppd"])) + EPS * abs(lp)
    else:
        assert "p_waic" not in got and "elpd_waic" not in got


@pytest.mark.parametrize("sampler,K,n", [("collapsed", 5, 6), ("dp", 9, 8), ("stickbreaking", 6, 10), ("full", 4, 7)])
def test_the_fold(sampler, K, n):
    X, _, _, _ = synth(2500, 30, 3, seed=8)
    N = X.shape[0]

    def run():
        with _chain(sampler, X, K, alpha=None) as c:
            c.sweeps(2)
            trace = c.sweeps_loo(n, trace=True)
            return trace, c.loo()

    trace, got = run()
    _check_fold(sampler, trace, got, n, N)
    with _chain(sampler, X, K, alpha=None) as c:  # the same chain stepped by hand
        c.sweeps(2)
        for s in range(n):
            c.sweeps(1)
            assert np.array_equal(c.loo_state(), trace[s]), s
        with pytest.raises(bm.BmmError):
            c.loo()  # loo_state folds nothing
        c.sweeps_loo(2)
        c.loo_reset()
        c.sweeps_loo(3)
        assert c.loo()["n_folded"] == 3
    trace2, got2 = run()
    assert trace2.tobytes() == trace.tobytes()
    for key in got:
        assert np.asarray(got2[key]).tobytes() == np.asarray(got[key]).tobytes(), key


# ---------------------------------------------------------------- the wrappers
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
def test_loo_changes_nothing_of_the_chain(sampler, relabel):
    X = load_dataset("K3_N1000_P5")
    fit, Xnew = X[:800], X[800:]
    kw = dict(relabel=True, burnrelabel=3, stephens="device") if relabel else {}
    plain = _call(sampler, fit, 4, **kw)
    assert "loo" not in plain
    with_loo = _call(sampler, fit, 4, loo="trace", **kw)
    for key in plain:
        assert np.array_equal(plain[key], with_loo[key], equal_nan=True), key
    lo = with_loo["loo"]
    assert lo["ell"].shape == (8, 800) and lo["n_folded"] == 8
    assert ("p_waic" in lo) == (sampler in ("stickbreaking", "full"))
    want = lref.summary(lo["ell"])
    assert np.max(np.abs(lo["log_cpo"] - want["log_cpo"])) < 1e-12
    assert "ell" not in _call(sampler, fit, 4, loo=True, **kw)["loo"]
    both = _call(sampler, fit, 4, newdata=Xnew, partition="binder", **kw)
    everything = _call(sampler, fit, 4, newdata=Xnew, partition="binder", loo=True, **kw)
    for key in plain:
        assert np.array_equal(plain[key], everything[key], equal_nan=True), key
    assert np.array_equal(everything["predictive"]["lppd"], both["predictive"]["lppd"])
    assert everything["partition"]["best"] == both["partition"]["best"]
    for key in ("log_cpo", "ess", "lppd", "mean", "var"):
        assert np.array_equal(everything["loo"][key], lo[key]), key
    assert everything["loo"]["lpml"] == lo["lpml"]
    assert "loo" not in _call(sampler, fit, 4)  # the summary was disarmed when its run returned


@pytest.mark.parametrize("sampler", ["collapsed", "dp", "stickbreaking", "full"])
def test_one_call_equals_the_resident_chain(sampler):
    X = load_dataset("K3_N1000_P5")
    fit = np.asfortranarray(X[:800])
    K, ns, burnin = 4, 14, 6
    got = _call(sampler, fit, K, loo=True)["loo"]
    rng = np.random.default_rng(17)
    with bm.Chain(sampler, 800, 5, K, seed=21) as c:
        c.set_data(fit)
        if sampler == "collapsed":
            c.set_initial_labels(rng.integers(1, K + 1, 800).astype(np.int32))
        elif sampler != "dp":
            c.set_initial_params(np.ones(K) / K, np.asfortranarray(0.1 + 0.8 * rng.random((K, 5))))
        c.set_loo()
        c.sweeps(burnin - 1)           # sweeps j = 1 .. burnin - 1 are not kept
        c.sweeps_loo(ns - burnin)      # j = burnin .. nsamples - 1
        want = c.loo()
    assert want["n_folded"] == ns - burnin and set(got) == set(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), key


def test_without_burnin_the_starting_row_is_not_folded():
    X = load_dataset("K3_N1000_P5")
    out = bm.gibbs_dp(X, 6, burnin=0, maxK=5, seed=2, loo="trace")["loo"]
    assert out["n_folded"] == 5 and np.all(np.isnan(out["ell"][0])) and np.all(np.isfinite(out["ell"][1:]))
    assert np.max(np.abs(out["log_cpo"] - lref.summary(out["ell"][1:])["log_cpo"])) < 1e-12


def test_lpml_prefers_three_components_to_one():
    fit = load_dataset("K3_N1000_P5")[:800]
    z3 = np.random.default_rng(1).integers(1, 4, 800).astype(np.int32)
    l3 = bm.gibbs_collapsed(fit, 120, 3, alpha=1.0, burnin=20, seed=5, initial_K=z3, loo=True)["loo"]
    l1 = bm.gibbs_collapsed(fit, 120, 1, alpha=1.0, burnin=20, seed=5, initial_K=np.ones(800, dtype=np.int32), loo=True)["loo"]
    # one component: every state is the same, the product of the Beta-Bernoulli marginals of the other 799 rows
    s = fit.sum(axis=0).astype(np.float64) - fit
    marg = (fit * np.log(0.5 + s) + (1 - fit) * np.log(0.5 + 799 - s) - np.log(1.0 + 799)).sum(axis=1)
    np.testing.assert_allclose(l1["log_cpo"], marg, rtol=RTOL)
    np.testing.assert_allclose(l1["ess"], 100.0, rtol=RTOL)
    print("lpml of 800 fitted rows: K = 3", l3["lpml"], "K = 1", l1["lpml"], "margin", l3["lpml"] - l1["lpml"],
          "smallest ess of the K = 3 fit", l3["min_ess"], "of", l3["n_folded"])
    assert l3["lpml"] > l1["lpml"]


def test_refusals_leave_the_chain_usable():
    X, _, _, _ = synth(1000, 10, 3, seed=1)
    for sampler, K in (("dp", 6), ("stickbreaking", 4), ("full", 3)):
        with _chain(sampler, X, K) as c:
            with pytest.raises(bm.BmmError, match="first sweep") as e:
                c.loo_state()
            assert e.value.code == 5  # BMM_E_STATE
            c.sweeps(1)
            _check_state(c, X, 0.5, 0.5, "%s after the refusal" % sampler)
    with _chain("collapsed", X, 3) as c:
        c.set_loo(False)
        for call in (c.loo, c.loo_state, c.loo_reset, lambda: c.sweeps_loo(1)):
            with pytest.raises(bm.BmmError, match="not armed") as e:
                call()
            assert e.value.code == 5
        c.sweeps(1)
        c.set_loo()
        with pytest.raises(bm.BmmError, match="folded"):
            c.loo()
        c.sweeps_loo(2)
        assert c.loo()["n_folded"] == 2
    with bm.Chain("stickbreaking", 1000, 10, 4, seed=1) as c:
        c.set_data(X)
        c.set_shard(2000, 0)
        with pytest.raises(bm.BmmError, match="sharded"):
            c.set_loo()
    with pytest.raises(ValueError, match="chains"):
        bm.gibbs_collapsed(X, 6, 3, chains=2, loo=True)
    with pytest.raises(ValueError):
        bm.gibbs_collapsed(X, 6, 3, loo="everything")
    assert "loo" in bm.gibbs_collapsed(X, 6, 3, seed=1, loo=True)
