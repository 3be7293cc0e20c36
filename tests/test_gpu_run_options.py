"""What the options of a whole-run call compute, pinned bit for bit (chains are reproducible for a fixed seed): several
options armed for one call give the chain of the call without them and the summaries of a resident chain driven by
hand; an option is armed for exactly one call, whatever that call returns.

The shape: N = 257 is one full 256-row tile and a one-row tile, P = 33 two plane words with one live bit in the second."""
import ctypes as C

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi

pytestmark = pytest.mark.gpu

N, P, K, M, NS, SEED = 257, 33, 6, 5, 6, 11
LOO_ROWS = ("log_cpo", "ess", "lppd", "mean", "var")


def _data():
    rng = np.random.default_rng(5)
    theta = 0.1 + 0.8 * rng.random((3, P))
    rows = (rng.random((N + M, P)) < theta[rng.integers(0, 3, N + M)]).astype(np.int32)
    return np.asfortranarray(rows[:N]), np.asfortranarray(rows[N:])


X, XNEW = _data()
Z0 = np.random.default_rng(6).integers(1, K + 1, N).astype(np.int32)
PI0 = np.ones(K) / K
TH0 = np.asfortranarray(0.1 + 0.8 * np.random.default_rng(7).random((K, P)))


def _same(got, want, what):
    assert np.array_equal(got, want, equal_nan=True), what


def _resident(sampler, split_merge):
    c = bm.Chain(sampler, N, P, K, seed=SEED)
    c.set_data(X)
    if sampler == "full":
        c.set_initial_params(PI0, TH0)
    if split_merge:
        c.set_split_merge(split_merge)
    return c


def _check_against_resident(sampler, out, burnin, split_merge):
    """the predictive and the leave-one-out outputs of a run against two resident chains of the same seed"""
    S, first = NS - burnin, 1 if burnin == 0 else 0   # without burn-in row 0 is the starting state: NaN, not folded
    pr, lo = out["predictive"], out["loo"]
    assert pr["logdens"].shape == (S, M) and lo["ell"].shape == (S, N)
    if first:
        assert np.isnan(pr["logdens"][0]).all() and np.isnan(lo["ell"][0]).all()
    assert not np.isnan(pr["logdens"][first:]).any() and not np.isnan(lo["ell"][first:]).any()
    with _resident(sampler, split_merge) as c:
        c.set_newdata(XNEW)
        if burnin > 1:
            c.sweeps(burnin - 1)
        trace = c.sweeps_predict(S - first, trace=True)
        want = c.predictive()
    assert want["n"] == S - first
    _same(pr["logdens"][first:], trace, "log-density trace")
    _same(pr["lppd"], want["lppd"], "lppd")
    with _resident(sampler, split_merge) as c:
        c.set_loo(True)
        if burnin > 1:
            c.sweeps(burnin - 1)
        trace = c.sweeps_loo(S - first, trace=True)
        want = c.loo()
    assert lo["n_folded"] == want["n_folded"] == S - first
    _same(lo["ell"][first:], trace, "leave-one-out trace")
    for key in LOO_ROWS + ("lpml", "min_ess") + (("p_waic", "elpd_waic") if sampler == "full" else ()):
        _same(lo[key], want[key], key)


@pytest.mark.parametrize("burnin", [0, 2])
def test_options_together_on_the_dp_sampler(burnin):
    kw = dict(burnin=burnin, maxK=K, seed=SEED, split_merge=1)
    plain = bm.gibbs_dp(X, NS, **kw)
    out = bm.gibbs_dp(X, NS, newdata=XNEW, predictive_trace=True, loo="trace", partition="binder", **kw)
    for key in ("z", "theta", "alpha"):
        _same(out[key], plain[key], key)
    assert out["split_merge"] == plain["split_merge"]
    pt = out["partition"]
    assert pt["n_used"] == NS - burnin - (1 if burnin == 0 else 0)
    _same(pt["z"], out["z"][pt["best"]], "the partition's row of the trace")
    _check_against_resident("dp", out, burnin, 1)


@pytest.mark.parametrize("burnin", [0, 2])
def test_options_together_on_the_full_sampler(burnin):
    kw = dict(burnin=burnin, seed=SEED, initial_pi=PI0, initial_theta=TH0)
    plain = bm.gibbs_full(X, NS, K, **kw)
    out = bm.gibbs_full(X, NS, K, newdata=XNEW, predictive_trace=True, loo="trace", partition="binder", **kw)
    for key in ("z", "theta", "alpha", "pi"):
        _same(out[key], plain[key], key)
    pt = out["partition"]
    assert pt["n_used"] == NS - burnin - (1 if burnin == 0 else 0)
    _same(pt["z"], out["z"][pt["best"]], "the partition's row of the trace")
    _check_against_resident("full", out, burnin, 0)


@pytest.mark.parametrize("burnin", [0, 2])
def test_feature_selection_in_one_call_equals_the_resident_chain(burnin):
    f = bm.gibbs_collapsed(X, NS, K, alpha=1.0, burnin=burnin, seed=SEED, initial_K=Z0, select_features=True, rho=0.5)["features"]
    S, first = NS - burnin, 1 if burnin == 0 else 0
    with bm.Chain("collapsed", N, P, K, alpha=1.0, seed=SEED) as c:
        c.set_data(X)
        c.set_initial_labels(Z0)
        c.set_feature_select(True, 0.5)
        if burnin > 1:
            c.sweeps(burnin - 1)
            c.feature_reset()          # the steps of the sweeps that are not kept are not folded by a run
        trace = c.sweeps_features(S - first)
        want = c.feature_summary()
    assert f["gamma"].shape == (S, P)
    if first:
        assert f["gamma"][0].all()     # the initial mask
    _same(f["gamma"][first:], trace, "indicator trace")
    _same(f["n_selected"], f["gamma"].sum(axis=1), "n_selected")
    assert f["n_folded"] == want["n_folded"] == S - first
    _same(f["inclusion"], want["inclusion"], "inclusion")
    _same(f["inclusion_rb"], want["inclusion_rb"], "inclusion_rb")


@pytest.mark.parametrize("burnin", [0, 2])
def test_allocation_run_is_reproducible(burnin):
    z0 = np.random.default_rng(8).integers(1, 4, N).astype(np.int32)
    a, b = (bm.gibbs_allocation(X, NS, K, K0=3, burnin=burnin, seed=SEED, initial_K=z0) for _ in range(2))
    assert a["K"].shape == (NS - burnin,) and np.all((a["K"] >= 1) & (a["K"] <= K))
    _same(a["K"], b["K"], "K trace")
    assert a["moves"] == b["moves"]
    _same(a["z"], b["z"], "z")
    if burnin == 0:
        assert a["K"][0] == 3


# ---------------------------------------------------------------- armed for exactly one call
def _plain():
    return bm.gibbs_collapsed(X, NS, K, alpha=1.0, burnin=2, seed=SEED, initial_K=Z0)


def _armed():
    """the partition and the leave-one-out summary armed by hand, for a run of NS - 2 kept sweeps"""
    pt = bm._Partition("binder", 1, None, N, NS - 2)
    lo = bm._Loo(N, NS - 2)
    pt.arm()
    lo.arm()
    return pt, lo


def _untouched(pt, lo):
    return (pt.n_used.value == 0 and pt.best.value == -1 and np.isnan(pt.loss).all() and lo.n.value == 0
            and all(np.isnan(lo.rows[k]).all() for k in LOO_ROWS))


def _fail_on_burnin():
    z, th, al = np.zeros((1, N), dtype=np.int32), np.zeros((K, P, 1)), np.zeros(1)
    rc = _capi.lib().bmm_collapsed_run_probs(
        _capi.vp(X), C.c_int64(N), C.c_int(P), _capi.vp(Z0), C.c_int(NS), C.c_int(K), C.c_double(1.0), C.c_double(0.5),
        C.c_double(0.5), C.c_double(1.0), C.c_double(1.0), C.c_int(NS), C.c_int64(0), C.c_uint64(SEED), C.c_int(0),
        _capi.vp(z), _capi.vp(th), _capi.vp(al), None)
    assert rc == 1 and b"burnin must be in [0, nsamples)" in _capi.lib().bmm_last_error()


def _fail_on_create():
    with pytest.raises(bm.BmmError) as e:   # a DP chain with beta != gamma does not exist: refused once the run creates it
        bm.gibbs_dp(X, NS, burnin=2, maxK=K, seed=SEED, beta=0.5, gamma=0.7)
    assert e.value.code == 1


def _two_chains():
    outs = bm.gibbs_collapsed(X, NS, K, alpha=1.0, burnin=2, seed=SEED, chains=2)
    assert len(outs) == 2 and all("partition" not in o and "loo" not in o for o in outs)


def test_an_armed_summary_is_written_by_the_next_run():
    """(what the three tests below rely on to tell an armed run from one that is not)"""
    want = _plain()
    pt, lo = _armed()
    got = _plain()
    assert not _untouched(pt, lo)
    assert pt.n_used.value == NS - 2 and lo.n.value == NS - 2 and not np.isnan(lo.rows["log_cpo"]).any()
    for key in ("z", "theta", "alpha"):
        _same(got[key], want[key], key)
    again = _plain()                       # ... and by that run only
    for key in ("z", "theta", "alpha"):
        _same(again[key], want[key], key)


@pytest.mark.parametrize("call", [_fail_on_burnin, _fail_on_create, _two_chains])
def test_armed_for_exactly_one_call(call):
    want = _plain()
    pt, lo = _armed()
    call()
    assert _untouched(pt, lo)
    got = _plain()
    assert _untouched(pt, lo)
    assert "partition" not in got and "loo" not in got
    for key in ("z", "theta", "alpha"):
        _same(got[key], want[key], key)
