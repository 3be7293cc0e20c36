"""Folds on ensemble chains (include/bmm_mcmc.h): what needs no device -- bm.ensemble_pool against
one summary over the concatenated states, bmm_ensemble_fold_plan against hand-derived values, bmm_ensemble_run_ex with a
null struct refused and accepted exactly where bmm_ensemble_run is, the refusals of the struct, the wrapper's refusals
ahead of the library, and the public names."""
import ctypes as C

import numpy as np
import pytest

import bmm_mcmc_amd as bm
import loo_ref as lref
import predictive_ref as pref
import test_ensemble_cpu as base
from bmm_mcmc_amd import _capi

E_ARG, E_UNSUPPORTED = 1, 2


# ---------------------------------------------------------------- the pool
def _traces(seed, lengths, N):
    rng = np.random.default_rng(seed)
    centre = -1.0 - 4.0 * rng.random(N)
    return [centre + 0.8 * rng.standard_normal((n, N)) for n in lengths]


def test_the_pooled_loo_summary_is_the_summary_of_the_concatenated_states():
    tr = _traces(1, (7, 12, 3, 20), 40)
    outs = [{"loo": lref.summary(t)} for t in tr]
    want = lref.summary(np.concatenate(tr))
    got = bm.ensemble_pool(outs)["loo"]
    for key in ("log_cpo", "lppd"):
        assert np.max(np.abs(got[key] - want[key])) < 1e-12, key
    np.testing.assert_allclose(got["ess"], want["ess"], rtol=1e-12)
    np.testing.assert_allclose(got["lpml"], want["lpml"], rtol=1e-12)
    np.testing.assert_allclose(got["min_ess"], want["min_ess"], rtol=1e-12)
    assert got["n_folded"] == 42 and isinstance(got["n_folded"], int)
    # the per-chain LPMLs and their spread, by hand
    lp = [float((np.log(t.shape[0]) - np.log(np.exp(-t).sum(axis=0))).sum()) for t in tr]
    np.testing.assert_allclose(got["lpml_chains"], lp, rtol=1e-12)
    mean = sum(lp) / 4
    sd = (sum((v - mean) ** 2 for v in lp) / 3) ** 0.5
    assert abs(got["lpml_sd"] - sd) <= 1e-12 * sd
    assert set(got) == {"log_cpo", "ess", "lppd", "lpml", "min_ess", "n_folded", "lpml_chains", "lpml_sd"}


def test_the_pooled_predictive_is_the_lppd_of_the_concatenated_states():
    tr = _traces(2, (5, 9, 2), 17)
    outs = [{"predictive": {"lppd": pref.lppd(t), "n_folded": t.shape[0]}} for t in tr]
    got = bm.ensemble_pool(outs)
    assert set(got) == {"predictive"} and set(got["predictive"]) == {"lppd", "n_folded", "lppd_chains"}
    got = got["predictive"]
    assert np.max(np.abs(got["lppd"] - pref.lppd(np.concatenate(tr)))) < 1e-12
    assert got["n_folded"] == 16
    by_hand = [float(sum(np.log(np.exp(t[:, m]).sum() / t.shape[0]) for m in range(17))) for t in tr]
    np.testing.assert_allclose(got["lppd_chains"], by_hand, rtol=1e-12)


def test_the_pool_refuses_what_it_cannot_pool():
    with pytest.raises(ValueError, match="no chain"):
        bm.ensemble_pool([])
    with pytest.raises(ValueError, match="neither"):
        bm.ensemble_pool([{"z": None}])
    s = lref.summary(_traces(3, (4,), 5)[0])
    with pytest.raises(ValueError, match="folded no state"):
        bm.ensemble_pool([{"loo": s}, {"loo": dict(s, n_folded=0)}])


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize("sampler,N,P,K,chains,M,loo,want", [
    # K = 2, P = 5: the sweep's slice, 2416 bytes, four chains a workgroup.  loo: 5 chains * (12 * 130 + 8) doubles = 62720;
    # 65 new rows: 5 * 3 * 65 doubles = 7800 and one plane word a row = 260
    ("collapsed", 130, 5, 2, 5, 65, True, (2416, 4, 62720 + 7800 + 260, 5 * 130 * 8, 5 * 65 * 8, 2)),
    # DP, maxK = 63, P = 12: 29648 bytes; loo alone: 300 * (12 * 2000 + 8) * 8
    ("dp", 2000, 12, 63, 300, 0, True, (29648, 4, 300 * 24008 * 8, 300 * 2000 * 8, 0, 1)),
    # K = 20, P = 112: 82688 bytes, one chain a workgroup; 200 new rows alone: 7 * 600 doubles and 4 plane words a row
    ("collapsed", 4100, 112, 20, 7, 200, False, (82688, 1, 7 * 600 * 8 + 4 * 200 * 4, 0, 7 * 200 * 8, 1)),
])
def test_fold_plan_against_hand_derived_values(sampler, N, P, K, chains, M, loo, want):
    p = bm.ensemble_fold_plan(sampler, N, P, K, chains, M=M, loo=loo)
    keys = ("lds_bytes_per_chain", "chains_per_workgroup", "accumulator_bytes", "ell_bytes_per_kept_sweep",
            "logdens_bytes_per_kept_sweep", "launches_per_kept_sweep")
    assert tuple(p[k] for k in keys) == want
    assert p["lds_bytes_per_chain"] == bm.ensemble_plan(sampler, N, P, K, chains)["lds_bytes_per_chain"]


def test_fold_plan_refuses_as_the_plan_does():
    out = np.zeros(6, dtype=np.int64)
    L = _capi.lib()
    for sampler, N, P, K, chains, code, word in base.CASES:
        rc = L.bmm_ensemble_fold_plan(C.c_int(sampler), C.c_int64(N), C.c_int(P), C.c_int(K), C.c_int(chains), C.c_int64(0), C.c_int(1), _capi.vp(out))
        base._refused(rc, code, word)
    base._refused(L.bmm_ensemble_fold_plan(C.c_int(0), C.c_int64(100), C.c_int(5), C.c_int(3), C.c_int(4), C.c_int64(-1), C.c_int(0), _capi.vp(out)),
                  E_ARG, "M must be >= 0")
    assert L.bmm_ensemble_fold_plan(C.c_int(0), C.c_int64(100), C.c_int(5), C.c_int(3), C.c_int(4), C.c_int64(0), C.c_int(0), _capi.vp(out)) == 0
    assert out[2] == 0 and out[5] == 0  # nothing asked: nothing added


# ---------------------------------------------------------------- bmm_ensemble_run_ex
def _run_ex(sampler, N, P, K, chains, folds=None, beta=0.5, gamma=0.5, z0=None, nsamples=5):
    """bmm_ensemble_run_ex on a zero matrix with every buffer in place (tests/test_ensemble_cpu.py's _run)"""
    X = np.zeros((N, P), dtype=np.int32, order="F")
    S = nsamples - 1
    n = max(chains, 1)
    if z0 is None and sampler == 0:
        z0 = [np.ones(N, dtype=np.int32) for _ in range(n)]
    z = [np.zeros((S, N), dtype=np.int32, order="F") for _ in range(n)]
    nk = [np.zeros((S, K), dtype=np.int32) for _ in range(n)]
    th = [np.zeros((K, P, S), order="F") for _ in range(n)]
    al = [np.zeros(S) for _ in range(n)]
    zl = [np.zeros(N, dtype=np.int32) for _ in range(n)]
    keep = (X, z0, z, nk, th, al, zl)
    rc = _capi.lib().bmm_ensemble_run_ex(
        C.c_int(sampler), _capi.vp(X), C.c_int64(N), C.c_int(P), C.c_int(chains), bm._ptr_table(z0) if z0 is not None else None,
        C.c_int(nsamples), C.c_int(K), C.c_double(1.0), C.c_double(beta), C.c_double(gamma), C.c_double(1), C.c_double(1), C.c_int(1),
        C.c_uint64(1), C.c_int(0), bm._ptr_table(z), bm._ptr_table(nk), bm._ptr_table(th), bm._ptr_table(al), bm._ptr_table(zl),
        C.byref(folds) if folds is not None else None)
    del keep
    return rc


@pytest.mark.parametrize("sampler,N,P,K,chains,code,word", base.CASES)
def test_a_null_struct_is_refused_where_the_run_is(sampler, N, P, K, chains, code, word):
    base._refused(_run_ex(sampler, N, P, K, chains), code, word)
    base._refused(base._run(sampler, N, P, K, chains), code, word)


def test_a_null_struct_refuses_bad_arguments_as_the_run_does():
    base._refused(_run_ex(1, 50, 5, 6, 2, beta=0.5, gamma=0.7), E_ARG, "non-symmetric priors")
    base._refused(_run_ex(0, 50, 5, 3, 2, z0=[np.ones(50, dtype=np.int32), np.full(50, 4, dtype=np.int32)]), E_ARG, "initialK out of range: chain 1")
    base._refused(_run_ex(0, 50, 5, 3, 2, nsamples=1), E_ARG, "burnin must be in [0, nsamples)")
    base._refused(_run_ex(0, 50, 5, 3, 2, beta=0.0), E_ARG, "beta and gamma must be > 0")


def test_a_null_struct_is_accepted_where_the_run_is():
    """a shape the library takes gets past every refusal of both entries alike: the next word is the device's or none"""
    have_gpu = _capi.device_count() > 0
    for run in (base._run, _run_ex):
        rc = run(0, 50, 5, 3, 2)
        msg = _capi.lib().bmm_last_error().decode()
        if have_gpu:
            assert rc == 0, msg
        else:
            assert rc not in (0, E_ARG, E_UNSUPPORTED), (rc, msg)  # past the checks that need no device


def test_an_armed_run_option_is_still_refused_and_disarmed():
    L = _capi.lib()
    lv = np.array([1] * 5, dtype=np.int32)
    assert L.bmm_set_categorical(_capi.vp(lv), C.c_int(lv.size)) == 0
    base._refused(_run_ex(0, 50, 5, 3, 2), E_UNSUPPORTED, "no run option is offered")
    assert L.bmm_set_split_merge(C.c_int(1), C.c_int(2)) == 0
    base._refused(_run_ex(1, 50, 5, 6, 2, folds=bm._EnsembleFolds()), E_UNSUPPORTED, "no run option is offered")
    # nothing stays armed: the next refusal is the next call's own
    base._refused(_run_ex(0, 50, 5, 65, 2), E_UNSUPPORTED, "65 categories exceed 64")


def test_the_struct_is_checked_before_a_device_is_touched():
    chains, N, P, M = 2, 50, 5, 3
    Xn = np.zeros((M, P), dtype=np.int32, order="F")
    lppd = [np.zeros(M) for _ in range(chains)]
    tab = bm._ptr_table(lppd)
    f = bm._EnsembleFolds()
    f.newdata, f.M, f.pred_lppd = Xn.ctypes.data, M, C.cast(tab, C.c_void_p)
    Xn[1, 3] = 2  # a cell outside {0, 1}
    base._refused(_run_ex(0, N, P, 3, chains, folds=f), E_ARG, "newdata must be binary")
    Xn[1, 3] = -1
    base._refused(_run_ex(0, N, P, 3, chains, folds=f), E_ARG, "newdata must be binary")
    Xn[1, 3] = 1
    f.M = -1
    base._refused(_run_ex(0, N, P, 3, chains, folds=f), E_ARG, "M must be >= 0")
    f.M, f.newdata = M, None
    base._refused(_run_ex(0, N, P, 3, chains, folds=f), E_ARG, "Xnew is null")
    f.newdata, f.pred_lppd = Xn.ctypes.data, None
    base._refused(_run_ex(0, N, P, 3, chains, folds=f), E_ARG, "null buffer: pred_lppd")
    f.pred_lppd, f.predictive_trace = C.cast(tab, C.c_void_p), 1
    base._refused(_run_ex(0, N, P, 3, chains, folds=f), E_ARG, "null buffer: pred_logdens")
    g = bm._EnsembleFolds()
    g.loo = 1
    base._refused(_run_ex(0, N, P, 3, chains, folds=g), E_ARG, "null buffer: loo_log_cpo")
    # the shape's refusal comes first, as without the struct
    base._refused(_run_ex(0, N, P, 65, chains, folds=g), E_UNSUPPORTED, "65 categories exceed 64")


# ---------------------------------------------------------------- the wrapper refuses before the library is asked
def test_the_wrapper_refuses_before_the_run_is_asked(monkeypatch):
    def never(*args):
        raise AssertionError("the library's run was asked")

    monkeypatch.setattr(bm, "_ensemble_run", never)
    monkeypatch.setattr(bm, "_ensemble_run_ex", never)
    X = np.zeros((40, 5), dtype=np.int32)
    with pytest.raises(ValueError, match='loo must be True, "trace" or False'):
        bm.gibbs_ensemble(X, 5, 3, loo="tracee")
    with pytest.raises(ValueError, match="the 5 columns of data"):
        bm.gibbs_ensemble(X, 5, 3, newdata=np.zeros((4, 6), dtype=np.int32))
    with pytest.raises(ValueError, match="newdata has no rows"):
        bm.gibbs_ensemble(X, 5, 3, newdata=np.zeros((0, 5), dtype=np.int32), predictive_trace=True)
    with pytest.raises(ValueError, match="predictive_trace needs newdata"):
        bm.gibbs_ensemble(X, 5, 3, predictive_trace=True)
    with pytest.raises(bm.BmmError, match="65 categories exceed 64"):
        bm.gibbs_ensemble(X, 5, 65, loo=True)


def test_a_call_without_folds_goes_through_the_old_entry(monkeypatch):
    asked = []
    monkeypatch.setattr(bm, "_ensemble_run", lambda *a: asked.append(len(a)) or 0)
    monkeypatch.setattr(bm, "_ensemble_run_ex", lambda *a: (_ for _ in ()).throw(AssertionError("the new entry was asked")))
    outs = bm.gibbs_ensemble(np.zeros((40, 5), dtype=np.int32), 5, 3, chains=2, seed=1)
    assert asked == [21] and len(outs) == 2 and "loo" not in outs[0] and "predictive" not in outs[0]


def test_the_new_names_are_public():
    for name in ("ensemble_pool", "ensemble_fold_plan"):
        assert name in bm.__all__ and callable(getattr(bm, name))
    for sym in ("bmm_ensemble_fold_plan", "bmm_ensemble_run_ex"):
        assert sym in _capi.SYMBOLS and hasattr(_capi.lib(), sym)
