"""Incomplete new rows on the device (include/bmm_mcmc.h "incomplete new rows") against
tests/predictive_na_ref.py, the NumPy restatement that tests/test_predictive_na_ref.py pins to predictive_ref's
complete-row densities summed over all completions and to exact enumeration.  The restatement is fed with the state
read from the same chain (Chain.counts / alpha / params), so the two differ only in 1-ulp log / exp and the order of the
sums.  Tolerances, the project's own: rtol 1e-12 on log p(x_O | state) and on the log of each cell's joint (atol 1e-12
where the value is 0: the row with every cell missing); atol 1e-11 on the responsibilities, cell_state and cell_mean;
responsibilities summing to 1 within 1e-14."""
import ctypes as C

import numpy as np
import pytest

import bmm_mcmc_amd as bm
import predictive_na_ref as nref
import predictive_ref as pref
from bmm_mcmc_amd import _capi
from test_gpu_predict import _call, _chain, _newrows
from util import load_dataset, synth

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def _parts(c, beta, gamma):
    """the restatement's weights and Bernoulli terms from the state read off the chain"""
    if c.sampler in ("stickbreaking", "full"):
        return nref.explicit_parts(*c.params())
    Nk, S = c.counts()
    fn = nref.collapsed_parts if c.sampler == "collapsed" else nref.dp_parts
    return fn(Nk, S, c.alpha(), c.N, beta, gamma)


def _close_logs(got, want, zero, what):
    """rtol 1e-12, atol 1e-12 where the value is 0 (`zero` marks those entries)"""
    zero = np.broadcast_to(zero, got.shape)
    rel = np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])
    print(what, "largest relative difference", rel.max() if rel.size else 0.0,
          "largest |difference| where the value is 0", np.abs(got[zero] - want[zero]).max() if zero.any() else 0.0)
    np.testing.assert_allclose(got[~zero], want[~zero], rtol=RTOL, atol=0)
    np.testing.assert_allclose(got[zero], want[zero], rtol=0, atol=1e-12)


def _check_state(c, Xnew, miss, beta, gamma, tag):
    rows, cols = nref.cells_of(miss)
    ld, rp, cl = c.predict_state(responsibilities=True, cells=True)
    want_ld, want_rp, want_lj, want_cl = nref.state(Xnew, miss, _parts(c, beta, gamma))
    allmiss = miss.all(axis=1)
    _close_logs(ld, want_ld, allmiss, tag + " logdens")
    _close_logs(np.log(cl) + ld[rows], want_lj, np.zeros(rows.size, dtype=bool), tag + " log joint of the cells")
    assert np.array_equal(c.predict_state(), ld)
    assert rp.shape == want_rp.shape and cl.shape == (rows.size,)
    assert np.max(np.abs(rp.sum(axis=1) - 1.0)) < 1e-14
    np.testing.assert_allclose(rp, want_rp, rtol=0, atol=1e-11)
    np.testing.assert_allclose(cl, want_cl, rtol=0, atol=1e-11)
    return ld, cl


def _incomplete(rng, M, P, frac):
    Xnew = _newrows(rng, M, P)
    miss = nref.case_mask(rng, M, P, frac)
    Xna = Xnew.astype(np.float64)
    Xna[miss] = np.nan
    return Xnew, miss, Xna


# ---------------------------------------------------------------- 1. predict_state against the restatement
@pytest.mark.parametrize("sampler,K,P,beta,gamma,M,frac", nref.CASES)
def test_predict_state_with_cells_equals_the_restatement(sampler, K, P, beta, gamma, M, frac):
    X, _, _, _ = synth(3000, P, 3, seed=K + P)
    Xnew, miss, Xna = _incomplete(np.random.default_rng(K * 1000 + P + M), M, P, frac)
    tag = "%s K=%d P=%d M=%d %s" % (sampler, K, P, M, bm.predict_na_plan(sampler, K, P)["form"])
    with _chain(sampler, X, K, beta=beta, gamma=gamma) as c:
        c.set_newdata(Xna, missing="na")
        _check_state(c, Xnew, miss, beta, gamma, tag + " sweep 0")
        c.sweeps(1)
        _check_state(c, Xnew, miss, beta, gamma, tag + " sweep 1")
        c.sweeps(3)
        ld, cl = _check_state(c, Xnew, miss, beta, gamma, tag + " sweep 4")
        # the mask as a boolean matrix over arbitrary values, and as a cell list: the same bits
        junk = np.where(miss, 1 - Xnew, Xnew)
        c.set_newdata(junk, missing=miss)
        ld2, cl2 = c.predict_state(cells=True)
        assert np.array_equal(ld2, ld) and np.array_equal(cl2, cl)
        c.set_newdata(np.where(miss, 0, Xnew))
        c.set_newdata_missing(*nref.cells_of(miss))
        ld3, cl3 = c.predict_state(cells=True)
        assert np.array_equal(ld3, ld) and np.array_equal(cl3, cl)


def test_a_state_with_empty_labels():
    """labels 3, 5 and 6 of 6 start empty and stay so: the predictive keeps their prior weight and prior terms"""
    X, _, _, _ = synth(2000, 20, 3, seed=2)
    z0 = np.random.default_rng(0).choice([1, 2, 4], X.shape[0]).astype(np.int32)
    Xnew, miss, Xna = _incomplete(np.random.default_rng(1), 300, 20, 0.3)
    with _chain("collapsed", X, 6, z0=z0, beta=0.7, gamma=0.4) as c:
        c.set_newdata(Xna, missing="na")
        for n in (0, 1, 3):
            c.sweeps(n)
            assert np.all(c.counts()[0][[2, 4, 5]] == 0)
            _check_state(c, Xnew, miss, 0.7, 0.4, "empty labels, %d more" % n)


def test_a_dp_state_at_maxk():
    """three generating components and maxK = 3: two clusters and one label that stays free (tests/test_gpu_predict.py)"""
    X, _, _, _ = synth(2000, 30, 3, seed=6)
    Xnew, miss, Xna = _incomplete(np.random.default_rng(3), 300, 30, 0.3)
    with _chain("dp", X, 3) as c:
        c.set_newdata(Xna, missing="na")
        _check_state(c, Xnew, miss, 0.5, 0.5, "dp before the first sweep (new cluster only)")
        c.sweeps(5)
        assert (c.counts()[0] > 0).sum() == 2
        _check_state(c, Xnew, miss, 0.5, 0.5, "dp at maxK")


# ---------------------------------------------------------------- 2. the sum over completions, on the device
@pytest.mark.parametrize("sampler,K", [("collapsed", 4), ("dp", 5), ("stickbreaking", 6), ("full", 3)])
def test_the_masked_density_is_the_sum_of_the_complete_row_kernel_over_all_completions(sampler, K):
    P = 6
    X, _, _, _ = synth(1500, P, 3, seed=11)
    rng = np.random.default_rng(4)
    Xnew = _newrows(rng, 41, P)
    miss = np.zeros((41, P), dtype=bool)
    for m in range(40):
        miss[m, rng.choice(P, m % 4, replace=False)] = True  # 0 to 3 cells
    miss[40] = True
    prior = dict(beta=0.5, gamma=0.5) if sampler == "dp" else dict(beta=0.7, gamma=0.4)  # (the DP sampler takes beta == gamma only)
    with _chain(sampler, X, K, **prior) as c:
        c.sweeps(3)
        c.set_newdata(pref.all_rows(P))
        dens = np.exp(c.predict_state())  # the existing complete-row kernel over all 2^P rows
        c.set_newdata(Xnew, missing=miss)
        ld = c.predict_state()
    weights = 1 << np.arange(P)
    want = np.array([np.log(dens[nref.completions(Xnew[m], miss[m]) @ weights].sum()) for m in range(41)])
    _close_logs(ld, want, miss.all(axis=1), "%s: masked logdens against the completions" % sampler)


# ---------------------------------------------------------------- 3. the fold
@pytest.mark.parametrize("sampler,K", [("collapsed", 5), ("dp", 9), ("stickbreaking", 6), ("full", 4)])
def test_the_fold(sampler, K):
    X, _, _, _ = synth(4000, 30, 3, seed=8)
    Xnew, miss, Xna = _incomplete(np.random.default_rng(5), 700, 30, 0.3)
    rows, cols = nref.cells_of(miss)
    n = 12

    def run(reset_first=False):
        with _chain(sampler, X, K, alpha=None) as c:
            c.set_newdata(Xna, responsibilities=True, missing="na")
            if reset_first:  # two folded sweeps thrown away: the same twelve states are folded afterwards
                c.sweeps_predict(2)
                c.predict_reset()
            else:
                c.sweeps(2)
            trace = c.sweeps_predict(n, trace=True)
            return trace, c.predictive(responsibilities=True)

    trace, pr = run()
    assert pr["n"] == n and pr["cells"]["n_folded"] == n and pr["cells"]["n_cells"] == rows.size
    assert np.array_equal(pr["cells"]["rows"], rows) and np.array_equal(pr["cells"]["cols"], cols)
    lj = np.empty((n, rows.size))
    with _chain(sampler, X, K, alpha=None) as c:  # the same chain stepped by hand
        c.set_newdata(Xna, missing="na")
        c.sweeps(2)
        for s in range(n):
            c.sweeps(1)
            ld, cl = c.predict_state(cells=True)
            assert np.array_equal(ld, trace[s]), s
            lj[s] = np.log(cl) + ld[rows]
        with pytest.raises(bm.BmmError):
            c.predictive()  # predict_state folds nothing
    want_lppd, want_mean = nref.fold(trace, lj, rows)
    _close_logs(pr["lppd"], want_lppd, miss.all(axis=1), sampler + " lppd")
    print(sampler, "largest |cell_mean - fold|", np.abs(pr["cells"]["mean"] - want_mean).max())
    np.testing.assert_allclose(pr["cells"]["mean"], want_mean, rtol=0, atol=1e-11)
    assert np.max(np.abs(pr["resp"].sum(axis=1) - 1.0)) < 1e-13
    for again in (run(), run(reset_first=True)):
        assert np.array_equal(again[0], trace)
        assert np.array_equal(again[1]["lppd"], pr["lppd"]) and np.array_equal(again[1]["resp"], pr["resp"])
        assert np.array_equal(again[1]["cells"]["mean"], pr["cells"]["mean"])


# ---------------------------------------------------------------- 4. the one call
def _na_split():
    X = load_dataset("K3_N1000_P5")
    fit, Xnew = np.asfortranarray(X[:800]), np.asfortranarray(X[800:])
    miss = nref.case_mask(np.random.default_rng(9), 200, 5, 0.3)
    Xna = Xnew.astype(np.float64)
    Xna[miss] = np.nan
    return fit, Xnew, miss, Xna


def _call_b(sampler, X, K, burnin, **kw):
    rng = np.random.default_rng(17)
    if sampler == "collapsed":
        return bm.gibbs_collapsed(X, 14, K, burnin=burnin, seed=21, initial_K=rng.integers(1, K + 1, X.shape[0]).astype(np.int32), **kw)
    if sampler == "dp":
        return bm.gibbs_dp(X, 14, burnin=burnin, maxK=K, seed=21, **kw)
    fn = bm.gibbs_stickbreaking if sampler == "stickbreaking" else bm.gibbs_full
    return fn(X, 14, K, burnin=burnin, seed=21, initial_pi=np.ones(K) / K,
              initial_theta=np.asfortranarray(0.1 + 0.8 * rng.random((K, X.shape[1]))), **kw)


@pytest.mark.parametrize("burnin", [6, 0])
@pytest.mark.parametrize("sampler", ["collapsed", "dp", "stickbreaking", "full"])
def test_one_call_equals_the_resident_chain(sampler, burnin):
    fit, Xnew, miss, Xna = _na_split()
    K, ns = 4, 14
    got = _call_b(sampler, fit, K, burnin, newdata=Xna, newdata_missing="na", predictive_trace=True, responsibilities=True)["predictive"]
    rng = np.random.default_rng(17)
    with bm.Chain(sampler, 800, 5, K, seed=21) as c:
        c.set_data(fit)
        if sampler == "collapsed":
            c.set_initial_labels(rng.integers(1, K + 1, 800).astype(np.int32))
        elif sampler != "dp":
            c.set_initial_params(np.ones(K) / K, np.asfortranarray(0.1 + 0.8 * rng.random((K, 5))))
        c.set_newdata(Xna, responsibilities=True, missing="na")
        first = burnin if burnin > 0 else 1   # without burn-in row 0 of the traces is the start, not a sweep
        c.sweeps(first - 1)
        trace = c.sweeps_predict(ns - first, trace=True)
        want = c.predictive(responsibilities=True)
    assert want["n"] == ns - first and got["cells"]["n_folded"] == ns - first
    assert np.array_equal(got["lppd"], want["lppd"]) and np.array_equal(got["resp"], want["resp"])
    assert np.array_equal(got["cells"]["mean"], want["cells"]["mean"])
    assert np.array_equal(got["cells"]["rows"], want["cells"]["rows"]) and np.array_equal(got["cells"]["cols"], want["cells"]["cols"])
    skip = first - burnin  # the NaN row 0 of a run without burn-in is left out
    assert got["logdens"].shape == (ns - burnin, 200) and np.all(np.isnan(got["logdens"][:skip]))
    assert np.array_equal(got["logdens"][skip:], trace)
    assert np.all((got["cells"]["mean"] > 0) & (got["cells"]["mean"] < 1))


@pytest.mark.parametrize("sampler", ["collapsed", "dp", "stickbreaking", "full"])
def test_incomplete_newdata_changes_nothing_of_the_chain(sampler):
    fit, Xnew, miss, Xna = _na_split()
    plain = _call(sampler, fit, 4)
    with_new = _call(sampler, fit, 4, newdata=Xna, newdata_missing="na")
    for key in plain:
        assert np.array_equal(plain[key], with_new[key], equal_nan=True), key
    assert set(with_new["predictive"]) == {"lppd", "cells"}
    # the mask given as a matrix over a complete newdata: the same cells, the same bits
    by_mask = _call(sampler, fit, 4, newdata=Xnew, newdata_missing=miss)["predictive"]
    assert np.array_equal(by_mask["lppd"], with_new["predictive"]["lppd"])
    assert np.array_equal(by_mask["cells"]["mean"], with_new["predictive"]["cells"]["mean"])


def test_missing_fitted_cells_and_incomplete_new_rows_in_one_run():
    """missing= imputes the fitted matrix, newdata_missing= integrates the new rows' cells out: the two combine, and the
    new rows change nothing of the chain or of the imputation"""
    fit, Xnew, miss, Xna = _na_split()
    hole = np.random.default_rng(3).random(fit.shape) < 0.1
    plain = _call("collapsed", fit, 4, missing=hole)
    both = _call("collapsed", fit, 4, missing=hole, newdata=Xna, newdata_missing="na")
    for key in ("z", "theta", "alpha"):
        assert np.array_equal(plain[key], both[key], equal_nan=True), key
    assert np.array_equal(plain["missing"]["mean"], both["missing"]["mean"])
    mean = both["predictive"]["cells"]["mean"]
    assert mean.shape == (int(miss.sum()),) and np.all((mean > 0) & (mean < 1))


@pytest.mark.parametrize("sampler", ["collapsed", "dp", "stickbreaking", "full"])
def test_a_set_without_missing_cells_is_byte_equal_with_and_without_the_keyword(sampler):
    fit, Xnew, _, _ = _na_split()
    kw = dict(newdata=Xnew, predictive_trace=True, responsibilities=True)
    without = _call(sampler, fit, 4, **kw)
    for form in ("na", np.zeros(Xnew.shape, dtype=bool)):
        with_kw = _call(sampler, fit, 4, newdata_missing=form, **kw)
        assert set(with_kw["predictive"]) == set(without["predictive"]) == {"lppd", "logdens", "resp"}
        for key in without["predictive"]:
            assert np.array_equal(without["predictive"][key], with_kw["predictive"][key], equal_nan=True), key
        for key in without:
            if key != "predictive":
                assert np.array_equal(without[key], with_kw[key], equal_nan=True), key
    with _chain(sampler, fit, 4) as c:  # ... and on a resident chain, a mask dropped again
        c.set_newdata(Xnew)
        c.sweeps(2)
        before = c.predict_state(responsibilities=True)
        c.set_newdata(Xnew, missing="na")
        assert all(np.array_equal(a, b) for a, b in zip(before, c.predict_state(responsibilities=True)))
        c.set_newdata_missing([3], [1])
        assert not np.array_equal(c.predict_state(), before[0])
        c.set_newdata_missing([], [])
        assert all(np.array_equal(a, b) for a, b in zip(before, c.predict_state(responsibilities=True)))
        c.sweeps_predict(1)
        assert "cells" not in c.predictive()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_chain_usable():
    X, _, _, _ = synth(1000, 10, 3, seed=1)
    Xnew, miss, Xna = _incomplete(np.random.default_rng(2), 100, 10, 0.3)
    L = _capi.lib()
    with pytest.raises(ValueError):  # NA without the keyword, as ever
        bm.gibbs_collapsed(X, 6, 3, seed=1, newdata=Xna)
    with pytest.raises(bm.BmmError, match="binary"):
        bm.gibbs_collapsed(X, 6, 3, seed=1, newdata=np.where(miss, _capi.NA_INTEGER, Xnew).astype(np.int32))
    with pytest.raises(ValueError, match="newdata_missing"):
        bm.gibbs_collapsed(X, 6, 3, seed=1, newdata=Xnew, newdata_missing=miss[:, :9])
    with pytest.raises(ValueError, match="newdata_missing"):
        bm.gibbs_collapsed(X, 6, 3, seed=1, newdata=Xnew, newdata_missing="nan")
    with pytest.raises(NotImplementedError):
        bm.gibbs_collapsed(X, 6, 3, chains=2, newdata=Xna, newdata_missing="na")
    assert "cells" in bm.gibbs_collapsed(X, 6, 3, seed=1, newdata=Xna, newdata_missing="na")["predictive"]
    assert "predictive" not in bm.gibbs_collapsed(X, 6, 3, seed=1)  # nothing stays armed
    rows, cols = nref.cells_of(miss)
    with _chain("collapsed", X, 3) as c:
        with pytest.raises(bm.BmmError, match="no new data"):
            c.set_newdata_missing(rows, cols)
        with pytest.raises(ValueError):
            c.set_newdata(Xna)
        with pytest.raises(ValueError):
            c.set_newdata(Xnew, missing=miss[:50])
        c.set_newdata(Xna, missing="na")
        c.sweeps(1)
        before = c.predict_state(cells=True)

        def refused(r, q, n=None):
            r, q = np.ascontiguousarray(r, dtype=np.int64), np.ascontiguousarray(q, dtype=np.int32)
            with pytest.raises(bm.BmmError):
                _capi.check(L.bmm_chain_set_newdata_missing(c._h, _capi.vp(r), _capi.vp(q), C.c_int64(r.size if n is None else n)))
            after = c.predict_state(cells=True)
            assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])  # the earlier mask is still there

        refused(rows[::-1], cols[::-1])                      # unsorted
        refused([3, 3, 2], [1, 4, 0])                        # rows out of order
        refused([3, 3], [4, 4])                              # a repeated cell
        refused([3, 100], [4, 0])                            # a row outside M
        refused([3, 4], [4, 10])                             # a column outside P
        refused([-1], [0])
        refused([3], [4], n=-1)
        with pytest.raises(bm.BmmError):
            _capi.check(L.bmm_chain_set_newdata_missing(c._h, None, None, C.c_int64(2)))
        c.sweeps_predict(2)
        pr = c.predictive()
        assert pr["n"] == 2 and pr["cells"]["n_folded"] == 2
        c.set_newdata(Xnew)  # a new set drops the mask
        with pytest.raises(ValueError):
            c.predict_state(cells=True)
        with pytest.raises(bm.BmmError):
            _capi.check(L.bmm_chain_get_predictive_cells(c._h, _capi.vp(np.zeros(4)), None))
        c.sweeps(1)
    with _chain("stickbreaking", X, 4) as c:
        c.set_shard(2000, 0)
        with pytest.raises(bm.BmmError, match="sharded"):
            c.set_newdata_missing(rows, cols)


# ---------------------------------------------------------------- 6. usefulness
def test_cell_mean_beats_the_observed_rates_on_planted_data():
    """synth, N = 4096, P = 24, K = 3, gibbs_collapsed; 512 held-out rows with 20 % of their cells hidden completely at
    random: the Brier score of cell_mean against the hidden values is below that of each feature's observed rate in the
    fitted data.  tests/test_predictive_na_ref.py holds the same data to the condition with the oracle's chain and the
    restatement first: 0.20973 against 0.23239."""
    X, Xnew, miss, truth, rate = nref.planted()
    r = bm.gibbs_collapsed(X, 150, 3, burnin=50, seed=0, newdata=Xnew, newdata_missing=miss)
    cells = r["predictive"]["cells"]
    assert cells["n_cells"] == truth.size and cells["n_folded"] == 100
    b_model, b_rate = nref.brier(cells["mean"], truth), nref.brier(rate[cells["cols"]], truth)
    print("Brier: cell_mean %.5f, observed rate %.5f" % (b_model, b_rate))
    assert b_model < b_rate
