"""Missing data on the device (include/bmm_mcmc.h "missing data"): the imputation step against the
host statement over bmm_spec.h (tests/na/na_host.cpp) bit for bit, the count invariant, the untouched behaviour of an
unarmed run, the exact posterior given the observed cells alone, a run against stepping by hand, the refusals, and
planted data."""
import importlib
import itertools
import os
import sys

import numpy as np
import pytest
from scipy.special import betaln, gammaln

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import na_ref as ref  # noqa: E402
import split_merge_checks as chk  # noqa: E402
from test_na_ref import seven_missing, seven_observations  # noqa: E402

pytestmark = pytest.mark.gpu

BETA = GAMMA = 0.5
ALPHA = 1.3
EXPLICIT = ("stickbreaking", "full")


@pytest.fixture(scope="module")
def bmm():
    return importlib.import_module("bmm_mcmc_amd")  # (the module the dbg_lib fixture steers)


def _data(N, P, frac, seed, comps=(0.15, 0.5, 0.85)):
    """(X, mis): a mixture, holes completely at random, one row with every cell missing (N > 1: the middle one) and
    feature 1 missing in every row, so that no label has an observed cell of it"""
    rng = np.random.default_rng(seed)
    comp = rng.integers(len(comps), size=N)
    X = (rng.random((N, P)) < np.asarray(comps)[comp][:, None]).astype(np.int32)
    mis = rng.random((N, P)) < frac
    mis[N // 2] = True
    if P > 1:
        mis[:, 1] = True
    return X, mis


def _chain(bmm, sampler, X, mis, K, batch, seed, arm=True):
    N, P = X.shape
    c = bmm.Chain(sampler, N, P, K, alpha=ALPHA, beta=BETA, gamma=GAMMA, batch=batch, seed=seed)
    c.set_data(np.asfortranarray(np.where(mis, 0, X).astype(np.int32)))
    rng = np.random.default_rng(seed)
    if sampler == "collapsed":
        c.set_initial_labels(rng.integers(1, K + 1, N).astype(np.int32))
    elif sampler in EXPLICIT:
        c.set_initial_params(np.ones(K) / K, 0.1 + 0.8 * rng.random((K, P)))
    if arm:
        c.set_missing(mask=mis)
    return c


def _completed(X, mis, bits):
    Xc = np.where(mis, 0, X).astype(np.int32)
    Xc[np.nonzero(mis)] = bits
    return Xc


# ---------------------------------------------------------------- 1. the step, device against host program, bit for bit
# (sampler, N, P, K, share of holes): a partial last word and a site in it (P = 31, 33, 65); one row; past one workgroup
# of sites (N = 257) and, with the test variant's two-workgroup grid, past one grid stride (N = 1025); a DP chain with
# unused labels; both sides of the LDS cap (K * P * 8 <= 48 KiB: K = 3 with P = 5 inside, K = 60 with P = 100 just inside,
# where the draw's 12 bytes per (k, j) pass 64 KiB of dynamic LDS, K = 50 with P = 200 outside);
# the four samplers.  Every case has a row with every cell missing and a feature no label has observed (the prior draw).
STEP_CASES = [("collapsed", 40, 31, 3, 0.3), ("dp", 40, 33, 12, 0.3), ("stickbreaking", 40, 65, 3, 0.3), ("full", 40, 33, 4, 0.3),
              ("collapsed", 1, 5, 2, 0.5), ("full", 1, 33, 2, 0.5), ("dp", 257, 65, 30, 0.5), ("stickbreaking", 257, 31, 5, 0.6),
              ("collapsed", 300, 200, 50, 0.2), ("stickbreaking", 300, 200, 50, 0.2), ("dp", 90, 5, 3, 0.3), ("full", 90, 5, 3, 0.3),
              ("collapsed", 300, 100, 60, 0.2), ("full", 300, 100, 60, 0.2)]


def _step_against_host(bmm, sampler, N, P, K, frac, seed=77):
    X, mis = _data(N, P, frac, N + P)
    rows, cols = np.nonzero(mis)
    with _chain(bmm, sampler, X, mis, K, max(1, N // 4), seed) as c:
        # the starting fill: the uniform of sweep 0 against the prior mean, rows without a seat
        bits0 = c.missing_state()
        fill = ref.host_step(np.where(mis, 0, X), np.full(N, -1), np.zeros(K), np.zeros((K, P)), rows, cols, seed, 0, BETA, GAMMA, mode=0)
        np.testing.assert_array_equal(bits0, fill["bits"][0])
        c.sweeps(2)
        z = c.labels() - 1
        Xc = _completed(X, mis, c.missing_state())
        Nk, S = c.counts()
        rNk, rS = ref.recount(Xc, z, K)
        np.testing.assert_array_equal(Nk, rNk)
        np.testing.assert_array_equal(S, rS)
        if sampler == "dp" and K >= 12:
            assert (Nk == 0).any()  # labels never used
        theta = c.params()[1] if sampler in EXPLICIT else None
        c.missing_reset()
        c.impute_step()
        h = ref.host_step(Xc, z, Nk, S, rows, cols, seed, 2, BETA, GAMMA, theta=theta)
        if theta is None:  # the feature no label observes: the prior's parameters
            for k in np.flatnonzero(Nk > 0):
                m, o, s, n, a, b, ph = h["cnt"][int(k) * P + 1]
                assert (s, n, a, b) == (0, 0, BETA, GAMMA)
        np.testing.assert_array_equal(c.missing_state(), h["bits"][0])
        Nk1, S1 = c.counts()
        np.testing.assert_array_equal(Nk1, Nk)
        np.testing.assert_array_equal(S1, h["S"])
        summ = c.missing_summary()
        assert summ["n_folded"] == 1
        np.testing.assert_array_equal(summ["mean"].view(np.uint64), h["sum"].view(np.uint64))
        np.testing.assert_array_equal(summ["mean_draw"], h["ones"].astype(np.float64))


@pytest.mark.parametrize("sampler,N,P,K,frac", STEP_CASES)
def test_step_equals_the_host_program(bmm, sampler, N, P, K, frac):
    _step_against_host(bmm, sampler, N, P, K, frac)


@pytest.mark.parametrize("sampler", ["collapsed", "stickbreaking"])
def test_step_past_one_grid_stride(bmm, dbg_lib, sampler):
    """N = 1025 rows, every one with holes, on two workgroups of 256 sites: a thread walks more than two sites"""
    dbg_lib.setenv("BMM_DEBUG_NA_GRID", "2")
    _step_against_host(bmm, sampler, 1025, 33, 3, 0.3)


# ---------------------------------------------------------------- 2. counts() is a recount of the completed matrix
@pytest.mark.parametrize("sampler", ["collapsed", "dp", "stickbreaking", "full"])
def test_counts_equal_a_recount_after_every_sweep(bmm, sampler):
    N, P, K = 600, 37, 6
    X, mis = _data(N, P, 0.25, 9)
    with _chain(bmm, sampler, X, mis, K, 50, 5) as c:
        assert sampler in EXPLICIT or c.batch == 50
        for t in range(5):
            c.sweeps(1)
            Xc = _completed(X, mis, c.missing_state())
            rNk, rS = ref.recount(Xc, c.labels() - 1, K)
            Nk, S = c.counts()
            np.testing.assert_array_equal(Nk, rNk)
            np.testing.assert_array_equal(S, rS)
            np.testing.assert_array_equal(Xc[~mis], X[~mis])  # no observed cell is ever touched


def test_declared_after_the_rows_have_labels(bmm):
    """the fill moves the folded counts where the rows already have seats"""
    N, P, K = 300, 33, 4
    X, mis = _data(N, P, 0.3, 4)
    for sampler in ("collapsed", "dp", "full"):
        with _chain(bmm, sampler, X, mis, K, 40, 6, arm=False) as c:
            c.sweeps(2)
            c.set_missing(mask=mis)
            for t in range(2):
                Xc = _completed(X, mis, c.missing_state())
                rNk, rS = ref.recount(Xc, c.labels() - 1, K)
                Nk, S = c.counts()
                np.testing.assert_array_equal(Nk, rNk)
                np.testing.assert_array_equal(S, rS)
                c.sweeps(1)


# ---------------------------------------------------------------- 3. nothing changes for who declares nothing
def _run(bmm, sampler, X, nsamples, K, seed, **kw):
    if sampler == "collapsed":
        return bmm.gibbs_collapsed(X, nsamples, K, alpha=ALPHA, burnin=kw.pop("burnin", 0), seed=seed, **kw)
    if sampler == "dp":
        return bmm.gibbs_dp(X, nsamples, alpha=ALPHA, maxK=K, burnin=kw.pop("burnin", 0), seed=seed, **kw)
    fn = bmm.gibbs_stickbreaking if sampler == "stickbreaking" else bmm.gibbs_full
    return fn(X, nsamples, K, alpha=ALPHA, burnin=kw.pop("burnin", 0), seed=seed, **kw)


@pytest.mark.parametrize("sampler", ["collapsed", "dp", "stickbreaking", "full"])
def test_zero_cells_and_none_are_the_unarmed_run(bmm, sampler):
    """(tests/golden holds no recorded run of a shape like this one: the comparison is with a second unarmed call)"""
    X, _ = _data(500, 20, 0.0, 2)
    X = np.asfortranarray(X)
    plain = _run(bmm, sampler, X, 30, 5, 21)
    again = _run(bmm, sampler, X, 30, 5, 21, missing=None)
    armed = _run(bmm, sampler, X, 30, 5, 21, missing=np.zeros(X.shape, dtype=bool))
    assert armed["missing"]["n_cells"] == 0 and armed["missing"]["n_folded"] == 0 and "missing" not in again
    for key in ("z", "theta", "alpha"):
        assert plain[key].tobytes() == again[key].tobytes() == armed[key].tobytes(), key


# ---------------------------------------------------------------- 4. the exact posterior given the observed cells
SWEEPS = 30_001


def _seven_na():
    X, obs = seven_observations(), seven_missing()
    Xna = X.astype(np.float64)
    Xna[~obs] = np.nan
    return X, obs, Xna


def test_dp_samples_the_posterior_given_the_observed_cells(bmm):
    X, obs, Xna = _seven_na()
    parts, w = ref.exact_dp_posterior(X, obs, ALPHA, BETA, GAMMA)
    r = bmm.gibbs_dp(Xna, SWEEPS, alpha=ALPHA, maxK=12, burnin=1, batch=1, seed=5, missing="na")
    assert r["missing"]["n_cells"] == 4 and r["missing"]["n_folded"] == SWEEPS - 1
    worst = chk.check_against_enumeration([ref.canonical(row) for row in r["z"]], parts, w)
    print("dp: worst deviation / standard error %.2f" % worst)


def _labelled_check(z, K, exact, states):
    """a labelled chain against the enumeration over all K^N allocations: the label shares and every co-clustering
    probability within 4 standard errors (batch means over 100 batches, never below the independent-sample error)"""
    N = z.shape[1]
    Z = np.array(states)
    feats = [((Z == k).mean(axis=1), "share of label %d" % k) for k in range(K)]
    feats += [((Z[:, i] == Z[:, j]).astype(float), "co(%d,%d)" % (i, j)) for i in range(N) for j in range(i + 1, N)]
    code = (z * (K ** np.arange(N - 1, -1, -1))).sum(axis=1)
    n = len(code) // 100 * 100
    worst = 0.0
    for f, name in feats:
        p = float(f @ exact)
        series = f[code[:n]]
        var_iid = float((f ** 2) @ exact - p * p)
        se = max(series.reshape(100, -1).mean(axis=1).std(ddof=1) / 10.0, np.sqrt(max(var_iid, 0.0) / n))
        dev = abs(series.mean() - p)
        print("%-20s exact %.5f chain %.5f dev/se %.2f" % (name, p, series.mean(), dev / se))
        assert dev <= 4.0 * se, (name, p, series.mean(), se)
        worst = max(worst, dev / se)
    return worst


def test_stickbreaking_samples_the_posterior_given_the_observed_cells(bmm):
    X, obs, Xna = _seven_na()
    K, alpha = 3, 1.7
    states = list(itertools.product(range(K), repeat=7))
    logw = []
    for z in states:
        z = np.array(z)
        n = np.bincount(z, minlength=K)
        lw = sum(betaln(1 + n[k], alpha + n[k + 1:].sum()) - betaln(1, alpha) for k in range(K - 1))
        logw.append(lw + sum(ref.block_loglik_observed(X, obs, np.flatnonzero(z == k), BETA, GAMMA) for k in range(K) if n[k]))
    exact = np.exp(np.array(logw) - max(logw))
    exact /= exact.sum()
    r = bmm.gibbs_stickbreaking(Xna, SWEEPS, K, alpha=alpha, burnin=1, seed=9, missing="na",
                                initial_pi=np.ones(K) / K, initial_theta=np.full((K, 3), 0.5))
    print("stick-breaking: worst %.2f" % _labelled_check(r["z"] - 1, K, exact, states))


def test_full_samples_the_posterior_given_the_observed_cells(bmm):
    X, obs, Xna = _seven_na()
    K, alpha = 2, 2.0
    states = list(itertools.product(range(K), repeat=7))
    logw = []
    for z in states:
        z = np.array(z)
        n = np.bincount(z, minlength=K)
        lw = float(np.sum(gammaln(alpha / K + n) - gammaln(alpha / K)))
        logw.append(lw + sum(ref.block_loglik_observed(X, obs, np.flatnonzero(z == k), BETA, GAMMA) for k in range(K) if n[k]))
    exact = np.exp(np.array(logw) - max(logw))
    exact /= exact.sum()
    r = bmm.gibbs_full(Xna, SWEEPS, K, alpha=alpha, burnin=1, seed=4, missing="na",
                       initial_pi=np.ones(K) / K, initial_theta=np.full((K, 3), 0.5))
    print("full: worst %.2f" % _labelled_check(r["z"] - 1, K, exact, states))


# ---------------------------------------------------------------- 5. a whole run against stepping by hand
@pytest.mark.parametrize("sampler", ["collapsed", "dp", "stickbreaking", "full"])
def test_run_equals_sweeps_by_hand(bmm, sampler):
    """the run's folds against a resident chain swept one sweep at a time (each sweep followed by its step) and a NumPy
    fold of what the chain shows after every sweep: the cells drawn, and for the explicit samplers theta[z_i, j], the
    rate each cell was drawn from; then one impute_step() by hand, which redraws the last step's bits"""
    N, P, K, nsamples, burnin, seed = 400, 21, 4, 12, 4, 31
    X, mis = _data(N, P, 0.3, 8)
    rows, cols = np.nonzero(mis)
    Xna = X.astype(np.float64)
    Xna[mis] = np.nan
    rng = np.random.default_rng(seed)
    kw = {}
    if sampler == "collapsed":
        z0 = rng.integers(1, K + 1, N).astype(np.int32)
        kw["initial_K"] = z0
    elif sampler in EXPLICIT:
        pi0, th0 = np.ones(K) / K, np.asfortranarray(0.1 + 0.8 * rng.random((K, P)))
        kw.update(initial_pi=pi0, initial_theta=th0)
    r1 = _run(bmm, sampler, Xna, nsamples, K, seed, burnin=burnin, missing="na", **kw)
    r2 = _run(bmm, sampler, Xna, nsamples, K, seed, burnin=burnin, missing=np.isnan(Xna), **kw)
    for key in ("mean", "mean_draw", "last"):
        assert r1["missing"][key].tobytes() == r2["missing"][key].tobytes(), key
    assert r1["z"].tobytes() == r2["z"].tobytes()
    m = r1["missing"]
    assert m["n_cells"] == len(rows) and m["n_folded"] == nsamples - burnin and abs(m["fraction"] - mis.mean()) < 1e-15
    np.testing.assert_array_equal(m["rows"], rows)
    np.testing.assert_array_equal(m["cols"], cols)
    batch = None if sampler in EXPLICIT else int(bmm.default_batch(sampler, N))
    c = bmm.Chain(sampler, N, P, K, alpha=ALPHA, beta=BETA, gamma=GAMMA, batch=batch, seed=seed)
    with c:
        c.set_data(np.asfortranarray(np.where(mis, 0, X).astype(np.int32)))
        if sampler == "collapsed":
            c.set_initial_labels(z0)
        elif sampler in EXPLICIT:
            c.set_initial_params(pi0, th0)
        c.set_missing(rows, cols)
        ones, sum_phi = np.zeros(len(rows)), np.zeros(len(rows))
        for t in range(1, nsamples):
            c.sweeps(1)
            if t == burnin - 1:
                c.missing_reset()
            if t >= burnin:
                ones += c.missing_state()
                if sampler in EXPLICIT:
                    sum_phi = sum_phi + c.params()[1][c.labels()[rows] - 1, cols]
        np.testing.assert_array_equal(c.labels(), r1["z"][-1])
        np.testing.assert_array_equal(c.missing_state(), m["last"])
        assert (ones / (nsamples - burnin)).tobytes() == m["mean_draw"].tobytes()
        s = c.missing_summary()
        assert s["n_folded"] == nsamples - burnin
        assert s["mean"].tobytes() == m["mean"].tobytes() and s["mean_draw"].tobytes() == m["mean_draw"].tobytes()
        if sampler in EXPLICIT:
            assert (sum_phi / (nsamples - burnin)).tobytes() == m["mean"].tobytes()
            c.impute_step()  # the same theta, labels and keys: the same bits again
            np.testing.assert_array_equal(c.missing_state(), m["last"])
        assert np.all((m["mean"] > 0) & (m["mean"] < 1))


# ---------------------------------------------------------------- 6. every refusal, with its code
def _code(bmm, name):
    import re
    hdr = open(os.path.join(ref.ROOT, "include", "bmm_mcmc.h")).read()
    return int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, hdr).group(1))


def _refused(bmm, code, fn, *a, **kw):
    with pytest.raises(bmm._capi.BmmError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals_of_the_resident_chain(bmm):
    ARG, UNS = _code(bmm, "BMM_E_ARG"), _code(bmm, "BMM_E_UNSUPPORTED")
    N, P, K = 200, 20, 4
    X, mis = _data(N, P, 0.2, 3)
    rows, cols = np.nonzero(mis)
    with _chain(bmm, "dp", X, mis, K, 20, 1, arm=False) as c:
        _refused(bmm, ARG, c.set_missing, [N], [0])           # out of range
        _refused(bmm, ARG, c.set_missing, [0], [P])
        _refused(bmm, ARG, c.set_missing, [0], [-1])
        _refused(bmm, ARG, c.set_missing, [3, 2], [0, 0])     # out of order
        _refused(bmm, ARG, c.set_missing, [3, 3], [4, 4])     # a cell twice
        c.sweeps(2)                                           # the chain is usable afterwards
        c.set_split_merge(1)
        _refused(bmm, UNS, c.set_missing, rows, cols)
        c.set_split_merge(0)
        c.set_missing(rows, cols)
        for fn, a in [(c.set_split_merge, (1,)), (c.set_loo, ()), (c.set_feature_select, ()), (c.set_temper, (0.5,)),
                      (c.set_pair_check, ()), (c.init_labels, ("kmodes", 3)), (c.sweep_probs, ())]:
            _refused(bmm, UNS, fn, *a)
        with bmm.Chain("dp", N, P, K, alpha=ALPHA, seed=2) as other:
            _refused(bmm, UNS, other.share_data, c)
        c.sweeps(2)
        Nk, S = c.counts()
        np.testing.assert_array_equal(S, ref.recount(_completed(X, mis, c.missing_state()), c.labels() - 1, K)[1])
        assert c.set_missing() == 0                           # withdrawn: the options are back
        c.set_loo()
        _refused(bmm, UNS, c.set_missing, rows, cols)
        c.set_loo(False)
    for arm_first in ("set_loo", "set_temper", "set_pair_check", "set_feature_select"):
        with _chain(bmm, "collapsed", X, mis, K, 20, 1, arm=False) as c:
            getattr(c, arm_first)(*((0.5,) if arm_first == "set_temper" else ()))
            _refused(bmm, UNS, c.set_missing, rows, cols)
            c.sweeps(1)
    with bmm.Chain("collapsed", N, P, K, alpha=ALPHA, seed=2, x_layout="int32") as c:  # the int32 layout
        c.set_data(np.asfortranarray(np.where(mis, 0, X).astype(np.int32)))
        c.set_initial_labels(np.ones(N, dtype=np.int32))
        _refused(bmm, UNS, c.set_missing, rows, cols)
        c.sweeps(1)
    with _chain(bmm, "collapsed", X, mis, K, 20, 1, arm=False) as a, bmm.Chain("collapsed", N, P, K, alpha=ALPHA, seed=3) as b:
        b.share_data(a)                                       # shared planes, either side
        _refused(bmm, UNS, a.set_missing, rows, cols)
        _refused(bmm, UNS, b.set_missing, rows, cols)
    with bmm.Chain("full", N, P, K, alpha=ALPHA, seed=2) as c:  # a sharded chain
        c.set_shard(2 * N, 0)
        c.set_data(np.asfortranarray(np.where(mis, 0, X).astype(np.int32)))
        _refused(bmm, UNS, c.set_missing, rows, cols)


class _NeverCalled:
    """host relabelling code for the hooked hand-off: the run is refused before it could be called"""

    def batch(self, p):
        raise AssertionError("the hand-off ran")

    def online(self, Q, p, j):
        raise AssertionError("the hand-off ran")


def test_refusals_of_the_run(bmm):
    ARG, UNS = _code(bmm, "BMM_E_ARG"), _code(bmm, "BMM_E_UNSUPPORTED")
    N, P, K = 200, 20, 4
    X, mis = _data(N, P, 0.2, 3)
    Xf = X.astype(np.float64)
    Xf[mis] = np.nan
    with pytest.raises(ValueError):
        bmm.gibbs_collapsed(Xf, 10, K, seed=1)                # missing=None: an NA cell is an error, as before
    Xi = X.copy()
    Xi[mis] = bmm._capi.NA_INTEGER
    with pytest.raises((ValueError, bmm._capi.BmmError)):
        bmm.gibbs_dp(Xi, 10, seed=1)
    for kw in (dict(loo=True), dict(select_features=True), dict(temper=2), dict(pair_check=True), dict(init="kmodes"),
               dict(relabel=True, stephens="device", burnin=10, burnrelabel=5), dict(relabel=True, stephens=_NeverCalled(), burnin=10, burnrelabel=5),
               dict(chains=2)):
        _refused(bmm, UNS, bmm.gibbs_collapsed, Xf, 20, K, seed=1, missing="na", **kw)
    _refused(bmm, UNS, bmm.gibbs_dp, Xf, 20, seed=1, missing="na", split_merge=1)
    _refused(bmm, UNS, bmm.gibbs_full, Xf, 20, K, seed=1, missing="na", loo=True)
    _refused(bmm, UNS, bmm.gibbs_stickbreaking, Xf, 20, K, seed=1, missing="na", chains=2)
    # the allocation sampler's run answers an armed declaration; afterwards nothing is armed
    rows, cols = np.nonzero(mis)
    mi = bmm._Missing(rows.astype(np.int64), cols.astype(np.int32), N, P)
    mi.arm()
    _refused(bmm, UNS, bmm.gibbs_allocation, np.where(mis, 0, X), 10, 6, seed=1)
    plain = bmm.gibbs_collapsed(np.where(mis, 0, X), 10, K, seed=1)
    assert "missing" not in plain
    # a cell list the C entry is handed out of order
    bad = bmm._Missing(rows[::-1].astype(np.int64).copy(), cols[::-1].astype(np.int32).copy(), N, P)
    bad.arm()
    args_ok = bmm.gibbs_collapsed(Xi, 10, K, burnin=5, seed=1, missing="na", partition="binder", logpost=True,
                                  newdata=X[:5], relabel="ecr")  # (the armed bad list was taken by this call's own arm)
    assert args_ok["missing"]["n_folded"] == 5 and "partition" in args_ok and "logpost" in args_ok and "predictive" in args_ok
    bad.arm()
    _refused(bmm, ARG, bmm.gibbs_collapsed, np.where(mis, 0, X), 10, K, seed=1)


# ---------------------------------------------------------------- 7. planted data
def test_imputed_means_beat_the_observed_rates_on_planted_data(bmm):
    """synth, N = 4096, P = 24, K = 3, 20 % of the cells hidden completely at random: the Brier score of missing["mean"]
    against the hidden values is below that of each feature's observed rate.  The restatement's finite chain
    (tests/na_ref.py finite_chain, 40 sweeps of which 15 burn-in, batch 1) over 8 seeds of data, holes and chain:
    Brier of the mean / of the observed rate: 0.2068 / 0.2290, 0.2071 / 0.2261, 0.2016 / 0.2230, 0.2006 / 0.2311,
    0.2152 / 0.2304, 0.2242 / 0.2394, 0.1922 / 0.2249, 0.2077 / 0.2332 -- it clears the case on all 8 (the first pair is
    the data and the holes of this test)."""
    synth = importlib.import_module("bmm_mcmc_amd.synth")
    X, labels, theta, w = synth.host_matrix(4096, 24, 3, 100)
    X = np.array(X)
    obs = np.random.default_rng(1000).random(X.shape) >= 0.2
    Xna = X.astype(np.float64)
    Xna[~obs] = np.nan
    r = bmm.gibbs_collapsed(Xna, 150, 3, burnin=50, seed=0, missing="na")
    rows, cols = np.nonzero(~obs)
    truth = X[rows, cols]
    rate = np.array([X[obs[:, j], j].mean() for j in range(24)])
    b_model, b_rate = ref.brier(r["missing"]["mean"], truth), ref.brier(rate[cols], truth)
    print("Brier: imputed mean %.5f, observed rate %.5f" % (b_model, b_rate))
    assert b_model < b_rate
