"""Pins of tests/predictive_na_ref.py, the NumPy restatement of the predictive of incomplete new rows (DESIGN.md section
28) that tests/test_gpu_predict_na.py holds the device kernels to:

  1. the masked density is the sum of predictive_ref's complete-row densities over all 2^|U| completions of the missing
     cells, for all three families, with an empty finite label, unused DP labels with beta != gamma, and a row with
     every cell missing;
  2. cell_state is the ratio of two complete-data marginals, and over x_d in {0, 1} the two joints add up to the masked
     density;
  3. cell_mean estimates what it should: folded over the states of a batch-1 oracle chain it lies within four standard
     errors (batch means of the ratio, 40 batches) of the exact P(x_d = 1 | x_O, X) by enumeration, and the plain mean
     of cell_state is a different number;
  4. the plan (bm.predict_na_plan) against hand-derived values, and the proof that the GPU cases reach both forms;
  5. the usefulness condition of the GPU test, first on the CPU: oracle chain and restatement.
"""
import numpy as np
import pytest

import bmm_mcmc_amd as bm
import predictive_na_ref as nref
import predictive_ref as pref
from bmm_mcmc_amd import _capi
from test_predictive_ref import (BETA, GAMMA, N7, P7, _batch_means_se, _ml, _partitions, _state, data7)  # noqa: F401

RTOL = 1e-12
P6 = 6


def _families():
    """(name, parts, complete-row terms function) of the three families on P = 6"""
    rng = np.random.default_rng(7)
    X, z, Nk, S = _state(rng, 60, P6, 5, empty=(2,))
    assert Nk[2] == 0
    yield ("collapsed", nref.collapsed_parts(Nk, S, 1.7, 60, 0.7, 0.4),
           lambda R: pref.collapsed_terms(R, Nk, S, 1.7, 60, 0.7, 0.4))
    X, z, Nk2, S2 = _state(rng, 60, P6, 6, empty=(1, 4))
    yield ("dp", nref.dp_parts(Nk2, S2, 0.9, 60, 0.3, 1.1), lambda R: pref.dp_terms(R, Nk2, S2, 0.9, 60, 0.3, 1.1))
    pi = rng.dirichlet(np.ones(4)) * 0.93  # (a truncated stick: the weights need not sum to 1)
    theta = rng.random((4, P6))
    yield ("explicit", nref.explicit_parts(pi, theta), lambda R: pref.explicit_terms(R, pi, theta))


def _rows_and_masks(rng):
    """rows with 0 to 3 cells masked (every count several times), and one with every cell missing"""
    X, miss = [], []
    for n_miss in (0, 1, 2, 3) * 6:
        X.append((rng.random(P6) < 0.5).astype(np.int32))
        m = np.zeros(P6, dtype=bool)
        m[rng.choice(P6, n_miss, replace=False)] = True
        miss.append(m)
    X.append(np.ones(P6, dtype=np.int32))
    miss.append(np.ones(P6, dtype=bool))
    return np.array(X), np.array(miss)


# ---------------------------------------------------------------- 1. the sum over completions
@pytest.mark.parametrize("family", ["collapsed", "dp", "explicit"])
def test_the_masked_density_is_the_sum_over_all_completions(family):
    name, parts, complete = next(f for f in _families() if f[0] == family)
    X, miss = _rows_and_masks(np.random.default_rng(1))
    ld = pref.logdens(nref.masked_terms(X, miss, parts))
    if family == "dp":
        assert np.isneginf(parts[0][[1, 4]]).all()  # the unused labels
    for m in range(X.shape[0]):
        comp = nref.completions(X[m], miss[m])
        assert comp.shape[0] == 1 << int(miss[m].sum())
        want = np.log(np.exp(pref.logdens(complete(comp))).sum())
        if miss[m].all() and family != "explicit":
            assert abs(ld[m]) < 1e-12 and abs(want) < 1e-12  # every cell missing: the weights sum to 1
        else:
            assert ld[m] == pytest.approx(want, rel=RTOL)
    t = nref.masked_terms(X, miss, parts)
    assert np.abs(pref.resp(t).sum(axis=1) - 1.0).max() < 1e-14


def test_a_row_of_every_cell_missing_has_density_sum_pi_for_explicit_parameters():
    name, parts, complete = next(f for f in _families() if f[0] == "explicit")
    ld = pref.logdens(nref.masked_terms(np.zeros((1, P6), dtype=np.int32), np.ones((1, P6), dtype=bool), parts))
    assert ld[0] == pytest.approx(np.log(np.exp(parts[0]).sum()), rel=RTOL)
    assert ld[0] == pytest.approx(np.log(0.93), rel=1e-10)


def test_masked_values_are_ignored_and_extreme_theta_stays_finite():
    """whatever X holds in a missing cell changes nothing; theta exactly 0 or 1 in a missing cell leaves the density
    finite (only terms of observed cells are ever added: nothing is taken back out)"""
    pi = np.array([0.3, 0.7])
    theta = np.array([[0.0, 0.4, 1.0], [0.2, 0.5, 0.9]])
    parts = nref.explicit_parts(pi, theta)
    miss = np.array([[True, False, True]])
    a = pref.logdens(nref.masked_terms(np.array([[1, 1, 0]]), miss, parts))
    b = pref.logdens(nref.masked_terms(np.array([[0, 1, 1]]), miss, parts))
    assert a[0] == b[0] == pytest.approx(np.log(0.3 * 0.4 + 0.7 * 0.5), rel=RTOL)


# ---------------------------------------------------------------- 2. the cells
@pytest.mark.parametrize("family", ["collapsed", "dp", "explicit"])
def test_cell_state_is_a_ratio_of_two_marginals_and_the_joints_add_up(family):
    name, parts, complete = next(f for f in _families() if f[0] == family)
    X, miss = _rows_and_masks(np.random.default_rng(2))
    ld, rp, lj, cs = nref.state(X, miss, parts)
    rows, cols = nref.cells_of(miss)
    assert rows.size == 6 * (1 + 2 + 3) + P6 and np.all(np.diff(rows * P6 + cols) > 0)
    for q, (m, d) in enumerate(zip(rows, cols)):
        comp = nref.completions(X[m], miss[m])
        dens = np.exp(pref.logdens(complete(comp)))
        one = comp[:, d] == 1
        assert cs[q] == pytest.approx(dens[one].sum() / dens.sum(), rel=1e-11)
        assert lj[q] == pytest.approx(np.log(dens[one].sum()), rel=RTOL)
        # the joint with a 0 in the cell: the cell observed at 0
        x0, m0 = X[m].copy(), miss[m].copy()
        x0[d], m0[d] = 0, False
        l0 = pref.logdens(nref.masked_terms(x0[None, :], m0[None, :], parts))[0]
        assert np.exp(lj[q]) + np.exp(l0) == pytest.approx(np.exp(ld[m]), rel=RTOL)
        assert 0.0 < cs[q] < 1.0


def test_the_fold_weights_the_states_by_the_density_of_the_observed_cells():
    ld = np.log(np.array([[0.1], [0.4]]))
    lj = np.log(np.array([[0.05], [0.1]]))
    lppd, mean = nref.fold(ld, lj, np.array([0]))
    assert lppd[0] == pytest.approx(np.log(0.25), rel=RTOL)
    assert mean[0] == pytest.approx(0.15 / 0.5, rel=RTOL)          # not (0.5 + 0.25) / 2
    assert np.exp(lj - ld).mean() == pytest.approx(0.375, rel=RTOL)


# ---------------------------------------------------------------- 3. what cell_mean estimates
ROW7 = np.array([0, 0, 0], dtype=np.int32)      # the new row: cell 2 observed at 0 ...
MISS7 = np.array([True, True, False])           # ... cells 0 and 1 hidden


def _exact_cells(exact):
    """P(x_d = 1 | x_O, X) of the two hidden cells from the exact p(x* | X) of all 2^P complete rows"""
    rows = pref.all_rows(P7)
    comp = rows[:, 2] == ROW7[2]
    return np.array([exact[comp & (rows[:, d] == 1)].sum() / exact[comp].sum() for d in (0, 1)])


def _ratio_se(q, p, nbatch=40):
    """standard error of sum q / sum p over a correlated series by batch means of the ratio"""
    S = q.shape[0] // nbatch * nbatch
    rb = q[:S].reshape(nbatch, -1, q.shape[1]).sum(axis=1) / p[:S].reshape(nbatch, -1, 1).sum(axis=1)
    return rb.std(axis=0, ddof=1) / np.sqrt(nbatch)


def test_dp_cell_mean_estimates_the_exact_conditional_over_all_877_partitions(oracle, data7):  # noqa: F811
    """The chain of test_dp_lppd_estimates_the_exact_predictive_over_all_877_partitions (200 000 kept sweeps, batch 1,
    alpha = 1.3).  Measured: exact 0.598144, 0.480560; folded cell_mean 0.598054, 0.480639 (standard errors 8.8e-5,
    9.3e-5: -1.0 and 0.9 of them away); the plain mean of cell_state of cell 0 is 0.597542, 7.0 of its own standard
    errors from the exact value -- the estimator the header warns against is a different number on this data."""
    from scipy.special import gammaln
    alpha, sweeps, burn = 1.3, 200_000, 2_000
    rows = pref.all_rows(P7)
    logw, pred = [], []
    for p in _partitions(N7):
        blocks = {}
        for i, b in enumerate(p):
            blocks.setdefault(b, []).append(i)
        logw.append(len(blocks) * np.log(alpha) + sum(gammaln(len(r)) + _ml(data7[r]) for r in blocks.values()))
        px = []
        for x in rows:
            v = alpha / (N7 + alpha) * np.exp(_ml(x))
            for r in blocks.values():
                v += len(r) / (N7 + alpha) * np.exp(_ml(np.vstack([data7[r], x])) - _ml(data7[r]))
            px.append(v)
        pred.append(px)
    assert len(logw) == 877
    post = np.exp(np.array(logw) - max(logw))
    post /= post.sum()
    exact = _exact_cells(post @ np.array(pred))
    maxK = 12
    r = oracle.dp(data7, sweeps + burn, alpha, BETA, GAMMA, 1, 1, burn, maxK, seed=5, batch=1)
    states, inverse = np.unique(r["z"], axis=0, return_inverse=True)
    ld_u, lj_u = np.empty((len(states), 1)), np.empty((len(states), 2))
    for u, z in enumerate(states):
        Nk, S = pref.counts_from_labels(data7, z, maxK)
        ld, _, lj, _ = nref.state(ROW7[None, :], MISS7[None, :], nref.dp_parts(Nk, S, alpha, N7, BETA, GAMMA))
        ld_u[u], lj_u[u] = ld, lj
    ld_s, lj_s = ld_u[inverse.ravel()], lj_u[inverse.ravel()]
    _, got = nref.fold(ld_s, lj_s, np.array([0, 0]))
    se = _ratio_se(np.exp(lj_s), np.exp(ld_s[:, 0]))
    print("dp: exact", exact, "cell_mean", got, "se", se, "z-scores", (got - exact) / se)
    assert np.all(np.abs(got - exact) < 4 * se), (got, exact, se)
    cell_state = np.exp(lj_s - ld_s)
    plain, se_plain = cell_state.mean(axis=0), _batch_means_se(cell_state)
    print("dp: plain mean of cell_state", plain, "se", se_plain, "z-scores", (plain - exact) / se_plain)
    assert abs(plain[0] - exact[0]) > 4 * se_plain[0] and abs(plain[0] - exact[0]) > 4 * se[0]


def test_full_cell_mean_estimates_the_exact_conditional_over_all_128_allocations(oracle, data7):  # noqa: F811
    """The chain of test_full_lppd_estimates_the_exact_predictive_over_all_128_allocations (40 000 kept sweeps, K = 2,
    alpha = 2).  Measured: exact 0.606402, 0.468445; cell_mean 0.606335, 0.469245 (standard errors 1.1e-3, 1.3e-3).
    With a tenth of the DP chain's sweeps and pi, theta sampled, the plain mean of cell_state (0.606235, 0.469125) is
    within its own standard error of both: this chain cannot tell the two estimators apart, the DP chain above does."""
    import itertools

    from scipy.special import gammaln
    K, alpha, sweeps, burn = 2, 2.0, 40_000, 2_000
    rows = pref.all_rows(P7)
    logw, pred = [], []
    for z in itertools.product(range(K), repeat=N7):
        z = np.array(z)
        n = np.bincount(z, minlength=K)
        logw.append(float(np.sum(gammaln(alpha / K + n) - gammaln(alpha / K))) + sum(_ml(data7[z == k]) for k in range(K) if n[k]))
        px = []
        for x in rows:
            v = 0.0
            for k in range(K):
                blk = data7[z == k]
                v += (alpha / K + n[k]) / (alpha + N7) * np.exp(_ml(np.vstack([blk, x])) - (_ml(blk) if n[k] else 0.0))
            px.append(v)
        pred.append(px)
    assert len(logw) == 128
    post = np.exp(np.array(logw) - max(logw))
    post /= post.sum()
    exact = _exact_cells(post @ np.array(pred))
    r = oracle.full(data7, np.ones(K) / K, np.full((K, P7), 0.5), sweeps + burn, K, alpha, BETA, GAMMA, 1, 1, burn, seed=4)
    ld_s, lj_s = np.empty((sweeps, 1)), np.empty((sweeps, 2))
    for s in range(sweeps):
        ld, _, lj, _ = nref.state(ROW7[None, :], MISS7[None, :], nref.explicit_parts(r["pi"][s], r["theta"][:, :, s]))
        ld_s[s], lj_s[s] = ld, lj
    _, got = nref.fold(ld_s, lj_s, np.array([0, 0]))
    se = _ratio_se(np.exp(lj_s), np.exp(ld_s[:, 0]))
    print("full: exact", exact, "cell_mean", got, "se", se, "z-scores", (got - exact) / se)
    assert np.all(np.abs(got - exact) < 4 * se), (got, exact, se)


# ---------------------------------------------------------------- 4. the plan
def _gw(sampler, K, P):
    return _capi.lib().bmm_spec_group_width_for(_capi.SAMPLER_CODE[sampler], K, P)


def test_the_plan_against_hand_derived_values():
    # the north star's table shape: 10 groups of 5, 20 accumulators: 2 * 10 * 20 * 32 doubles, 20 constants, 256 of exp
    assert bm.predict_na_plan("collapsed", 20, 50) == {"form": "lds", "lds_bytes": (12800 + 20 + 256) * 8, "threads": 512,
                                                       "table_bytes": 104608}
    # 64 accumulators at P = 50: groups of 4, 13 of them: 2 * 13 * 64 * 16 doubles do not fit
    assert _gw("collapsed", 64, 50) == 4
    assert bm.predict_na_plan("collapsed", 64, 50) == {"form": "global", "lds_bytes": 0, "threads": 256,
                                                       "table_bytes": (26624 + 64 + 256) * 8}
    # the example of the design: KT = 64, P = 128: two tables of 32 * 64 * 16 doubles, 524 288 bytes
    assert bm.predict_na_plan("collapsed", 64, 128)["table_bytes"] == 524288 + (64 + 256) * 8
    assert bm.predict_na_plan("collapsed", 64, 128)["form"] == "global"
    # the smallest shape: one group, 4 accumulators
    assert bm.predict_na_plan("collapsed", 2, 1) == {"form": "lds", "lds_bytes": 4128, "threads": 512, "table_bytes": 4128}
    # the DP counts its new-cluster column: 19 labels are 20 categories, 20 labels are 21 and take 24 accumulators
    assert bm.predict_na_plan("dp", 19, 50) == bm.predict_na_plan("collapsed", 20, 50)
    assert bm.predict_na_plan("dp", 20, 50)["table_bytes"] == (2 * 10 * 24 * 32 + 24 + 256) * 8
    # a generic shape: 70 categories are 72 accumulators in 3 groups of 4
    assert bm.predict_na_plan("stickbreaking", 70, 10) == {"form": "global", "lds_bytes": 0, "threads": 256,
                                                          "table_bytes": (2 * 3 * 72 * 16 + 72 + 256) * 8}
    assert bm.predict_na_plan("collapsed", 3, 150)["form"] == "global"
    # the LDS form in groups of 4: the sweep's own image needs them, the doubled head still fits
    assert _gw("collapsed", 20, 120) == 4
    assert bm.predict_na_plan("collapsed", 20, 120) == {"form": "lds", "lds_bytes": (2 * 30 * 20 * 16 + 20 + 256) * 8,
                                                        "threads": 512, "table_bytes": 155808}
    with pytest.raises(bm.BmmError):
        bm.predict_na_plan("collapsed", 0, 5)


def test_the_plan_is_the_restated_rule_on_every_case():
    for sampler, K, P, *_ in nref.CASES:
        assert bm.predict_na_plan(sampler, K, P) == nref.plan(sampler, K, P, _gw(sampler, K, P)), (sampler, K, P)
    for sampler in ("collapsed", "dp", "stickbreaking", "full"):
        for K, P in [(1, 1), (5, 128), (12, 128), (16, 128), (20, 128), (24, 100), (63, 20), (64, 20), (65, 20), (40, 60)]:
            assert bm.predict_na_plan(sampler, K, P) == nref.plan(sampler, K, P, _gw(sampler, K, P)), (sampler, K, P)


def test_the_cases_reach_every_form():
    """the GPU cases of tests/test_gpu_predict_na.py run the LDS form in groups of 5 and of 4, and the global form on a
    resident shape (score columns of its own) and on both kinds of generic shape (the chain's score columns)"""
    got = set()
    for sampler, K, P, *_ in nref.CASES:
        p = bm.predict_na_plan(sampler, K, P)
        Kc = K + 1 if sampler == "dp" else K
        generic = Kc > 64 or P > 128
        got.add((p["form"], _gw(sampler, K, P) if p["form"] == "lds" else 0, generic))
        assert p["lds_bytes"] <= 163840
    assert got == {("lds", 5, False), ("lds", 4, False), ("global", 0, False), ("global", 0, True)}
    assert {(s, K, P) for s, K, P, *_ in nref.CASES} >= {
        ("collapsed", 2, 1), ("collapsed", 3, 5), ("collapsed", 3, 33), ("collapsed", 4, 37), ("collapsed", 20, 50),
        ("collapsed", 32, 100), ("collapsed", 64, 50), ("dp", 19, 50), ("stickbreaking", 50, 50), ("full", 8, 100),
        ("collapsed", 3, 150), ("stickbreaking", 70, 10)}
    assert {c[5] for c in nref.CASES} == {1, 511, 513, 1300} and {c[6] for c in nref.CASES} == {0.1, 0.6}
    assert any(P > 128 for _, _, P, *_ in nref.CASES) and any(K > 64 for _, K, *_ in nref.CASES)


# ---------------------------------------------------------------- 5. usefulness, first on the CPU
def test_cell_mean_beats_the_observed_rates_on_planted_data(oracle):
    """The data, the held-out rows and the holes of the GPU test (tests/test_gpu_predict_na.py), the oracle's finite
    chain (batch 1, 60 sweeps of which 20 burn-in) and the restatement's fold.  Measured: Brier score of cell_mean
    0.20973 against 0.23239 for the feature's observed rate in the fitted data."""
    X, Xnew, miss, truth, rate = nref.planted()
    N, K = X.shape[0], 3
    z0 = np.random.default_rng(0).integers(1, K + 1, N).astype(np.int32)
    r = oracle.collapsed(X, z0, 60, K, 1.0, 0.5, 0.5, 1, 1, 20, seed=0, batch=1)
    rows, cols = nref.cells_of(miss)
    ld_s, lj_s = [], []
    for s in range(r["z"].shape[0]):
        Nk, S = pref.counts_from_labels(X, r["z"][s], K)
        ld, _, lj, _ = nref.state(Xnew, miss, nref.collapsed_parts(Nk, S, float(np.ravel(r["alpha"])[s]), N, 0.5, 0.5))
        ld_s.append(ld)
        lj_s.append(lj)
    _, mean = nref.fold(np.array(ld_s), np.array(lj_s), rows)
    b_model, b_rate = nref.brier(mean, truth), nref.brier(rate[cols], truth)
    print("Brier: cell_mean %.5f, observed rate %.5f" % (b_model, b_rate))
    assert b_model < b_rate
