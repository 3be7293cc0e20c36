"""The log joint trace and the keep-best allocation on the device (include/bmm_mcmc.h "log joint trace", DESIGN.md
section 20).  The device's row is held to the host statement of bmm_spec.h (tests/logpost/logpost_host.cpp) bit for
bit, from the counts, alpha, K and mask read off the same chain, and to the SciPy restatement (tests/logpost_ref.py)
within eps (LGAMMA_ULPS + 2 + depth) sum max(1, |v_i|) (tests/logpost_host.py: bound); its differences are tied to what
the split-merge, eject / absorb and feature steps report; the run option, the keep-best state and the stand-alone call
are tied to the resident calls."""
import os
import sys

import numpy as np
import pytest
from scipy.special import gammaln

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_ref  # noqa: E402
import logpost_host as host  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("log_lik", "log_prior", "log_hyper", "log_joint")
A, B = 2.0, 0.5  # the Gamma(a, b) prior of a sampled alpha


@pytest.fixture(scope="module")
def bmm():
    import importlib
    return importlib.import_module("bmm_mcmc_amd")


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def _mixture(N, P, thetas, seed):
    rng = np.random.default_rng(seed)
    comp = rng.integers(len(thetas), size=N)
    X = (rng.random((N, P)) < np.asarray(thetas)[comp][:, None]).astype(np.int32)
    return np.asfortranarray(X), comp


def _chain(bmm, sampler, X, K, alpha, beta, gamma, seed=3, batch=None, layout=None, labels=None):
    N, P = X.shape
    c = bmm.Chain(sampler, N, P, K, alpha=alpha, beta=beta, gamma=gamma, a=A, b=B, batch=batch, seed=seed, x_layout=layout)
    c.set_data(X)
    rng = np.random.default_rng(seed)
    if sampler == "collapsed":
        c.set_initial_labels(rng.integers(1, (labels or K) + 1, N).astype(np.int32))
    elif sampler in ("stickbreaking", "full"):
        pi = rng.random(K) + 0.1
        c.set_initial_params(pi / pi.sum(), rng.random((K, P)) * 0.8 + 0.1)
    return c


def _row(c):
    st = c.logpost_state()
    return np.array([st[k] for k in KEYS])


def _check_state(c, model, beta, gamma, sample_alpha, **kw):
    """the device's row against the host program (bits) and the restatement (bound), from what the chain itself holds;
    returns (row, bound, error / bound)"""
    got = _row(c)
    Nk, S = c.counts()
    alpha = c.alpha()
    N = c.N
    assert Nk.sum() == N
    kw = dict(kw, sample_alpha=sample_alpha, a=A, b=B)
    bits, vals = host.run(model, Nk, S, N, alpha, beta, gamma, **kw)
    assert np.array_equal(_bits(got), bits), (got, vals)
    ratio = host.check(model, got, Nk, S, N, alpha, beta, gamma, **kw)
    np.testing.assert_array_equal(_bits(_row(c)), bits)  # one state gives the same bits twice
    return got, host.bound(model, Nk, S, N, alpha, beta, gamma, **kw), ratio


# ---------------------------------------------------------------- 1. bits and bound over the shapes
# (sampler, N, P, K, labels the start uses, layout, batch): cell counts K P below, at and above one pass of the 256
# lanes; P = 130 (the generic kernel) and P = 1024 with K = 13; K = 70 above the resident kernels' 64; N = 1, 63, 64, 65,
# 1300; empty labels (K = 20 on N = 40; a DP chain with maxK = 30 on three clusters); the int32 layout; batch 700 of 3000
SHAPES = [
    ("collapsed", 63, 5, 3, None, None, None), ("collapsed", 300, 32, 32, None, None, None),
    ("collapsed", 200, 41, 25, None, None, None), ("full", 64, 130, 4, None, None, None),
    ("collapsed", 500, 1024, 13, None, None, None), ("collapsed", 400, 6, 70, None, None, None),
    ("collapsed", 1, 3, 2, None, None, None), ("collapsed", 40, 7, 20, None, None, None),
    ("dp", 1300, 12, 30, None, None, None), ("stickbreaking", 65, 9, 6, None, None, None),
    ("full", 300, 20, 5, None, None, None), ("collapsed", 300, 37, 5, None, "int32", None),
    ("dp", 300, 37, 8, None, "int32", None), ("collapsed", 3000, 10, 6, None, None, 700),
]


@pytest.mark.parametrize("sample_alpha", [False, True])
@pytest.mark.parametrize("sampler,N,P,K,labels,layout,batch", SHAPES)
def test_the_row_is_the_host_statement_bit_for_bit_and_the_restatement_within_the_bound(bmm, sampler, N, P, K, labels, layout,
                                                                                        batch, sample_alpha):
    X, _ = _mixture(N, P, [0.2, 0.5, 0.8], N + P)
    beta, gamma = (0.5, 0.5) if sampler == "dp" else (0.7, 1.9)
    worst = 0.0
    with _chain(bmm, sampler, X, K, None if sample_alpha else 1.3, beta, gamma, batch=batch, layout=layout, labels=labels) as c:
        if sampler == "collapsed":  # before the first sweep: every statistic is in the delta replicas
            worst = max(worst, _check_state(c, sampler, beta, gamma, sample_alpha)[2])
            assert c.sweep_index == 0
        for n in (1, 3):  # after 1 and after 4 sweeps
            c.sweeps(n)
            worst = max(worst, _check_state(c, sampler, beta, gamma, sample_alpha)[2])
    print("largest error / bound: %.3e" % worst)


def test_unseated_chains_are_refused_and_stay_usable(bmm):
    X, _ = _mixture(100, 8, [0.2, 0.8], 1)
    for sampler in ("dp", "stickbreaking", "full"):
        with _chain(bmm, sampler, X, 5, 1.0, 0.5, 0.5) as c:
            with pytest.raises(bmm.BmmError) as e:
                c.logpost_state()
            assert e.value.code == 5  # BMM_E_STATE
            c.set_logpost(True)
            rows = c.sweeps_logpost(2, trace=True)
            assert np.all(np.isfinite(rows))
            np.testing.assert_array_equal(_bits(rows[1]), _bits(_row(c)))


# ---------------------------------------------------------------- 2. ties to the moves and steps of the device
def _accepted(step_fn, row_fn, want, tries):
    """the first accepted move of every kind in `want`: {kind: (row before, step record, row after)}"""
    found = {}
    for _ in range(tries):
        before = row_fn()
        d = step_fn()
        if d["accepted"] and d["kind"] in want and d["kind"] not in found:
            found[d["kind"]] = (before, d, row_fn())
        if len(found) == len(want):
            break
    return found


def test_an_accepted_split_and_merge_change_the_log_joint_by_what_the_step_reports(bmm):
    N, P, K = 400, 20, 12
    X, comp = _mixture(N, P, [0.15, 0.85], 8)
    planted = {"merge": np.where(comp == 0, 1 + np.random.default_rng(2).integers(2, size=N), 3).astype(np.int32),
               "split": np.ones(N, dtype=np.int32)}
    for kind, z0 in planted.items():
        with _chain(bmm, "dp", X, K, 1.0, 0.5, 0.5, seed=5) as c:
            c.sweeps(1)
            c.set_labels(z0)
            c.set_split_merge(1, 2)
            c.set_split_merge(0, 2)
            got = _accepted(c.split_merge_step, lambda: _check_state(c, "dp", 0.5, 0.5, False), [kind], 300)
            assert kind in got
            (r0, b0, _), d, (r1, b1, _) = got[kind]
            delta = (r1[0] + r1[1]) - (r0[0] + r0[1])
            print(kind, delta, d["log_prior"] + d["log_lik"], b0 + b1)
            assert abs(delta - (d["log_prior"] + d["log_lik"])) <= b0 + b1


def test_an_accepted_eject_and_absorb_and_set_k_change_the_log_joint_by_what_they_should(bmm):
    N, P, maxK, a = 300, 16, 6, 0.9
    lpk = bmm.log_prior_k("poisson", maxK)  # the vector the chain is armed with, to the bit
    np.testing.assert_allclose(lpk, alloc_ref.poisson_prior(maxK), rtol=1e-13)

    def state(c):
        return _check_state(c, "allocation", 0.5, 0.8, False, k_open=c.k(), log_prior_k=lpk)

    # an eject from one label over two well separated components; an absorb of two labels cut through one component
    cases = {"eject": (_mixture(N, P, [0.15, 0.85], 4)[0], 1, 1), "absorb": (_mixture(N, P, [0.5], 4)[0], 2, 2)}
    for kind, (X, labels, k0) in cases.items():
        with _chain(bmm, "collapsed", X, maxK, a, 0.5, 0.8, seed=9, labels=labels) as c:
            c.set_alloc("poisson", 0, 1.0)
            c.set_k(k0)
            r_low = state(c)
            c.set_k(maxK)  # K up: only log p(K) and the Dirichlet's normaliser change
            r_up = state(c)
            want = (lpk[maxK - 1] - lpk[k0 - 1]) + ((gammaln(maxK * a) - gammaln(maxK * a + N)) - (gammaln(k0 * a) - gammaln(k0 * a + N)))
            assert abs((r_up[0][1] - r_low[0][1]) - want) <= r_low[1] + r_up[1]
            assert r_up[0][0] == r_low[0][0]
            c.set_k(k0)  # and down again: the bits of before
            np.testing.assert_array_equal(_bits(state(c)[0]), _bits(r_low[0]))
            got = _accepted(c.alloc_step, lambda: state(c), [kind], 300)
            assert kind in got
            (r0, b0, _), d, (r1, b1, _) = got[kind]
            delta = (r1[0] + r1[1]) - (r0[0] + r0[1])
            print(kind, delta, d["log_prior"] + d["log_lik"], b0 + b1)
            assert abs(delta - (d["log_prior"] + d["log_lik"])) <= b0 + b1


@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
def test_flipping_a_feature_changes_the_log_joint_by_its_lambda(bmm, sampler):
    N, P, K, rho = 300, 37, 6, 0.3
    X, _ = _mixture(N, P, [0.2, 0.5, 0.8], 6)
    with _chain(bmm, sampler, X, K, 1.3, 0.5, 0.5) as c:
        c.set_feature_select(True, rho)
        c.sweeps(3)
        step = c.feature_step()
        c.set_feature_select(False)
        mask = c.features()
        np.testing.assert_array_equal(mask, step["gamma"])
        base = _check_state(c, sampler, 0.5, 0.5, False, mask=mask, rho=rho)
        for d in (0, 5, 31, 32, P - 1):
            flipped = mask.copy()
            flipped[d] ^= 1
            c.set_features(flipped)
            r = _check_state(c, sampler, 0.5, 0.5, False, mask=flipped, rho=rho)
            sign = 1.0 if flipped[d] else -1.0
            assert abs((r[0][3] - base[0][3]) - sign * step["lambda"][d]) <= r[1] + base[1]
        c.set_features(mask)


def test_with_every_feature_included_the_bits_are_the_unmasked_chains(bmm):
    """log_lik and log_prior, bit for bit; log_hyper differs by the mask's own prior, P log rho, and log_joint by that"""
    N, P, K = 300, 37, 6
    X, _ = _mixture(N, P, [0.2, 0.5, 0.8], 6)
    with _chain(bmm, "collapsed", X, K, None, 0.7, 1.9) as plain, _chain(bmm, "collapsed", X, K, None, 0.7, 1.9) as masked:
        masked.set_features(np.ones(P, dtype=np.uint8))
        for c in (plain, masked):
            c.sweeps(3)
        np.testing.assert_array_equal(plain.labels(), masked.labels())
        r0, r1 = _row(plain), _row(masked)
        np.testing.assert_array_equal(_bits(r0[:2]), _bits(r1[:2]))
        _check_state(masked, "collapsed", 0.7, 1.9, True, mask=np.ones(P, dtype=np.uint8), rho=0.5)
        assert r1[2] - r0[2] == pytest.approx(P * np.log(0.5), rel=1e-14)


# ---------------------------------------------------------------- 3. keep-best and whole runs
RUN = dict(nsamples=9, K=4, burnin=2, seed=7, batch=50)


def _run_data():
    X, _ = _mixture(300, 12, [0.2, 0.5, 0.8], 2)
    z0 = np.random.default_rng(1).integers(1, 5, 300).astype(np.int32)
    return X, z0


def _rows_of(lp):
    return np.stack([lp[k] for k in KEYS], axis=1)


def test_the_trace_of_a_run_is_logpost_state_sweep_by_sweep_on_a_resident_twin(bmm):
    X, z0 = _run_data()
    out = bmm.gibbs_collapsed(X, initial_K=z0, logpost=True, a=A, b=B, beta=0.7, gamma=1.9, **RUN)
    lp = out["logpost"]
    rows = _rows_of(lp)
    with bmm.Chain("collapsed", 300, 12, 4, alpha=None, beta=0.7, gamma=1.9, a=A, b=B, batch=50, seed=7) as c:
        c.set_data(X)
        c.set_initial_labels(z0)
        for j in range(1, RUN["nsamples"]):
            c.sweeps(1)
            if j >= RUN["burnin"]:
                np.testing.assert_array_equal(c.labels(), out["z"][j - RUN["burnin"]])
                np.testing.assert_array_equal(_bits(_row(c)), _bits(rows[j - RUN["burnin"]]))
    assert lp["n_used"] == 7 and lp["best"] == int(np.argmax(lp["log_joint"]))
    np.testing.assert_array_equal(lp["z_map"], out["z"][lp["best"]])
    assert np.isfinite(lp["ess"]) or lp["n_used"] < 8
    again = bmm.gibbs_collapsed(X, initial_K=z0, logpost=True, a=A, b=B, beta=0.7, gamma=1.9, **RUN)["logpost"]
    np.testing.assert_array_equal(_bits(_rows_of(again)), _bits(rows))  # two runs give the same bits
    np.testing.assert_array_equal(again["z_map"], lp["z_map"])
    plain = bmm.gibbs_collapsed(X, initial_K=z0, a=A, b=B, beta=0.7, gamma=1.9, **RUN)
    np.testing.assert_array_equal(plain["z"], out["z"])  # the option changes nothing of the chain
    # under a relabelling the values are those of the state as sampled, and z_map is a row of z_original
    for kw in (dict(relabel="ecr"), dict(relabel=True, stephens="device", burnrelabel=2)):
        rel = bmm.gibbs_collapsed(X, initial_K=z0, logpost=True, a=A, b=B, beta=0.7, gamma=1.9, **kw, **RUN)
        np.testing.assert_array_equal(rel["z_original"], out["z"])
        np.testing.assert_array_equal(_bits(_rows_of(rel["logpost"])), _bits(rows))
        np.testing.assert_array_equal(rel["logpost"]["z_map"], rel["z_original"][lp["best"]])


def test_equal_rows_keep_the_first_and_row_0_without_burn_in_is_nan_and_never_best(bmm):
    X, _ = _run_data()
    out = bmm.gibbs_collapsed(X, 8, 1, alpha=1.0, burnin=3, seed=4, logpost=True)
    lp = out["logpost"]
    assert len(set(_bits(lp["log_joint"]).tolist())) == 1 and lp["best"] == 0 and lp["n_used"] == 5
    out = bmm.gibbs_collapsed(X, 6, 1, alpha=1.0, burnin=0, seed=4, logpost=True)
    lp = out["logpost"]
    assert np.all(np.isnan(_rows_of(lp)[0])) and np.all(np.isfinite(_rows_of(lp)[1:]))
    assert lp["best"] == 1 and lp["n_used"] == 5
    np.testing.assert_array_equal(lp["z_map"], out["z"][1])
    for fn, kw in ((bmm.gibbs_dp, {}), (bmm.gibbs_stickbreaking, {"maxK": 5}), (bmm.gibbs_full, {"K": 4})):
        out = fn(X, 7, burnin=0, seed=4, logpost=True, **kw)
        lp = out["logpost"]
        assert np.isnan(lp["log_joint"][0]) and lp["best"] == 1 + int(np.argmax(lp["log_joint"][1:])) and lp["n_used"] == 6
        np.testing.assert_array_equal(lp["z_map"], out["z"][lp["best"]])


def test_an_armed_chain_keeps_the_best_state_and_samples_what_an_unarmed_one_does(bmm):
    X, z0 = _run_data()

    def make():
        c = bmm.Chain("collapsed", 300, 12, 4, alpha=None, beta=0.5, gamma=0.5, batch=50, seed=11)
        c.set_data(X)
        c.set_initial_labels(z0)
        return c
    with make() as plain, make() as idle, make() as folding:
        idle.set_logpost(True)
        folding.set_logpost(True)
        plain.sweeps(6)
        idle.sweeps(6)  # armed, not folding
        rows = np.vstack([folding.sweeps_logpost(2, trace=True), folding.sweeps_logpost(4, trace=True)])
        np.testing.assert_array_equal(plain.labels(), idle.labels())
        np.testing.assert_array_equal(plain.labels(), folding.labels())
        with pytest.raises(bmm.BmmError):
            idle.best()  # nothing folded
        best = folding.best()
        j = int(np.argmax(rows[:, 3]))
        assert best["sweep"] == j + 1 and _bits(best["log_joint"]) == _bits(rows[j, 3])
        with make() as twin:
            twin.sweeps(j + 1)
            np.testing.assert_array_equal(best["z_map"], twin.labels())
        folding.logpost_reset()
        folding.sweeps_logpost(1)
        assert folding.best()["sweep"] == 7
        np.testing.assert_array_equal(folding.best()["z_map"], folding.labels())


# ---------------------------------------------------------------- 4. the stand-alone call and pooled chains
def test_log_joint_on_a_runs_own_trace_reproduces_its_rows_bit_for_bit(bmm):
    X, z0 = _run_data()
    out = bmm.gibbs_collapsed(X, initial_K=z0, logpost=True, a=A, b=B, beta=0.7, gamma=1.9, **RUN)
    got = bmm.log_joint(X, out["z"], "collapsed", 4, out["alpha"].ravel(), 0.7, 1.9, A, B, sample_alpha=True)
    np.testing.assert_array_equal(_bits(_rows_of(got)), _bits(_rows_of(out["logpost"])))
    out = bmm.gibbs_dp(X, 9, alpha=1.5, burnin=2, seed=7, maxK=12, logpost=True, split_merge=1)
    got = bmm.log_joint(X, out["z"], "dp", 12, out["alpha"].ravel())
    np.testing.assert_array_equal(_bits(_rows_of(got)), _bits(_rows_of(out["logpost"])))
    out = bmm.gibbs_allocation(X, 9, 6, a=0.9, K0=2, burnin=2, seed=7, beta=0.5, gamma=0.8, logpost=True)
    got = bmm.log_joint(X, out["z"], "allocation", 6, 0.9, 0.5, 0.8, k_open=out["K"], prior_k="poisson")
    np.testing.assert_array_equal(_bits(_rows_of(got)), _bits(_rows_of(out["logpost"])))
    lp = out["logpost"]
    assert lp["best"] == int(np.argmax(lp["log_joint"]))
    np.testing.assert_array_equal(lp["z_map"], out["z"][lp["best"]])


def test_a_run_with_feature_selection_is_reproduced_from_its_masks(bmm):
    X, z0 = _run_data()
    out = bmm.gibbs_collapsed(X, initial_K=z0, logpost=True, select_features=True, rho=0.3, alpha=1.3, **RUN)
    got = bmm.log_joint(X, out["z"], "collapsed", 4, 1.3, mask=out["features"]["gamma"], rho=0.3)
    np.testing.assert_array_equal(_bits(_rows_of(got)), _bits(_rows_of(out["logpost"])))


def test_a_bad_label_is_named(bmm):
    X, _ = _run_data()
    z = np.ones((3, 300), dtype=np.int32)
    z[2, 17] = 5
    with pytest.raises(bmm.BmmError) as e:
        bmm.log_joint(X, z, "collapsed", 4)
    assert e.value.code == 1 and "z[2, 17] = 5" in str(e.value)


def test_two_chains_are_scored_pooled_and_relabelled_to_the_overall_best(bmm):
    X, _ = _run_data()
    outs = bmm.gibbs_collapsed(X, 24, 4, burnin=4, seed=3, chains=2, relabel="ecr", ecr_pivot="map")
    lps = [o["logpost"] for o in outs]
    top = lps[0]["chain"]
    assert lps[1]["chain"] == top and lps[0]["rhat"] == lps[1]["rhat"] and np.isfinite(lps[0]["rhat"])
    assert top == int(np.argmax([lp["log_joint"].max() for lp in lps]))
    for c, o in enumerate(outs):
        single = bmm.gibbs_collapsed(X, 24, 4, burnin=4, seed=3 + c, logpost=True,
                                     initial_K=np.random.default_rng(3 + c).integers(1, 5, 300))
        np.testing.assert_array_equal(single["z"], o["z_original"])
        np.testing.assert_array_equal(_bits(_rows_of(single["logpost"])), _bits(_rows_of(o["logpost"])))
        np.testing.assert_array_equal(o["ecr"]["pivot"], lps[top]["z_map"])
        np.testing.assert_array_equal(o["logpost"]["z_map"], o["z_original"][o["logpost"]["best"]])
    best = lps[top]["best"]
    np.testing.assert_array_equal(outs[top]["z"][best], lps[top]["z_map"])  # the pivot's own row keeps its labels
    assert outs[top]["ecr"]["agree"][best] == 300
