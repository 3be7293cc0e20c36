"""The allocation sampler's restatement (tests/alloc_ref.py) held to the model on the CPU: the exact transition matrices
of the eject / absorb move and of the sweep's row updates against the brute-force target, the host build of the spec's
closed-form log q, and that every GPU case's seed reaches what the case is for."""
import os
import sys

import numpy as np
import pytest
from scipy.special import betaln, gammaln

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_cases as cases  # noqa: E402
import alloc_checks as chk  # noqa: E402
import alloc_ref as ref  # noqa: E402
import split_merge_checks as smchk  # noqa: E402

A, BETA, GAMMA = 0.7, 0.5, 0.5


def five_observations():
    return np.array([[1, 1, 0], [1, 0, 0], [0, 1, 1], [0, 0, 1], [1, 1, 1]], dtype=np.int64)


@pytest.mark.parametrize("prior", ["poisson", "uniform"])
@pytest.mark.parametrize("e", [1.0, 2.5])
def test_the_move_is_in_detailed_balance_on_the_lumped_state(prior, e):
    X, maxK = five_observations(), 3
    lp = ref.poisson_prior(maxK) if prior == "poisson" else ref.uniform_prior(maxK)
    states, T = ref.move_matrix(X, maxK, A, BETA, GAMMA, e, lp)
    assert len(states) == 1 + 2 ** 5 + 3 ** 5
    np.testing.assert_allclose(T.sum(1), 1.0, atol=1e-13)
    pi = ref.target_vector(states, X, A, BETA, GAMMA, lp)
    classes, pil, F, spread = ref.lump(states, pi, T)
    # measured (Poisson, e = 1): flow asymmetry 2.8e-17, spread within a class 2.2e-16
    print("lumped classes %d: max |F - F'| %.3e, spread within a class %.3e" % (len(classes), np.abs(F - F.T).max(), spread))
    assert np.abs(F - F.T).max() <= 1e-12      # detailed balance of the lumped chain against the lumped target
    assert spread <= 1e-12                     # ... which is a chain: every labelling of a class moves alike
    np.testing.assert_allclose(F.sum(1), pil, atol=1e-13)
    # every K communicates, and an empty component is ejected and absorbed
    assert all(T[s, t] > 0 for s, (K, z) in enumerate(states) for t, (K2, z2) in enumerate(states) if K2 == K + 1 and z2 == z)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_the_batch_1_sweep_targets_the_model_at_every_fixed_K(K):
    """A systematic scan is not reversible as a whole; each row's update is (it is a Gibbs step), and then the sweep,
    their product in row order, leaves the target invariant.  Both are checked, on the labelled and the lumped state."""
    X = five_observations()
    lp = ref.uniform_prior(3)
    sweep = None
    for i in range(len(X)):
        states, Ti = ref.row_matrix(X, K, i, A, BETA, GAMMA)
        pi = ref.target_vector(states, X, A, BETA, GAMMA, lp)
        flow = pi[:, None] * Ti
        assert np.abs(flow - flow.T).max() <= 1e-12
        sweep = Ti if sweep is None else sweep @ Ti
    print("K=%d: max |pi T - pi| of one sweep %.3e" % (K, np.abs(pi @ sweep - pi).max()))
    assert np.abs(pi @ sweep - pi).max() <= 1e-12
    classes, pil, F, spread = ref.lump(states, pi, sweep)
    assert np.abs(F.sum(0) - pil).max() <= 1e-12 and spread <= 1e-12
    if K > 1:  # an emptied label is taken again: from "all rows under label 0" every label is reachable
        assert sweep[0].min() > 0.0


def test_exact_posterior_sums_the_labellings():
    X = five_observations()
    lp = ref.poisson_prior(3)
    parts, w, pk = ref.exact_posterior(X, 3, A, BETA, GAMMA, lp)
    states = ref.labelled_states(5, 3)
    pi = ref.target_vector(states, X, A, BETA, GAMMA, lp)
    for K in (1, 2, 3):
        assert pk[K] == pytest.approx(sum(p for (k, _), p in zip(states, pi) if k == K), abs=1e-13)
    assert w.sum() == pytest.approx(1.0, abs=1e-13)


def test_closed_form_log_q_on_the_host_build(tmp_path):
    exe = chk.build_host(tmp_path)
    triples = [(e, n1, n2) for e in (0.5, 1.0, 2.5) for n1 in (0, 1, 2, 7, 300, 10 ** 6) for n2 in (0, 1, 5, 299, 10 ** 6)]
    got = chk.host_logq(exe, tmp_path, triples)
    worst = 0.0
    for (e, n1, n2), (lg, lb, lq) in zip(triples, got):
        want = betaln(e + n1, e + n2) - betaln(e, e)
        # four lgamma_ terms and two more of the constant, each within LGAMMA_ULPS ulps of max(1, |term|), five additions
        mags = [abs(gammaln(e + n1)), abs(gammaln(e + n2)), abs(gammaln(2 * e + n1 + n2)), 2 * abs(gammaln(e)), abs(gammaln(2 * e))]
        bound = 2.0 * (smchk.LGAMMA_ULPS + 6) * smchk.EPS * (sum(mags) + 6)
        assert abs(lq - want) <= bound, (e, n1, n2, lq, want)
        assert abs(lg - gammaln(e + n1)) <= smchk.LGAMMA_ULPS * smchk.EPS * max(1.0, abs(gammaln(e + n1)))
        worst = max(worst, abs(lq - want) / bound)
    print("log q: worst error as a share of its bound %.3g" % worst)
    assert got[triples.index((1.0, 0, 0))][2] == 0.0  # ejecting an empty component proposes one outcome


def restated_steps(case, tmp_path):
    """the case's 40 moves by the restatement alone, p_E from the host build; also holds the restated integer draws to
    the host build's"""
    exe = chk.build_host(tmp_path)
    X, z1, lp = cases.start(case)
    z, K = z1.astype(np.int64) - 1, case.K0
    seen = []
    for m in range(cases.STEPS):
        h = chk.host_draws(exe, tmp_path, case.seed, 1, m, K, case.maxK, case.e)
        dr = ref.PhiloxDraws(case.seed, 1, m, pe=h["pe"])
        r = ref.move(X, z, K, case.maxK, case.a, BETA_, GAMMA_, case.e, lp, dr)
        assert (0 if r["kind"] == ref.EJECT else 1, r["labels"][0], r["labels"][1]) == (h["kind"], h["j1"], h["j2"])
        assert dr.salt == h["salt"] and r["log_u"] == pytest.approx(np.log(h["u"]), abs=1e-12)
        seen.append(r)
        z, K = r["z"], r["K"]
    return z1, seen


BETA_, GAMMA_ = cases.BETA, cases.GAMMA


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_every_gpu_case_reaches_what_it_is_for(name, tmp_path):
    case = cases.BY_NAME[name]
    z1, seen = restated_steps(case, tmp_path)
    cases.check_reached(case, z1, seen)


@pytest.mark.parametrize("P", cases.TIE_P)
@pytest.mark.parametrize("batch", [1, 64])
def test_tie_seed_keeps_every_label_occupied(oracle, batch, P):
    """tests/test_gpu_alloc.py ties the armed chain with K = maxK = 4, a = 1/4 to the collapsed chain at alpha = 1, which
    holds only while no label is empty or holds a single row: the oracle's collapsed chain shows that the seed keeps clear."""
    X, z0 = cases.tie_start(P)
    out = oracle.collapsed(X, z0, cases.TIE_SWEEPS + 1, 4, 1.0, cases.BETA, cases.GAMMA, 1.0, 1.0, 0, cases.TIE_SEED, batch=batch)
    sizes = np.array([np.bincount(row - 1, minlength=4) for row in out["z"]])
    print("smallest label over the sweeps:", sizes.min())
    assert sizes.min() > 1
