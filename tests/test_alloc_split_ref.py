"""The split-merge move of the allocation sampler as defined (include/bmm_mcmc.h), on the CPU: the NumPy restatement
(tests/alloc_split_ref.py) is in detailed balance on the lumped state against the brute-force pi(K, rho), its own chain
passes the enumeration checks the device is held to (tests/test_gpu_alloc_split.py), and every GPU case's seed reaches
what the case is for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_checks as achk  # noqa: E402
import alloc_ref as al  # noqa: E402
import alloc_split_cases as cases  # noqa: E402
import alloc_split_ref as ref  # noqa: E402
import split_merge_checks as smchk  # noqa: E402
from test_alloc_ref import five_observations  # noqa: E402
from test_split_merge_ref import seven_observations  # noqa: E402

A = 0.7


@pytest.mark.parametrize("scans,prior,beta,gamma", [(0, "poisson", 0.5, 0.5), (1, "poisson", 0.5, 0.5), (0, "uniform", 0.5, 0.5),
                                                    (1, "uniform", 0.5, 0.5), (1, "poisson", 0.4, 1.1)])
def test_the_move_is_in_detailed_balance_on_the_lumped_state(scans, prior, beta, gamma):
    X, maxK = five_observations(), 3
    lp = al.poisson_prior(maxK) if prior == "poisson" else al.uniform_prior(maxK)
    states, T = ref.move_matrix(X, maxK, A, beta, gamma, lp, scans)
    assert len(states) == 276
    np.testing.assert_allclose(T.sum(1), 1.0, atol=1e-13)
    pi = al.target_vector(states, X, A, beta, gamma, lp)
    classes, pil, F, spread = al.lump(states, pi, T)
    assert len(classes) == 58
    # the lumped target by brute force, scipy's gammaln only: the labelled one summed over a class is the same thing
    want = ref.lumped_target(classes, X, A, beta, gamma, lp)
    np.testing.assert_allclose(pil, want, rtol=1e-12)
    flow = want[:, None] * (F / pil[:, None])
    off = ~np.eye(len(classes), dtype=bool)
    scale = np.maximum(flow, flow.T)
    rel = np.abs(flow - flow.T)[scale > 0] / scale[scale > 0]
    print("flows off the diagonal %d, largest relative imbalance %.3e, spread within a class %.3e"
          % (np.count_nonzero(flow[off]), rel.max(), spread))
    assert rel.max() <= 1e-12                       # detailed balance against pi(K, rho)
    assert spread <= 1e-12                          # the labellings of a class move alike
    assert np.count_nonzero(flow[off]) > 100        # the move goes places


@pytest.fixture(scope="module")
def seven():
    X = seven_observations().astype(np.int64)
    return X


@pytest.mark.parametrize("prior", ["poisson", "uniform"])
def test_the_restated_chain_with_both_moves_samples_the_enumeration(seven, prior):
    X, maxK = seven, 4
    lp = al.poisson_prior(maxK) if prior == "poisson" else al.uniform_prior(maxK)
    parts, w, pk = al.exact_posterior(X, maxK, cases.A7, cases.BETA, cases.GAMMA, lp)
    rng = np.random.default_rng(3)
    seen, st = ref.chain(X, np.zeros(7, dtype=np.int64), 1, maxK, cases.A7, cases.BETA, cases.GAMMA, 1.0, lp, 1, 20_000, rng)
    print(st)
    assert st["accepted_splits"] > 200 and st["accepted_merges"] > 200
    achk.check_k_posterior([K for K, _ in seen], pk)
    smchk.check_against_enumeration([p for _, p in seen], parts, w)


def test_the_restated_move_alone_samples_the_states_with_no_empty_component(seven):
    X, maxK = seven, 4
    lp = al.poisson_prior(maxK)
    parts, w, pk = ref.exact_posterior_no_empty(X, maxK, cases.A7, cases.BETA, cases.GAMMA, lp)
    rng = np.random.default_rng(4)
    seen, st = ref.chain(X, np.zeros(7, dtype=np.int64), 1, maxK, cases.A7, cases.BETA, cases.GAMMA, 1.0, lp, 1, 40_000, rng,
                         sweeps=False, ea_moves=0)
    print(st)
    assert all(K == max(p) + 1 for K, p in seen)  # the class is closed under the move
    assert st["accepted_splits"] > 500 and st["accepted_merges"] > 500
    achk.check_k_posterior([K for K, _ in seen], pk)
    smchk.check_against_enumeration([p for _, p in seen], parts, w)


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_every_gpu_case_reaches_what_it_is_for(name):
    case = cases.BY_NAME[name]
    cases.check_reached(case, cases.restated_steps(case))


def test_planted_components_are_found_by_the_restated_chain_for_all_ten_seeds():
    """fixes the data and the sweep budget of tests/test_gpu_alloc_split.py's planted test: ten of ten, each within half
    the budget"""
    from alloc_sweep_cases import planted
    N, comps = cases.PLANT_N, cases.PLANT_COMPS
    X, _ = planted(N, cases.PLANT_P, comps, 0, 1, 0, N, cases.PLANT_DATA_SEED)
    lp = al.poisson_prior(cases.PLANT_MAXK)
    arrivals = []
    for seed in cases.PLANT_SEEDS:
        used = ref.planted_chain(X, np.zeros(N, dtype=np.int64), 1, cases.PLANT_MAXK, 1.0, cases.BETA, cases.GAMMA, 1.0, lp,
                                 cases.PLANT_SCANS, cases.PLANT_SWEEPS, np.random.default_rng(seed))
        assert used[-1] == comps, (seed, used)
        arrivals.append(next(j + 1 for j in range(len(used)) if all(u == comps for u in used[j:])))
    print("arrives at sweep", arrivals)
    assert tuple(arrivals) == cases.PLANT_ARRIVALS and 2 * max(arrivals) <= cases.PLANT_SWEEPS
