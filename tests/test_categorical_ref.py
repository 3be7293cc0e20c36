"""The NumPy restatement of categorical features (tests/categorical_ref.py) against itself, against the Bernoulli
restatement and against the enumeration: what the GPU tests (tests/test_gpu_categorical.py) take as their reference."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref as cr  # noqa: E402
import feature_select_ref as fsr  # noqa: E402
import split_merge_checks as chk  # noqa: E402
import split_merge_ref as smr  # noqa: E402

ALPHA, BETA = 1.3, 0.5
SWEEPS = 30_001  # the length of the GPU test


def test_expand_and_column_map_against_hand_derived_values():
    first, lev = cr.column_map([3, 1, 2, 4])
    np.testing.assert_array_equal(first, [0, 3, 4, 6])
    np.testing.assert_array_equal(lev, [3, 3, 3, 0, 2, 2, 4, 4, 4, 4])
    X, lev2 = cr.expand([[2, 1, 0, 3], [0, 0, 1, 1]], [3, 1, 2, 4])
    np.testing.assert_array_equal(lev2, lev)
    np.testing.assert_array_equal(X, [[0, 0, 1, 1, 1, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 1, 0, 1, 0, 0]])
    assert X.dtype == np.int32 and X.flags.f_contiguous


def test_blocks_of_two_are_the_bernoulli_restatement_with_gamma_equal_beta():
    """Dirichlet(beta, beta) over (x = 0, x = 1) is Beta(beta, beta) on x: the one-hot pair of a binary column gives the
    conditional of that column alone, for both samplers, seated and unseated rows, to rounding"""
    rng = np.random.default_rng(4)
    N, P, K = 200, 9, 4
    Xb = (rng.random((N, P)) < rng.random(P)).astype(np.int64)
    X2, lev = cr.expand(Xb, [2] * P)  # value 1 -> the second column of the pair
    z = rng.integers(0, 3, N)  # (label 3 is empty)
    z[rng.random(N) < 0.1] = -1
    for sampler in ("collapsed", "dp"):
        want = fsr.z_conditional(Xb, z, K, ALPHA, BETA, BETA, np.ones(P, dtype=np.uint8), sampler)
        got = cr.z_conditional(X2, z, K, ALPHA, BETA, BETA, lev, sampler)
        assert np.abs(got - want).max() <= 1e-13
    # ... and no block at all is the Bernoulli restatement whatever gamma is
    for sampler in ("collapsed", "dp"):
        want = fsr.z_conditional(Xb, z, K, ALPHA, BETA, 0.8, np.ones(P, dtype=np.uint8), sampler)
        got = cr.z_conditional(Xb, z, K, ALPHA, BETA, 0.8, np.zeros(P, dtype=np.uint8), sampler)
        assert np.abs(got - want).max() <= 1e-13


def test_conditional_is_the_ratio_of_enumerated_joints():
    """z_conditional of the DP against exact_posterior's weights: moving one row between the partitions it can reach"""
    Xc, levels = cr.seven_rows()
    X1h, lev = cr.expand(Xc, levels)
    parts, w = cr.exact_posterior(Xc, levels, ALPHA, BETA)
    index = {s: k for k, s in enumerate(parts)}
    rng = np.random.default_rng(1)
    for _ in range(30):
        z = np.array(parts[rng.integers(len(parts))])
        i = int(rng.integers(7))
        cond = cr.z_conditional(X1h, z, 8, ALPHA, BETA, BETA, lev, "dp", rows=[i])[0]
        reach = {}
        for k in np.flatnonzero(cond > 0):
            z2 = z.copy()
            z2[i] = k
            reach[index[smr.canon(z2)]] = cond[k]
        tot = sum(w[s] for s in reach)
        for s, p in reach.items():
            assert abs(p - w[s] / tot) <= 1e-12


def test_the_two_models_differ_on_the_seven_rows_by_far_more_than_the_checks_margin():
    Xc, levels = cr.seven_rows()
    X1h, _ = cr.expand(Xc, levels)
    parts, w = cr.exact_posterior(Xc, levels, ALPHA, BETA)
    parts_b, wb = chk.exact_posterior(X1h, ALPHA, BETA, BETA)
    assert parts == parts_b and len(parts) == 877
    F, exact = cr.compared_quantities(parts, w)
    _, exact_b = cr.compared_quantities(parts, wb)
    # an independent sample of the GPU test's length has a margin of at most 4 sqrt(1 / (4 n)); a chain's is wider, but
    # not tenfold
    assert np.abs(exact - exact_b).max() > 10 * 4.0 * np.sqrt(0.25 / (SWEEPS - 1))


def test_sequential_sampler_passes_the_enumeration_check_at_the_gpu_tests_length():
    """the check of tests/test_gpu_categorical.py is one that a correct sampler of that length passes, and one that tells
    the Bernoulli posterior of the same columns from the categorical one"""
    Xc, levels = cr.seven_rows()
    X1h, _ = cr.expand(Xc, levels)
    parts, w = cr.exact_posterior(Xc, levels, ALPHA, BETA)
    visited = cr.sequential_dp(Xc, levels, ALPHA, BETA, BETA, SWEEPS, np.random.default_rng(3))[1:]
    chk.check_against_enumeration(visited, parts, w)
    F, exact = cr.compared_quantities(parts, w)
    _, exact_b = cr.compared_quantities(parts, chk.exact_posterior(X1h, ALPHA, BETA, BETA)[1])
    assert (np.abs(exact - exact_b) > cr.margins(visited, parts, F, exact)).any()
