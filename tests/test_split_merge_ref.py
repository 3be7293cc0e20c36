"""The split-merge move as defined (include/bmm_mcmc.h), on the CPU: the NumPy restatement satisfies detailed balance
against the brute-force posterior exactly; the spec's lgamma_ against scipy; and the restatement's own chain passes the
enumeration check the device is held to (tests/test_gpu_split_merge.py)."""
import sys
import os

import numpy as np
import pytest
from scipy.special import gammaln

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_merge_checks as chk  # noqa: E402
import split_merge_ref as ref  # noqa: E402

BETA = GAMMA = 0.5
ALPHA = 1.3


def seven_observations():
    """the set of tests/test_oracle_posterior.py"""
    rng = np.random.default_rng(11)
    X = (rng.random((7, 3)) < [0.8, 0.3, 0.6]).astype(np.int32)
    X[:3, 0] = 1
    X[4:, 0] = 0
    return X


@pytest.mark.parametrize("scans", [0, 1])
def test_detailed_balance_of_the_definition_over_all_52_partitions(scans):
    rng = np.random.default_rng(5)
    X = (rng.random((5, 3)) < [0.7, 0.4, 0.5]).astype(np.int64)
    states, T = ref.transition_matrix(X, ALPHA, BETA, GAMMA, scans)
    assert len(states) == 52
    np.testing.assert_allclose(T.sum(axis=1), 1.0, rtol=1e-12)
    # the posterior by brute force: scipy's gammaln only, nothing of the reference module's likelihood code
    logw = []
    for z in states:
        z = np.asarray(z)
        lw = 0.0
        for k in range(z.max() + 1):
            rows = X[z == k]
            n, s = len(rows), rows.sum(axis=0)
            lw += np.log(ALPHA) + gammaln(n)
            lw += float(np.sum(gammaln(BETA + s) + gammaln(GAMMA + n - s) - gammaln(BETA + GAMMA + n)
                               + gammaln(BETA + GAMMA) - gammaln(BETA) - gammaln(GAMMA)))
        logw.append(lw)
    pi = np.exp(np.asarray(logw) - np.max(logw))
    pi /= pi.sum()
    flow = pi[:, None] * T
    off = ~np.eye(len(states), dtype=bool)
    assert np.count_nonzero(flow[off]) > 100  # the move does go places
    scale = np.maximum(flow, flow.T)
    rel = np.abs(flow - flow.T)[scale > 0] / scale[scale > 0]
    print("largest relative imbalance", rel.max())
    assert rel.max() <= 1e-12
    np.testing.assert_allclose(pi @ T, pi, rtol=1e-11)


def test_lgamma_of_the_spec_on_the_host_against_scipy(tmp_path):
    exe = chk.build_lgamma_host(tmp_path)
    x = chk.lgamma_arguments()
    assert x.min() == 0.01 and x.max() >= 1e7 + 1
    got = chk.lgamma_host(exe, x, tmp_path)
    err = chk.lgamma_error_ulps(got, x)
    k = int(np.argmax(err))
    print("largest lgamma_ error: %.2f ulps of max(1, |lgamma|) at x = %r" % (err[k], x[k]))
    assert err[k] <= chk.LGAMMA_ULPS


def test_reference_chain_of_moves_samples_the_exact_posterior():
    X = seven_observations()
    parts, w = chk.exact_posterior(X, ALPHA, BETA, GAMMA)
    assert len(parts) == 877
    visited = ref.chain(X, np.zeros(7, dtype=int), 30, ALPHA, BETA, GAMMA, 2, 50_000, np.random.default_rng(3))
    chk.check_against_enumeration(visited, parts, w)


def test_philox_streams_of_the_restatement_match_the_known_answers():
    # Random123 kat_vectors (as tests/test_oracle_numerics.py pins the oracle's)
    assert ref.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    a, b = ref.philox2x32_10(np.array([0x243f6a88], dtype=np.uint64), 0x85a308d3, 0x13198a2e)
    assert (int(a[0]), int(b[0])) == (0xdd7ce038, 0xf62a4c12)
