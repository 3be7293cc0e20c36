"""Missing data by augmentation, on the CPU: the host statement of the imputation step (tests/na/na_host.cpp, over
bmm_spec.h) against the NumPy restatement (tests/na_ref.py), the joint it draws from, and the target of the chain.
The GPU tests (tests/test_gpu_missing.py) hold the device to the host program bit for bit and to the same targets."""
import os
import sys
from math import comb

import numpy as np
from scipy.special import betaln

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import na_ref as ref  # noqa: E402
import split_merge_checks as checks  # noqa: E402

BETA = GAMMA = 0.5


def seven_observations():
    """the data of tests/test_oracle_posterior.py"""
    rng = np.random.default_rng(11)
    X = (rng.random((7, 3)) < [0.8, 0.3, 0.6]).astype(np.int32)
    X[:3, 0] = 1
    X[4:, 0] = 0
    return X


def seven_missing():
    """4 cells declared missing, row 2 loses two"""
    obs = np.ones((7, 3), dtype=bool)
    for i, j in [(0, 1), (2, 0), (2, 2), (5, 1)]:
        obs[i, j] = False
    return obs


def _case(N, P, K, frac, seed):
    rng = np.random.default_rng(seed)
    X = (rng.random((N, P)) < 0.4).astype(np.int32)
    z = rng.integers(0, K, N)
    z[rng.random(N) < 0.1] = -1 if N > 4 else z[0]
    mis = rng.random((N, P)) < frac
    mis[N // 2] = True  # a row with every cell missing
    rows, cols = np.nonzero(mis)
    return X, z, rows, cols


def test_host_step_is_the_restatement():
    """site masks, census, observed-only Beta parameters, the uniforms' keys, bits, S deltas and the recount invariant"""
    seed, sweep = 0x1234567890ABCDEF, 7
    for N, P, K in [(9, 31, 3), (12, 33, 4), (5, 65, 2), (1, 5, 2)]:
        X, z, rows, cols = _case(N, P, K, 0.3, N * 100 + P)
        Nk, S = ref.recount(X, z, K)
        h = ref.host_step(X, z, Nk, S, rows, cols, seed, sweep, BETA, GAMMA)
        assert h["sites"] == ref.sites(rows, cols)
        for row, w, mask, first in h["sites"]:
            assert 0 < mask < 2 ** 32 and all(w * 32 + b < P for b in range(32) if mask >> b & 1)
        M, O = ref.census(X, z, rows, cols, K)
        assert sorted(h["cnt"]) == [int(kj) for kj in np.flatnonzero(M.ravel() > 0)]
        phi = np.zeros((K, P))
        for kj, (m, o, s, n, a, b, ph) in h["cnt"].items():
            k, j = divmod(kj, P)
            seated_obs = (z == k)
            n_obs = int(seated_obs.sum()) - int(M[k, j])
            s_obs = int(S[k, j]) - int(O[k, j])
            assert (m, o, s, n) == (M[k, j], O[k, j], s_obs, n_obs)
            assert a == BETA + s_obs and b == GAMMA + n_obs - s_obs and 0.0 < ph < 1.0
            # the observed-only counts are those of a recount that never looks at a missing cell
            mis_col = np.zeros(N, dtype=bool)
            mis_col[rows[cols == j]] = True
            assert n_obs == int((seated_obs & ~mis_col).sum()) and s_obs == int(X[seated_obs & ~mis_col, j].sum())
            phi[k, j] = ph
        X1, S1, bits, u = ref.step_given_phi(X, z, S, rows, cols, phi, seed, sweep)
        seated = z[rows] >= 0
        assert np.array_equal(h["u"][seated], u[seated])  # the keys: cell identity and sweep, nothing else
        assert np.array_equal(h["bits"][0], bits) and np.array_equal(h["X"], X1) and np.array_equal(h["S"], S1)
        assert np.array_equal(ref.recount(h["X"], z, K)[1], h["S"])
        assert np.array_equal(h["sum"][seated], h["phi_cell"][seated]) and np.array_equal(h["ones"], bits * seated)
        # the starting fill: sweep 0, the prior mean
        f = ref.host_step(X, z, Nk, S, rows, cols, seed, 99, BETA, GAMMA, mode=0)
        want = np.array([ref.na_uniform(seed, int(i) * P + int(j), 0) < BETA / (BETA + GAMMA) for i, j in zip(rows, cols)])
        assert np.array_equal(f["bits"][0], want.astype(np.uint8))
        assert np.array_equal(ref.recount(f["X"], z, K)[1], f["S"])


def test_uniform_does_not_depend_on_the_order_of_the_cell_list():
    """a cell's uniform is keyed by (i * P + j, sweep): declaring fewer cells changes no other cell's draw"""
    X, z, rows, cols = _case(12, 33, 3, 0.3, 5)
    z[:] = np.abs(z)
    Nk, S = ref.recount(X, z, 3)
    theta = np.random.default_rng(1).random((3, 33))
    full = ref.host_step(X, z, Nk, S, rows, cols, 77, 3, BETA, GAMMA, theta=theta)
    keep = np.arange(len(rows)) % 2 == 0
    half = ref.host_step(X, z, Nk, S, rows[keep], cols[keep], 77, 3, BETA, GAMMA, theta=theta)
    assert np.array_equal(full["u"][keep], half["u"]) and np.array_equal(full["bits"][0][keep], half["bits"][0])


def test_the_joint_of_the_cells_of_one_label_and_feature_is_the_urns():
    """One label, one feature, 3 observed rows of which 2 hold a 1, 3 missing cells, 20 000 steps of the host program:
    the number of ones follows the beta-binomial within 4 standard errors per cell, and the plug-in binomial does not."""
    n, s, m_cells, sweeps = 3, 2, 3, 20_000
    X = np.array([[1], [1], [0], [0], [0], [0]], dtype=np.int32)
    z = np.zeros(6, dtype=np.int64)
    rows, cols = np.array([3, 4, 5]), np.array([0, 0, 0])
    Nk, S = ref.recount(X, z, 1)
    h = ref.host_step(X, z, Nk, S, rows, cols, 2024, 1, BETA, GAMMA, reps=sweeps)
    got = np.bincount(h["bits"].sum(axis=1), minlength=m_cells + 1) / sweeps
    a, b = BETA + s, GAMMA + n - s
    urn = np.array([comb(m_cells, m) * np.exp(betaln(a + m, b + m_cells - m) - betaln(a, b)) for m in range(m_cells + 1)])
    p = a / (a + b)
    plug = np.array([comb(m_cells, m) * p ** m * (1 - p) ** (m_cells - m) for m in range(m_cells + 1)])
    se = np.sqrt(urn * (1 - urn) / sweeps)
    print("ones  ", got, "\nurn   ", urn, "\nplug-in", plug, "\n4 se  ", 4 * se)
    assert np.all(np.abs(got - urn) <= 4 * se), (got, urn)
    assert np.any(np.abs(got - plug) > 4 * se), (got, plug)


def test_the_restatements_chain_samples_the_posterior_given_the_observed_cells():
    """the seven observations with 4 cells missing: all 877 partitions weighted by the CRP prior times the observed-cell
    marginal likelihood, against 30 000 sweeps of the literal conditional plus the imputation step"""
    X, obs = seven_observations(), seven_missing()
    parts, w = ref.exact_dp_posterior(X, obs, 1.3, BETA, GAMMA)
    assert len(parts) == 877
    visited = ref.dp_chain(X, obs, 1.3, BETA, GAMMA, 30_000, seed=3)
    worst = checks.check_against_enumeration(visited, parts, w)
    print("worst deviation / standard error %.2f" % worst)
    # and the target differs from the one that takes the zero-filled cells as observed: the case can tell them apart
    _, w0 = checks.exact_posterior(np.where(obs, X, 0), 1.3, BETA, GAMMA)
    assert np.abs(w - w0).max() > 0.004
