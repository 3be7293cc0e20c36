"""Constrained allocations on the CPU (include/bmm_mcmc.h "constraints"): the restatement
(tests/constrain_ref.py) against the oracle's own chains where nothing is listed, its properties where rows are, the
exactness of the constrained row update by enumeration on a 7-row data set -- finite K = 3 and the DP -- and the bound
the device's enumeration test (tests/test_gpu_constrain.py) is held to, validated here on the restatement's move."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constrain_ref as ref  # noqa: E402

BETA = GAMMA = 0.5


def _data(N, P, seed, comps=(0.15, 0.5, 0.85)):
    rng = np.random.default_rng(seed)
    comp = rng.integers(len(comps), size=N)
    return np.asfortranarray((rng.random((N, P)) < np.asarray(comps)[comp][:, None]).astype(np.int32)), comp


NONE = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64))


# ---------------------------------------------------------------- 1. with nothing listed the restatement is the oracle chain
@pytest.mark.parametrize("sampler,batch", [("collapsed", 7), ("collapsed", 50), ("dp", 7), ("dp", 50)])
def test_unlisted_restatement_is_the_oracle_chain(oracle, sampler, batch):
    """labels and the sampled concentration, bit for bit, over three sweeps: the draw rule, the DP's label rule, the
    batch schedule (the DP's first sweep included) and the concentration's update are the oracle's"""
    N, P, K, S, seed = 50, 9, 4 if sampler == "collapsed" else 8, 4, 17
    X, _ = _data(N, P, 3)
    z0 = np.random.default_rng(1).integers(1, K + 1, N).astype(np.int32)
    if sampler == "collapsed":
        want = oracle.collapsed(X, z0, S, K, 0.0, BETA, GAMMA, 1, 1, 0, seed=seed, batch=batch)
        z = z0
    else:
        want = oracle.dp(X, S, 0.0, BETA, GAMMA, 1, 1, 0, K, seed=seed, batch=batch)
        z = np.zeros(N, dtype=np.int32)
    alpha, stats = 1.0, [0, 0]
    for j in range(1, S):
        z = ref.sweep(oracle, sampler, X, z, j, K, alpha, BETA, GAMMA, seed, batch, *NONE, stats)
        alpha = ref.sweep_alpha(oracle, sampler, alpha, 1, 1, N, K, z, seed, j)
        assert np.array_equal(z, want["z"][j]), j
        assert alpha == want["alpha"][j, 0], j
    assert stats == [0, 0]


def test_unlisted_restatement_is_the_oracle_chain_explicit(oracle):
    """one exact batch from (pi, theta): the first sweep of the stick-breaking oracle chain"""
    N, P, K, seed = 40, 9, 4, 5
    X, _ = _data(N, P, 4)
    rng = np.random.default_rng(2)
    pi0, th0 = rng.dirichlet(np.ones(K)), np.asfortranarray(0.05 + 0.9 * rng.random((K, P)))
    want = oracle.stickbreaking(X, pi0, th0, 2, K, 1.0, BETA, GAMMA, 1, 1, 0, seed=seed)
    z = ref.sweep(oracle, "stickbreaking", X, np.zeros(N, dtype=np.int32), 1, K, 1.0, BETA, GAMMA, seed, N, *NONE, [0, 0],
                  pi=pi0, theta=th0)
    assert np.array_equal(z, want["z"][1])


# ---------------------------------------------------------------- 2. properties of the restatement where rows are listed
@pytest.mark.parametrize("sampler", ["collapsed", "dp", "full"])
def test_listed_rows_never_leave_their_sets(oracle, sampler):
    N, P, K, sweeps, seed, batch = 60, 9, 4, 4, 23, 16
    X, comp = _data(N, P, 6)
    rng = np.random.default_rng(8)
    known = np.where(rng.random(N) < 0.3, comp + 1, 0)
    A = np.ones((N, K), dtype=bool)
    if sampler != "dp":  # partial sets on a few of the free rows
        for i in np.flatnonzero(known == 0)[:10]:
            A[i, rng.integers(K)] = False
    for i in np.flatnonzero(known):
        A[i] = False
        A[i, known[i] - 1] = True
    rows, masks = ref.set_list(A)
    assert len(rows) > len(np.flatnonzero(known)) or sampler == "dp"
    z = ref.project_start(rng.integers(1, K + 1, N), rows, masks) if sampler == "collapsed" else np.zeros(N, dtype=np.int32)
    if sampler == "collapsed":
        assert all(z[i] in ref.allowed_labels(m) for i, m in zip(rows, masks))
    stats = [0, 0]
    pi, th = rng.dirichlet(np.ones(K)), np.asfortranarray(0.05 + 0.9 * rng.random((K, P)))
    for j in range(1, sweeps + 1):
        before = stats[1]
        z2 = ref.sweep(oracle, sampler, X, z, j, K, 1.3, BETA, GAMMA, seed, batch, rows, masks, stats, pi=pi, theta=th)
        for i, m in zip(rows, masks):
            assert z2[i] in ref.allowed_labels(m), (j, i)
        if j > 1 or sampler == "collapsed":
            held = np.flatnonzero(known)
            assert np.array_equal(z2[held], z[held]) and np.array_equal(z2[held], known[held])  # known rows never move
        assert stats[1] - before <= len(rows)
        z = z2
    assert stats[0] == len(rows) * sweeps and 0 < stats[1] <= stats[0]


def test_projection_rule():
    rows, masks = np.array([0, 2, 3]), np.array([0b0100, 0b1010, 0b1011], dtype=np.uint64)
    # row 0: singleton {3}; row 2: {2, 4}, label 3 -> (3 - 1) mod 2 = 0-th = 2; row 3: {1, 2, 4}, label 3 -> 2 mod 3 = 2nd = 4
    assert ref.project_start([1, 1, 3, 3, 2], rows, masks).tolist() == [3, 1, 2, 4, 2]
    assert ref.project_start([3, 4, 4, 2, 1], rows, masks).tolist() == [3, 4, 4, 2, 1]  # allowed labels stay


# ---------------------------------------------------------------- 3. the move is exact: enumeration on the 7-row set
ALPHA = 1.3


def test_finite_constrained_update_is_exact():
    """K = 3, rows 0 and 1 known, row 2 with a two-label set: the posterior restricted to the constraints is stationary
    for every row's update and each update is reversible with respect to it (detailed balance), to 1e-12"""
    X, K = ref.seven_rows(), 3
    rows, masks = ref.seven_lists(K)
    assert rows.tolist() == [0, 1, 2] and [bin(int(m)).count("1") for m in masks] == [1, 1, 2]
    states = ref.finite_states(K, rows, masks)
    assert len(states) == 2 * 3 ** 4
    pi = ref.restricted(states, lambda z: ref.finite_log_target(X, z, K, ALPHA, BETA, GAMMA))
    allowed = {int(i): [k - 1 for k in ref.allowed_labels(m)] for i, m in zip(rows, masks)}
    sweep_T = np.eye(len(states))
    for i in range(7):
        T = ref.constrained_row_matrix(states, lambda z, r: ref.finite_conditional(X, z, r, K, ALPHA, BETA, GAMMA), i, allowed.get(i))
        np.testing.assert_allclose(T.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert np.abs(pi @ T - pi).max() < 1e-12, i
        F = pi[:, None] * T
        assert np.abs(F - F.T).max() < 1e-12, i
        if i in (0, 1):
            assert np.array_equal(T != 0, np.eye(len(states)) != 0)  # a known row never moves
        sweep_T = sweep_T @ T
    assert np.abs(pi @ sweep_T - pi).max() < 1e-12
    # ... and the chain it drives is irreducible on the restricted space: the sweep's matrix has one stationary vector
    w, v = np.linalg.eig(sweep_T.T)
    assert (np.abs(w - 1.0) < 1e-9).sum() == 1


def test_dp_constrained_update_is_exact():
    """the DP over the partitions consistent with the known labels: rows 0 and 1 in different blocks for ever, row 2 in
    the block of one of them; the CRP posterior restricted to them is stationary and every row's update reversible"""
    X = ref.seven_rows()
    states = [p for p in ref.partitions(7) if ref.dp_consistent(p)]
    assert len(ref.partitions(7)) == 877 and 0 < len(states) < 877
    pi = ref.restricted(states, lambda p: ref.dp_log_target(X, p, ALPHA, BETA, GAMMA))
    sweep_T = np.eye(len(states))
    for i in range(7):
        T = ref.dp_row_matrix(X, states, i, ALPHA, BETA, GAMMA)
        np.testing.assert_allclose(T.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert np.abs(pi @ T - pi).max() < 1e-12, i
        F = pi[:, None] * T
        assert np.abs(F - F.T).max() < 1e-12, i
        sweep_T = sweep_T @ T
    w, _ = np.linalg.eig(sweep_T.T)
    assert (np.abs(w - 1.0) < 1e-9).sum() == 1


# ---------------------------------------------------------------- 4. the bound of the device's enumeration test
ENUM_SWEEPS = 30_001  # the chain length of the enumeration tests in tests/test_gpu_missing.py


def enum_bound(pi, n=ENUM_SWEEPS - 1):
    """The total-variation distance between the exact distribution pi and the visit frequencies of n draws.  For n
    independent draws cell i deviates by about N(0, p_i (1 - p_i) / n), so E TV = 1/2 sum_i sqrt(2 p_i (1 - p_i) /
    (pi n)).  The bound is four times that: a factor 2 for the chain's autocorrelation (an integrated autocorrelation
    time up to 4 sweeps; the 7-row chain redraws every free row from its full conditional in every sweep) and a factor
    2 for the fluctuation of TV around its mean.  Nothing of the code under test enters."""
    return 4.0 * 0.5 * float(np.sum(np.sqrt(2.0 * pi * (1.0 - pi) / (np.pi * n))))


def finite_enum_case():
    """(K, rows, masks, states, pi, codes of the states base K) of the finite 7-row case"""
    X, K = ref.seven_rows(), 3
    rows, masks = ref.seven_lists(K)
    states = ref.finite_states(K, rows, masks)
    pi = ref.restricted(states, lambda z: ref.finite_log_target(X, z, K, ALPHA, BETA, GAMMA))
    codes = np.array([int(np.dot(z, K ** np.arange(6, -1, -1))) for z in states])
    return X, K, rows, masks, states, pi, codes


def tv_of_codes(visited, codes, pi):
    index = {int(c): k for k, c in enumerate(codes)}
    emp = np.bincount([index[int(c)] for c in visited], minlength=len(codes)) / len(visited)  # (a KeyError: outside the sets)
    return 0.5 * float(np.abs(emp - pi).sum())


def test_enumeration_bound_holds_on_the_restated_move():
    """eight chains of the restatement's move (exact conditionals, NumPy uniforms, batch 1): the largest deviation from
    the restricted posterior is at most half the bound the device chain is held to"""
    X, K, rows, masks, states, pi, codes = finite_enum_case()
    pw = K ** np.arange(6, -1, -1)
    table = []
    for i in range(7):
        t = {}
        for z in np.ndindex(*([K] * 7)):
            if z[i] == 0:
                t[int(np.dot(z, pw))] = np.cumsum(ref.finite_conditional(X, z, i, K, ALPHA, BETA, GAMMA))
        table.append(t)
    bound = enum_bound(pi)
    worst = 0.0
    for seed in range(8):
        rng = np.random.default_rng(100 + seed)
        z0 = states[rng.integers(len(states))]
        visited = ref.literal_chain(table, K, rows, masks, z0, ENUM_SWEEPS - 1, rng)
        worst = max(worst, tv_of_codes(visited, codes, pi))
    print("bound %.4f, worst of 8 seeds %.4f" % (bound, worst))
    assert worst <= 0.5 * bound, (worst, bound)  # measured: see the print (DESIGN.md section 25 records it)
