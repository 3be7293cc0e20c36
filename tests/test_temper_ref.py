"""The restatement of parallel tempering (tests/temper_ref.py) held to what it must satisfy on its own, without a GPU:
the tempered scan leaves the tempered posterior invariant, the exchange leaves the product of two rungs' posteriors
invariant, scan and both parities of the exchange together leave the product of three rungs' posteriors invariant, at
b = 1 the conditional is the oracle's, the shapes and powers the device's exchange test uses make every pair both
accept and reject, and the inputs the device's swap, edge and replay tests choose hold what those tests need of them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_merge_ref as smr  # noqa: E402
import temper_ref as tr  # noqa: E402

BETA = GAMMA = 0.5
ALPHA = 1.3


def five_rows():
    return np.array([[1, 1, 0], [1, 0, 0], [0, 1, 1], [0, 0, 1], [1, 1, 1]], dtype=np.int32)


@pytest.fixture(scope="module")
def enumerated():
    X = five_rows()
    parts = smr.partitions(len(X))
    assert len(parts) == 52
    return X, parts


@pytest.mark.parametrize("b", [1.0, 0.5, 0.1])
def test_tempered_scan_leaves_the_tempered_posterior_invariant(enumerated, b):
    X, parts = enumerated
    pi, _ = tr.tempered_posterior(X, parts, ALPHA, BETA, GAMMA, b)
    T = tr.scan_matrix(X, parts, ALPHA, BETA, GAMMA, b, K=6)
    np.testing.assert_allclose(T.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    err = np.abs(pi @ T - pi).max()
    print("b = %g: worst |pi T - pi| = %.2e" % (b, err))
    assert err <= 1e-12
    if b != 1.0:  # and the check can tell: the untempered posterior is not invariant under the tempered scan
        pi1, _ = tr.tempered_posterior(X, parts, ALPHA, BETA, GAMMA, 1.0)
        assert np.abs(pi1 @ T - pi1).max() > 1e-4


@pytest.mark.parametrize("b", [0.5, 0.1])
def test_exchange_leaves_the_product_of_the_two_posteriors_invariant(enumerated, b):
    X, parts = enumerated
    pi1, L = tr.tempered_posterior(X, parts, ALPHA, BETA, GAMMA, 1.0)
    pib, _ = tr.tempered_posterior(X, parts, ALPHA, BETA, GAMMA, b)
    joint = np.outer(pi1, pib).reshape(-1)
    T = tr.exchange_matrix(L, 1.0, b)
    np.testing.assert_allclose(T.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    err = np.abs(joint @ T - joint).max()
    print("b = %g: worst |(pi_1 x pi_b) T - (pi_1 x pi_b)| = %.2e" % (b, err))
    assert err <= 1e-12
    other = np.outer(pib, pi1).reshape(-1)  # the rungs the wrong way round
    assert np.abs(other @ T - other).max() > 1e-6


def test_scan_then_both_parities_of_the_exchange_leave_the_product_of_three_posteriors_invariant(enumerated):
    """What a ladder of three does between two kept rows at swap_every = 1, twice over: every rung scans, then the
    even point proposes pair 0 or the odd point pair 1.  Composed -- scan, even point, odd point -- on the 52^3 joint
    states, without the matrix."""
    X, parts = enumerated
    powers = (1.0, 0.6, 0.3)
    pis, Ts = [], []
    for b in powers:
        pi, L = tr.tempered_posterior(X, parts, ALPHA, BETA, GAMMA, b)
        pis.append(pi)
        Ts.append(tr.scan_matrix(X, parts, ALPHA, BETA, GAMMA, b, K=6))
    joint = pis[0][:, None, None] * pis[1][None, :, None] * pis[2][None, None, :]
    after = tr.product_scan(joint, Ts)
    after = tr.product_exchange(after, L, powers, tr.proposed_pairs(3, 0))
    after = tr.product_exchange(after, L, powers, tr.proposed_pairs(3, 1))
    assert abs(after.sum() - 1.0) <= 1e-12
    err = np.abs(after - joint).max()
    print("worst |(pi_1 x pi_0.6 x pi_0.3) T - (pi_1 x pi_0.6 x pi_0.3)| = %.2e" % err)
    assert err <= 1e-12
    # the operator is exchange_matrix on two rungs ...
    two = np.outer(pis[0], pis[1])
    np.testing.assert_allclose(tr.product_exchange(two, L, powers, [0]).reshape(-1),
                               two.reshape(-1) @ tr.exchange_matrix(L, powers[0], powers[1]), rtol=0, atol=1e-15)
    # ... and the check can tell: a pair compared with the wrong rung's power, or the cold marginal under the wrong target
    wrong = tr.product_exchange(tr.product_exchange(tr.product_scan(joint, Ts), L, powers, [0]), L, (1.0, 0.3, 0.6), [1])
    assert np.abs(wrong - joint).max() > 1e-6
    other = pis[1][:, None, None] * pis[0][None, :, None] * pis[2][None, None, :]
    assert np.abs(tr.product_exchange(tr.product_scan(other, Ts), L, powers, [0]) - other).max() > 1e-6


@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
def test_at_power_one_the_conditional_is_the_oracles(oracle, sampler):
    N, P, K = 60, 7, 5
    X, _ = tr.mixture(N, P, [0.2, 0.5, 0.8], 5)
    rng = np.random.default_rng(1)
    z = rng.integers(0, K - 2, N)  # the last label unused: the DP's new cluster has a label to open
    z[3] = K - 2                   # ... and label K - 2 holds one row: emptied when that row is scored
    got = tr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, 1.0, sampler)
    worst = 0.0
    for i in range(N):
        fn = oracle.collapsed_cond if sampler == "collapsed" else oracle.dp_cond
        _, want = fn(X, (z + 1).astype(np.int32), i, K, ALPHA, BETA, GAMMA, spec=True)
        mine = got[i]
        if sampler == "dp":  # the oracle lists the K labels, then the new-cluster option; here it sits under the label it opens
            n = np.bincount(np.delete(z, i), minlength=K)
            free = np.flatnonzero(n == 0)[0]
            folded = np.array(want[:K])
            assert folded[free] == 0.0
            folded[free] = want[K]
            want = folded
        big = want > 1e-300
        worst = max(worst, float(np.max(np.abs(mine[big] - want[big]) / want[big])))
        assert np.all(mine[~big] <= 1e-300)
    print("%s: worst relative difference at b = 1: %.2e" % (sampler, worst))
    assert worst <= 1e-12


def test_a_power_below_one_flattens_the_conditional():
    X, _ = tr.mixture(60, 7, [0.2, 0.5, 0.8], 5)
    z = np.random.default_rng(1).integers(0, 4, 60)
    for sampler in ("collapsed", "dp"):
        cold = tr.z_conditional(X, z, 5, ALPHA, BETA, GAMMA, 1.0, sampler)
        warm = tr.z_conditional(X, z, 5, ALPHA, BETA, GAMMA, 0.3, sampler)
        assert np.abs(cold - warm).max() > 1e-3
        # at b -> 0 the prior weights alone are left
        flat = tr.z_conditional(X, z, 5, ALPHA, BETA, GAMMA, 1e-300, sampler)
        n = np.bincount(z, minlength=5).astype(np.float64)
        for i in (0, 7, 31):
            m = n.copy()
            m[z[i]] -= 1
            w = np.where(m > 0, m + (ALPHA / 5 if sampler == "collapsed" else 0.0), 0.0)
            if sampler == "dp":
                w[np.flatnonzero(m == 0)[0]] = ALPHA
            np.testing.assert_allclose(flat[i], w / w.sum(), rtol=1e-12, atol=0)


def test_exchange_rule_and_uniform(oracle):
    assert tr.accepts(0.0, 0.999) and tr.accepts(3.0, 0.999)
    assert not tr.accepts(float("nan"), 0.0)
    assert not tr.accepts(-np.inf, 0.0)
    assert tr.accepts(-1.0, 0.3) and not tr.accepts(-1.0, 0.4)  # exp(-1) = 0.3679
    us = np.array([[tr.exchange_uniform(77, r, t) for r in range(7)] for t in range(40)])
    assert np.all((us >= 0.0) & (us < 1.0)) and len(np.unique(us)) == us.size
    assert 0.35 < us.mean() < 0.65
    assert tr.exchange_uniform(77, 1, 2) != tr.exchange_uniform(77, 2, 1) != tr.exchange_uniform(78, 2, 1)
    assert tr.proposed_pairs(5, 0) == [0, 2] and tr.proposed_pairs(5, 1) == [1, 3] and tr.proposed_pairs(2, 1) == []


@pytest.mark.parametrize("R", sorted(tr.EXCHANGE_POWERS))
def test_the_device_tests_ladders_both_accept_and_reject(oracle, R):
    """The data and the powers of the device's exchange-decision test: the restated ladder, with the device's uniforms
    and its own sweeps, both accepts and rejects at least 10 proposals of every pair in the test's 60 steps (ladders of
    two and five; the ladders of four and eight are held to 3 on the device and clear it here with room: at least 7
    over three seeds of the restatement's own generator)."""
    N, P, K = tr.EXCHANGE_SHAPE
    X, _ = tr.mixture(N, P, tr.EXCHANGE_THETAS, tr.EXCHANGE_DATA_SEED)
    z0 = np.random.default_rng(11).integers(0, K, N)
    out = tr.restated_ladder(X, z0, K, ALPHA, BETA, GAMMA, tr.EXCHANGE_POWERS[R], tr.EXCHANGE_STEPS, seed=5)
    rejected = out["proposed"] - out["accepted"]
    print("R = %d: proposed %s accepted %s" % (R, out["proposed"], out["accepted"]))
    floor = tr.EXCHANGE_FLOOR[R]
    assert floor in (3, 10)
    assert np.all(out["accepted"] >= floor) and np.all(rejected >= floor)
    assert sorted(out["walker"]) == list(range(R))
    if floor == 3:  # "with room"
        for rs in (1, 2):
            more = tr.restated_ladder(X, z0, K, ALPHA, BETA, GAMMA, tr.EXCHANGE_POWERS[R], tr.EXCHANGE_STEPS, seed=5, rng_seed=rs)
            print("R = %d, generator %d: proposed %s accepted %s" % (R, rs, more["proposed"], more["accepted"]))
            assert np.all(more["accepted"] >= 2 * floor) and np.all(more["proposed"] - more["accepted"] >= 2 * floor)
        assert np.all(out["accepted"] >= 2 * floor) and np.all(rejected >= 2 * floor)


@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
def test_the_replayed_runs_ladder_exchanges_rung_0_often(oracle, sampler):
    """The run that tests/test_gpu_temper_ladders.py replays row by row must change walker_cold at least three times:
    the restated ladder of its shape, powers and ladder seed accepts rung 0's pair at least 6 times and rejects it too."""
    N, P, K = tr.REPLAY_SHAPE
    X, _ = tr.mixture(N, P, tr.REPLAY_THETAS, tr.REPLAY_DATA_SEED)
    z0 = np.random.default_rng(12).integers(0, K, N) if sampler == "collapsed" else np.full(N, -1)
    out = tr.restated_ladder(X, z0, K if sampler == "collapsed" else tr.REPLAY_MAXK, ALPHA, BETA, GAMMA, tr.REPLAY_POWERS[3],
                             tr.REPLAY_SWEEPS - 1, seed=tr.REPLAY_SEED, sampler=sampler, batch=tr.REPLAY_BATCH)
    print("%s: proposed %s accepted %s" % (sampler, out["proposed"], out["accepted"]))
    assert out["proposed"][0] == 20 and 6 <= out["accepted"][0] < 20
    for R in (4, 8):
        assert tr.REPLAY_POWERS[R][:3] == tr.REPLAY_POWERS[3] and np.all(np.diff(tr.REPLAY_POWERS[R]) < 0) and len(tr.REPLAY_POWERS[R]) == R


@pytest.mark.parametrize("N,P,K", tr.SWAP_SHAPES)
def test_the_swap_shapes_leave_the_first_trip_and_the_two_states_differ_in_every_tail(N, P, K):
    X, z_a, z_b = tr.swap_case(N, P, K)
    assert np.all(z_a != z_b) and z_a.min() >= 1 and z_b.max() <= K
    (Nk_a, S_a), (Nk_b, S_b) = (tr.fsr.counts(X, z - 1, K) for z in (z_a, z_b))
    assert Nk_a[K - 1] != Nk_b[K - 1] and S_a[K - 1, P - 1] != S_b[K - 1, P - 1]
    threads, reps = 256, 8                                   # kTemperThreads, kDeltaReps
    blocks = min(-(-N // (4 * threads)), 256)
    lanes = blocks * threads
    if N == 64:
        assert blocks == 1 and K % 4 == 1 and (K * P) % 4 == 1          # scalar tails of one
        assert (K * P) // 4 > lanes and (K * P * reps) // 4 > 10 * lanes  # S: a second pass, dS: eleven
        # the rejected twin: the hot rung holds z_b at a power of 2^-10 and its log_lik lies far enough below for any u
        d = tr.log_ratio(1.0, 2.0 ** -10, tr.log_lik(X, z_a - 1, BETA, GAMMA), tr.log_lik(X, z_b - 1, BETA, GAMMA))
        print("d of the rejected twin: %.1f" % d)
        assert d < -100.0
    else:
        assert blocks == 256 and N // 4 > lanes and N % 4 == 1           # a second pass and one label left over


def test_the_edge_case_holds_every_table_edge(oracle):
    N, P, K = tr.EDGE_SHAPE
    X, z = tr.edge_case()
    Nk, S = tr.fsr.counts(X, z, K)
    assert Nk[tr.EDGE_EMPTY] == 0 and Nk[tr.EDGE_SINGLE] == 1 and Nk[tr.EDGE_PAIR] == 2 and np.all(Nk[[0, 4, 5]] > 50)
    assert np.all(S[:, 0] == 0) and np.all(S[:, 1] == Nk)              # s = 0 and s = n in every label
    rows = list(tr.EDGE_ROWS["single"] + tr.EDGE_ROWS["pair"]) + [0, 1, 2]
    for b in (1.0, 0.3):
        fin = tr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, b, "collapsed", rows=rows)
        dp = tr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, b, "dp", rows=rows)
        assert np.all(fin[:, tr.EDGE_EMPTY] == 0.0)                     # the finite sampler never fills an empty label
        assert np.all(fin[0, [tr.EDGE_EMPTY, tr.EDGE_SINGLE]] == 0.0)   # nor the one its own row has just left
        assert np.all(dp[:, tr.EDGE_EMPTY] > 0.0)                       # the DP's new cluster opens the first free label
        assert dp[0, tr.EDGE_SINGLE] == 0.0
    for i in rows:  # and at b = 1 it is the oracle's conditional at those rows
        _, want = oracle.collapsed_cond(X, (z + 1).astype(np.int32), i, K, ALPHA, BETA, GAMMA, spec=True)
        got = tr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, 1.0, "collapsed", rows=[i])[0]
        np.testing.assert_allclose(got, np.array(want[:K]), rtol=1e-12, atol=1e-300)
