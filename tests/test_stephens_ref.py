"""The NumPy restatement of Stephens' relabelling (tests/stephens_ref.py) pinned on its own, without a GPU:
the assignment against brute force, the tie rule, and each quirk of src/stephens.cpp as it executes."""
import numpy as np
import pytest

import stephens_ref as sr


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7])
def test_hungarian_equals_brute_force(K):
    rng = np.random.default_rng(100 + K)
    for _ in range(40):
        C = rng.normal(size=(K, K))
        perm = sr.hungarian(C)
        best, arg = sr.brute_force(C)
        assert sorted(perm) == list(range(K))
        assert np.isclose(sum(C[perm[l], l] for l in range(K)), best, rtol=0, atol=1e-12)
        assert tuple(perm) in arg


def test_integer_costs_with_ties_stay_optimal():
    rng = np.random.default_rng(7)
    for K in (3, 5, 6):
        for _ in range(30):
            C = rng.integers(0, 3, size=(K, K)).astype(float)
            perm = sr.hungarian(C)
            best, arg = sr.brute_force(C)
            assert tuple(perm) in arg


def test_zero_columns_resolve_by_the_tie_rule():
    # an all-zero column of p costs exactly 0 against every row, whatever log q is (even -inf)
    N, K = 50, 4
    rng = np.random.default_rng(3)
    p = rng.random((N, K))
    p[:, 1] = 0.0
    p[:, 3] = 0.0
    Q = rng.random((N, K)) + 0.1
    Q[0, 2] = 0.0                                    # log q = -inf on a row where only zero columns ...
    p[0, :] = 0.0                                    # ... of p meet it
    p[0, 0] = 1.0
    Q[0, 0] = 0.5
    with np.errstate(divide="ignore"):
        C = sr.cost(p, np.log(Q), False)
    assert (C[:, 1] == 0).all() and (C[:, 3] == 0).all()
    # all-zero cost: every permutation ties; the lowest index wins every scan -> the identity
    assert list(sr.hungarian(np.zeros((5, 5)))) == [0, 1, 2, 3, 4]
    # two zero columns among non-zero ones: the lower-index zero column takes the lower free row
    C = np.array([[0.0, 5.0, 0.0], [0.0, 1.0, 0.0], [0.0, 9.0, 0.0]])
    assert list(sr.hungarian(C)) == [0, 1, 2]


def test_batch_runs_exactly_maxiter_and_returns_the_q_of_the_last_iterations_start():
    rng = np.random.default_rng(11)
    N, K, M = 40, 3, 4
    p = rng.dirichlet(np.ones(K), size=(N, M)).transpose(0, 2, 1)   # N x K x M, rows sum to 1
    seen = []
    q, perm, t = sr.batch(p, on_iter=lambda t, q, before, costs: seen.append((q.copy(), before.copy())))
    assert t == sr.MAXITER == 100 and len(seen) == 100      # 10^(-6) == -16: the criterion never stops it
    assert float(10 ^ (-6)) == -16.0
    q_last, perm_before_last = seen[-1]
    assert np.array_equal(q, q_last)
    # Q is the mean over slices of p[:, perm(iter, k), iter] with the permutations *before* the last solve
    want = np.zeros((N, K))
    for it in range(M):
        want += p[:, perm_before_last[it], it]
    assert np.array_equal(q, want / M)


def test_zeros_of_the_window_become_1e_6_before_q_is_built():
    N, K, M = 6, 2, 2
    p = np.zeros((N, K, M))
    p[:, 0, 0] = 1.0
    seen = []
    sr.batch(p, maxiter=1, on_iter=lambda t, q, before, costs: seen.append(q))
    q = seen[0]
    assert np.array_equal(q[:, 0], np.full(N, (1.0 + 1e-6) / 2))
    assert np.array_equal(q[:, 1], np.full(N, (1e-6 + 1e-6) / 2))


def test_k3_cycle_reorders_p_by_the_uninverted_perm():
    # cost minimised by assigning row k to column sigma(k) = (k + 1) % 3: perm[l] = row of column l = (l - 1) % 3
    N, K = 3, 3
    Q = np.full((N, K), 1.0)
    p = np.zeros((N, K))
    # make C[k, l] = -sum_n p(n,l) log q(n,k) + const small exactly on the cycle k -> k + 1
    Q[:, 0] = np.exp([0.0, 3.0, 0.0])
    Q[:, 1] = np.exp([0.0, 0.0, 3.0])
    Q[:, 2] = np.exp([3.0, 0.0, 0.0])
    p[0, 0], p[1, 1], p[2, 2] = 1.0, 1.0, 1.0           # column l lives on row n = l
    perm, Qn, C = sr.online(Q, p, 5)
    # column l's mass sits on row l; log q(l, k) = 3 for k = (l - 1) % 3 -> row (l - 1) % 3 takes column l
    assert list(perm) == [2, 0, 1]
    inverse = np.argsort(perm)
    assert list(inverse) == [1, 2, 0] and list(inverse) != list(perm)   # not an involution
    # p_reordered.col(k) = p.col(perm(k)) (stephens.cpp:88), with perm as solved -- not its inverse
    assert np.array_equal(Qn, (5.0 * (Q + p[:, [2, 0, 1]])) / 6.0)
    assert not np.array_equal(Qn, (5.0 * (Q + p[:, inverse])) / 6.0)


def test_online_q_after_n_steps_matches_the_closed_form():
    rng = np.random.default_rng(5)
    N, K = 30, 4
    Q0 = rng.random((N, K)) + 0.05
    Q = Q0.copy()
    want = Q0.copy()
    for j in range(7, 12):
        p = rng.dirichlet(np.ones(K), size=N)
        perm, Q, _ = sr.online(Q, p, j)
        want = (float(j) * (want + p[:, perm])) / float(j + 1)     # add, multiply, divide, in that order
        assert np.array_equal(Q, want)
    # not a running mean (which would stay near 1 / K): every step adds a row of p, Q keeps growing
    assert Q.mean() > Q0.mean() + 0.5


def test_online_cost_uses_p_not_log_p():
    rng = np.random.default_rng(9)
    N, K = 20, 3
    p = rng.dirichlet(np.ones(K), size=N)
    Q = rng.random((N, K)) + 0.1
    C = sr.cost(p, np.log(Q), False)
    for k in range(K):
        for l in range(K):
            assert np.isclose(C[k, l], np.sum(p[:, l] * (p[:, l] - np.log(Q[:, k]))), rtol=1e-14, atol=0)
    Cb = sr.cost(p, np.log(Q), True)
    assert np.isclose(Cb[1, 2], np.sum(p[:, 2] * (np.log(p[:, 2]) - np.log(Q[:, 1]))), rtol=1e-14, atol=0)


# ---- the restatement at the sizes the device tests trust it at (tests/test_gpu_stephens_forms.py) -----------

def _total(C, perm):
    return sum(C[perm[l], l] for l in range(C.shape[0]))


@pytest.mark.parametrize("K", [8, 33, 64, 65, 89, 128])
def test_hungarian_reaches_the_optimum_at_the_sizes_of_the_device_tests(K):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(500 + K)
    mats = [rng.normal(size=(K, K)), rng.random((K, K)) * 50, rng.integers(0, 3, size=(K, K)).astype(float),
            rng.integers(0, 4, size=(K, K)).astype(float), rng.choice([0.0, 3.0, 5.0], size=(K, K))]
    for C in mats:
        perm = sr.hungarian(C)
        assert sorted(perm) == list(range(K))
        rows, cols = lsa(C)
        # rounding of a K-term sum only
        assert abs(_total(C, perm) - C[rows, cols].sum()) <= 1e-12 * K * np.abs(C).max()


def test_hungarian_equals_brute_force_at_8():
    rng = np.random.default_rng(108)
    for C in (rng.normal(size=(8, 8)), rng.integers(0, 3, size=(8, 8)).astype(float)):
        perm = sr.hungarian(C)
        best, arg = sr.brute_force(C)
        assert abs(_total(C, perm) - best) <= 1e-12 * 8 * np.abs(C).max()
        assert tuple(perm) in arg


@pytest.mark.parametrize("K", [2, 7, 63, 64, 65, 88, 89, 127, 128])
def test_tie_inputs_lay_the_chosen_ties_under_the_assignment(K):
    rng = np.random.default_rng(300 + K)
    D = rng.choice([0, 1, 2, 3], size=(K, K)).astype(np.float64)
    Q, p = sr.tie_inputs(D)
    lq = np.log(Q)
    t = sr.terms(p, lq, False)                                    # t[k, n, l]
    off = ~np.eye(K, dtype=bool)
    assert (t[:, off] == 0).all() and not np.signbit(t[:, off]).any()   # terms of n != l: exact +0.0
    C = sr.cost(p, lq, False)
    assert np.array_equal(C, 1.0 - np.log(np.exp2(D)))
    vals = np.unique(D)
    assert len(np.unique(C)) == len(vals)
    for d in vals:
        assert len(np.unique(C[D == d])) == 1                     # equal entries of D: bit-equal costs
    assert all(C[D == a][0] > C[D == b][0] for a, b in zip(vals, vals[1:]))   # a larger D is cheaper
    if K >= 63:
        lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
        perm = sr.hungarian(C)
        rows, cols = lsa(C)
        assert abs(_total(C, perm) - C[rows, cols].sum()) <= 1e-12 * K * np.abs(C).max()


@pytest.mark.parametrize("K", [2, 7, 63, 64, 65, 88, 89, 127, 128])
def test_the_tie_rule_on_crafted_costs(K):
    """the literal permutations of crafted_ties, written out here once more where they are short to state"""
    cases = {name: (D, want) for name, D, want in sr.crafted_ties(K)}
    for name, (D, want) in cases.items():
        Q, p = sr.tie_inputs(D)
        C = sr.cost(p, np.log(Q), False)
        assert list(sr.hungarian(C)) == list(want), name
    assert list(cases["constant"][1]) == list(range(K))
    assert list(cases["cyclic"][1]) == [K - 1] + list(range(K - 1))
    assert list(cases["antidiagonal"][1]) == list(range(K - 1, -1, -1))
    assert ("registers" in cases) == (K >= 88) == ("lanes" in cases)
    if K >= 88:
        # the last row is equally cheap in columns 3 and 67 / 70 and 9: the lower column takes it, that
        # column's row moves to the free column K - 1
        swap = lambda a, b: [b if l == a else a if l == b else l for l in range(K)]
        D, want = cases["registers"]
        assert D[K - 1, 3] == D[K - 1, 67] == 1 and D.sum() == 2 and list(want) == swap(3, K - 1)
        D, want = cases["lanes"]
        assert D[K - 1, 9] == D[K - 1, 70] == 1 and D.sum() == 2 and list(want) == swap(9, K - 1)
        if K == 128:
            D, want = cases["registers3"]
            assert D[126, 63] == D[126, 127] == 1 and D.sum() == 2 and list(want) == swap(63, 126)


def test_margin_warm_equals_margin():
    rng = np.random.default_rng(77)
    for K in (1, 2, 3, 5, 8, 20, 33):
        for C in (rng.normal(size=(K, K)), rng.random((K, K)), rng.integers(0, 4, size=(K, K)).astype(float)):
            perm = sr.hungarian(C)
            a, b = sr.margin(C, perm), sr.margin_warm(C, perm)
            assert (np.isinf(a) and np.isinf(b)) or abs(a - b) <= 1e-12 * K * max(np.abs(C).max(), 1.0)
    C = np.zeros((4, 4))
    C[0, 1] = 1.0
    with pytest.raises(ValueError):
        sr.margin_warm(C, np.array([1, 0, 2, 3], dtype=np.int32))     # not the restatement's assignment


def test_blocked_cost_equals_cost():
    rng = np.random.default_rng(13)
    N, K = 5000, 3
    p = rng.dirichlet(np.ones(K), size=N)
    p[:, 1] = 0.0
    lq = np.log(rng.random((N, K)) * 3 + 0.01)
    for batch_form in (False, True):
        C = sr.cost(p, lq, batch_form)
        scale = sr.cost_scale(p, lq, batch_form)
        for got in (sr.cost_blocked(p, lq, batch_form, block=1024), sr.cost_blocked(p, lq, batch_form, wide=True)):
            assert np.all(np.abs(got - C) <= N * 2.0 ** -53 * scale) and (got[:, 1] == 0).all()
        assert np.allclose(sr.cost_scale_blocked(p, lq, batch_form, block=1024), scale, rtol=1e-13, atol=0)
