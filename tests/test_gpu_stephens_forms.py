"""Every form of the device Stephens kernels (k_st_*) against the NumPy restatement
(tests/stephens_ref.py).  Which form of a kernel runs depends on K, N and the number of slices M; the case tables
below are proven to reach every one of them by bm.stephens_plan, which reads the library's own launch arithmetic
(test_the_cases_reach_every_form fails if a threshold moves and a form drops out of the tables).

The assignment kernel is also run on cost matrices the test chooses bit for bit (stephens_ref.tie_inputs), so that
its tie rule -- the lowest column index wins, across the registers of a lane and across lanes -- is tested on
ties at the sizes where a lane holds two and three columns."""
import numpy as np
import pytest

import bmm_mcmc_amd as bm
import stephens_ref as sr

pytestmark = pytest.mark.gpu

EDGE_N = (1, 15, 16, 17, 63, 64, 65)

# (K, N, all-zero columns of p): the online step
ONLINE = (
    [(3, 300, ()), (4, 513, (2,)), (10, 1300, (9,)), (12, 2100, ()), (32, 1025, ()), (33, 1001, (7,)),
     (47, 700, ()), (61, 900, ()), (63, 650, ()), (64, 1100, (0, 63)), (65, 600, ()), (72, 2101, (0, 71)),
     (88, 777, ()), (89, 777, (88,)), (96, 1030, (5,)), (108, 515, ()), (109, 700, ()), (112, 300, ()),
     (127, 520, (64,)), (128, 1500, (127,)),
     (3, 600_001, (1,)),           # the cap of 1024 workgroups: 586 rows each, ten tiles per workgroup
     (128, 263_001, ())]           # the 64 MiB cap of the partials: 512 workgroups
    + [(5, n, ()) for n in EDGE_N] + [(33, n, ()) for n in EDGE_N])

# (K, N, M): the batch
BATCH = [(10, 300, 2), (33, 1501, 2), (64, 901, 2), (72, 701, 2), (96, 601, 2), (112, 603, 2), (128, 521, 2),
         (3, 200_003, 3),          # the per-slice cap ceil(1024 / 3) = 342 workgroups, 585 rows each
         (20, 500, 13)]            # M * K = 260: k_st_perm_identity on two blocks


def test_the_cases_reach_every_form():
    on = [(K, N, bm.stephens_plan(N, K)) for K, N, _ in ONLINE]
    ba = [(K, N, M, bm.stephens_plan(N, K, M)) for K, N, M in BATCH]
    plans = [p for *_, p in on] + [p for *_, p in ba]
    on_K = {K for K, _, _ in on}
    all_K = on_K | {K for K, *_ in ba}
    # blocks per thread: every instantiation of k_st_cost_partial, in the online and in the batch form
    assert {p["blocks_per_thread"] for *_, p in on} == {1, 2, 3, 4}
    assert {p["blocks_per_thread"] for *_, p in ba} == {1, 2, 3, 4}
    # tile height, and the two sides of its switch
    assert {p["tile_rows"] for p in plans} == {64, 16}
    assert bm.stephens_plan(100, 32)["tile_rows"] == 64 and bm.stephens_plan(100, 33)["tile_rows"] == 16
    assert {32, 33} <= on_K
    # thread-group shapes of the cost pass
    assert any(p["blocks"] == 1 for p in plans)
    assert any(9 <= K <= 12 and p["thread_groups"] > 1 and p["thread_groups"] * p["blocks"] < 256 for K, _, p in on)
    assert any(p["thread_groups"] == 1 and 128 < p["blocks"] < 256 for p in plans)
    assert any(K == 64 and p["blocks"] == 256 and p["thread_groups"] == 1 for K, _, p in on)
    assert any(p["thread_groups"] > 1 and p["thread_groups"] * p["blocks"] == 256 for p in plans)
    # the assignment: cost matrix in LDS / in global memory, one, two and three columns per lane
    assert {p["cost_in_lds"] for p in plans} == {0, 1}
    assert bm.stephens_plan(100, 88)["cost_in_lds"] == 1 and bm.stephens_plan(100, 89)["cost_in_lds"] == 0
    assert {88, 89} <= on_K
    assert {p["cols_per_lane"] for p in plans} == {1, 2, 3}
    assert {63, 64, 65, 127, 128} <= on_K
    assert [bm.stephens_plan(100, K)["cols_per_lane"] for K in (63, 64, 65, 127, 128)] == [1, 2, 2, 2, 3]
    # workgroup counts: one; fewer than the reduce has quarters; five; the caps
    G = {p["groups_online"] for *_, p in on}
    assert 1 in G and G & {2, 3} and 5 in G
    assert any(K == 3 and p["groups_online"] == 1024 and p["rows_online"] > 512 for K, _, p in on)
    assert any(M > 1 and p["groups_batch"] == -(-1024 // M) and p["rows_batch"] > 512 for _, _, M, p in ba)
    assert any(K == 128 and N > 262_144 and p["groups_online"] == (64 << 20) // (128 * 128 * 8) == 512
               and p["rows_online"] > 512 for K, N, p in on)
    assert any(M * K > 256 for K, _, M, _ in ba)
    # N below, at and above a tile on each side of the tile switch; a last workgroup with fewer rows
    for T in (64, 16):
        assert set(EDGE_N) <= {N for K, N, p in on if p["tile_rows"] == T}
    assert any(N % p["rows_online"] for _, N, p in on if p["groups_online"] > 1)
    assert any(N % p["rows_batch"] for _, N, _, p in ba if p["groups_batch"] > 1)
    assert {K % 4 for K in all_K} == {0, 1, 2, 3}


def _probs(rng, N, K, zero_cols=()):
    p = rng.dirichlet(np.full(K, 0.3), size=N)
    for l in zero_cols:
        p[:, l] = 0.0
    s = p.sum(axis=1, keepdims=True)
    return np.asfortranarray(np.where(s > 0, p / np.where(s > 0, s, 1), 0.0))


def _reference_cost(p, lq):
    """(cost, scale) of the online step.  Above 10^5 rows the restatement sums row blocks of 1024 in long double
    (long double throughout at K = 3), so that its own rounding stays below 1024 * 2^-53 = 1.2e-13 of the scale
    beside the 1e-12 the device is held to."""
    N, K = p.shape
    if N <= 100_000:
        return sr.cost(p, lq, False), sr.cost_scale(p, lq, False)
    return sr.cost_blocked(p, lq, False, block=1024, wide=K == 3), sr.cost_scale_blocked(p, lq, False, block=1024)


@pytest.mark.parametrize("K,N,zero_cols", ONLINE)
def test_online_step_matches_the_restatement(K, N, zero_cols):
    rng = np.random.default_rng(7000 + K * 1000 + N)
    p = _probs(rng, N, K, zero_cols)
    Q = np.asfortranarray(rng.random((N, K)) * 3 + 0.01)
    j = 17
    perm, Qn, C = bm.stephens_online(Q, p, j, with_cost=True)
    want_C, scale = _reference_cost(p, np.log(Q))
    ratio = np.abs(C - want_C) / (1e-12 * scale + 1e-300)
    print("K=%d N=%d: worst |C - C_ref| / (1e-12 scale) = %.3g" % (K, N, ratio.max()))
    assert np.all(np.abs(C - want_C) <= 1e-12 * scale + 1e-300)
    for l in zero_cols:
        assert (C[:, l] == 0).all()
    assert np.array_equal(perm, sr.hungarian(C))                  # the restatement on the device's own costs
    assert np.array_equal(Qn, (float(j) * (Q + p[:, perm])) / float(j + 1))
    perm2, Qn2, C2 = bm.stephens_online(Q, p, j, with_cost=True)
    assert np.array_equal(perm, perm2) and np.array_equal(Qn, Qn2) and np.array_equal(C, C2)


def batch_cube(K, N, M):
    """One labelling with its columns shuffled per slice (what label switching looks like) under 10 % noise, and a
    few exact zeros (the batch replaces them by 1e-6)."""
    rng = np.random.default_rng(9000 + K + N + M)
    base = _probs(rng, N, K)
    cube = np.empty((N, K, M), order="F")
    for m in range(M):
        cube[:, :, m] = base[:, rng.permutation(K)] * 0.9 + _probs(rng, N, K) * 0.1
    cube[:7, :, 0] = 0.0
    return cube


def batch_reference(cube):
    """The restatement's (Q, perm, iterations) and how far its assignments were from a tie: the smallest
    margin / cost scale over the slices of every iteration whose costs can differ from those of the iteration
    before (the first, and each one that starts from another permutation table) and of the last."""
    N, K, M = cube.shape
    pr = np.where(cube == 0, sr.MIN_PROB, cube)
    seen = {"margin": np.inf, "before": None, "checked": []}

    def on_iter(t, q, before, costs):
        if t < sr.MAXITER and seen["before"] is not None and np.array_equal(before, seen["before"]):
            return
        seen["before"] = before
        seen["checked"].append(t)
        lq = np.log(q)
        for m in range(M):
            scale = sr.cost_scale(pr[:, :, m], lq, True)
            seen["margin"] = min(seen["margin"], sr.margin_warm(costs[m]) / max(float(scale.max()), 1e-300))

    Q, perm, t = sr.batch(cube, on_iter=on_iter)
    return Q, perm, t, seen["margin"], seen["checked"]


@pytest.mark.parametrize("K,N,M", BATCH)
def test_batch_matches_the_restatement(K, N, M):
    cube = batch_cube(K, N, M)
    Q, perm = bm.stephens_batch(cube)
    want_Q, want_perm, t, margin, checked = batch_reference(cube)
    print("K=%d N=%d M=%d: margin / scale = %.3g at iterations %s" % (K, N, M, margin, checked))
    assert t == 100 and checked[0] == 1 and checked[-1] == 100
    assert margin >= 1e-9                                         # no comparison below is a rounding coin-flip
    assert np.array_equal(perm, want_perm)
    pr = np.where(cube == 0, 1e-6, cube)
    scale = np.abs(pr).sum(axis=2) / M
    assert np.all(np.abs(Q - want_Q) <= 1e-12 * scale)
    Q2, perm2 = bm.stephens_batch(cube)
    assert np.array_equal(Q, Q2) and np.array_equal(perm, perm2)


TIE_K = (2, 7, 63, 64, 65, 88, 89, 127, 128)


def _solve(D):
    """the device's (perm, cost) on the cost matrix that tie_inputs lays out for D, held to what that matrix is"""
    Q, p = sr.tie_inputs(D)
    perm, _, C = bm.stephens_online(Q, p, 3, with_cost=True)
    want_C = sr.cost(p, np.log(Q), False)
    assert np.all(np.abs(C - want_C) <= 1e-12 * sr.cost_scale(p, np.log(Q), False) + 1e-300)
    assert len(np.unique(C)) == len(np.unique(D))                 # equal entries of D: bit-equal costs
    for d in np.unique(D):
        assert len(np.unique(C[D == d])) == 1
    assert sorted(perm) == list(range(D.shape[0]))
    return perm, C


@pytest.mark.parametrize("K", TIE_K)
def test_assignment_on_heavy_ties(K):
    rng = np.random.default_rng(300 + K)
    for values in ((0, 1), (0, 1, 2, 3), (0, 3, 5)):
        D = rng.choice(values, size=(K, K)).astype(np.float64)
        perm, C = _solve(D)
        assert np.array_equal(perm, sr.hungarian(C)), values


@pytest.mark.parametrize("K", TIE_K)
def test_assignment_on_crafted_ties(K):
    """constant, cyclic and anti-diagonal costs, and (from K = 88) one row with equally cheap columns in two
    registers of a lane and in two lanes: the literal permutations of stephens_ref.crafted_ties"""
    cases = sr.crafted_ties(K)
    assert {"constant", "cyclic", "antidiagonal"} <= {name for name, _, _ in cases}
    if K >= 88:
        assert {"registers", "lanes"} <= {name for name, _, _ in cases}
    if K == 128:
        assert "registers3" in {name for name, _, _ in cases}
    for name, D, want in cases:
        perm, C = _solve(D)
        assert list(perm) == list(want), name
        assert np.array_equal(perm, sr.hungarian(C)), name
