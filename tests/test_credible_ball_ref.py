"""The restatement of the credible ball (tests/credible_ball_ref.py) against hand-written answers and against the
identities of include/bmm_mcmc.h "credible ball", in Python integers.  No device."""
import numpy as np
import pytest

import credible_ball_ref as cbr
import partition_ref as pr
import partition_search_ref as psr


def _three(b):
    return [(b[q]["sweep"], b[q]["ties"], b[q]["n_clusters"]) for q in ("horizontal", "upper", "lower")]


def test_level_one_takes_every_draw():
    D, k = [4, 0, 9, 2, 7], [3, 2, 4, 2, 3]
    b = cbr.ball(D, k, 1.0)
    assert (b["m"], b["at"], b["radius"], b["n_in"]) == (5, 2, 9, 5)
    # farthest: draw 2; fewest clusters (2): draws 1 and 3, the farther is 3; most (4): draw 2
    assert _three(b) == [(2, 1, 4), (3, 1, 2), (2, 1, 4)]


def test_smallest_level_gives_radius_zero_at_a_visited_centre():
    D, k = [4, 0, 9, 2, 7], [3, 2, 4, 2, 3]  # draw 1 is the centre itself
    b = cbr.ball(D, k, 1e-9)
    assert (b["m"], b["at"], b["radius"], b["n_in"]) == (1, 1, 0, 1)
    assert _three(b) == [(1, 1, 2)] * 3


def test_duplicate_draws_tie_at_the_radius_and_are_all_inside():
    D, k = [5, 1, 5, 3, 5, 8], [2, 2, 3, 2, 3, 4]
    b = cbr.ball(D, k, 0.5)  # m = 3: the order is 1, 3, 0, 2, 4, 5, the third is draw 0
    assert (b["m"], b["at"], b["radius"], b["n_in"]) == (3, 0, 5, 5)
    assert b["n_in"] > b["m"]
    # horizontal: 0, 2, 4 at the radius; upper (k = 2: draws 0, 1, 3): draw 0; lower (k = 3: draws 2, 4): draw 2
    assert _three(b) == [(0, 3, 2), (0, 1, 2), (2, 2, 3)]


def test_ties_in_k_and_in_distance_go_to_the_lowest_sweep():
    D, k = [6.5, 6.5, 2.0, 6.5, 2.0, 1.0], [3, 5, 3, 5, 5, 4]
    b = cbr.ball(D, k, 1.0)
    assert (b["radius"], b["n_in"]) == (6.5, 6)
    assert _three(b) == [(0, 3, 3), (0, 1, 3), (1, 2, 5)]


def test_upper_and_lower_coincide_when_every_draw_has_one_k():
    D, k = [3, 1, 3, 2, 9], [4, 4, 4, 4, 2]
    b = cbr.ball(D, k, 0.8)  # m = 4: draw 4, the only one with another k, stays outside
    assert (b["m"], b["radius"], b["n_in"]) == (4, 3, 4)
    assert _three(b) == [(0, 2, 4)] * 3


def test_m_follows_the_definition():
    for S, level, m in ((10, 0.95, 10), (200, 0.95, 190), (7, 0.5, 4), (3, 1e-12, 1), (1, 0.3, 1)):
        assert cbr.ball(list(range(S)), [1] * S, level)["m"] == m


TRACES = [(3, 5, 41, 9, 11), (6, 6, 64, 12, 12), (4, 7, 33, 5, 13)]  # (Kc, Ka, N, S, seed)


@pytest.mark.parametrize("case", TRACES, ids=lambda c: "Kc%d-Ka%d-N%d-S%d-s%d" % c)
def test_sim_is_the_similarity_matrix_summed_over_each_cluster(case):
    Kc, Ka, N, S, seed = case
    z, truth = psr.make_trace(Kc, N, S, 0.3, seed)
    c = truth
    s = cbr.sim(c, z, Ka)
    cnt = pr.similarity(z, np.arange(N))
    for i in range(N):
        for a in range(Ka):
            assert int(s[i, a]) == sum(int(cnt[i, j]) for j in range(N) if c[j] == a + 1)


@pytest.mark.parametrize("case", TRACES, ids=lambda c: "Kc%d-Ka%d-N%d-S%d-s%d" % c)
def test_own_cluster_sims_add_up_to_the_agreeing_pairs(case):
    """sum_i sim[i][c_i] = sum_t sum_ab T_t[a][b]^2 = (S sum_a n_a^2 + sum_t sum_b n_tb^2 - sum_t d2_t) / 2"""
    Kc, Ka, N, S, seed = case
    z, truth = psr.make_trace(Kc, N, S, 0.3, seed)
    c = np.asarray(truth)
    s = cbr.sim(c, z, Ka)
    d2, _, _ = cbr.distances(c, z, max(Kc, Ka), "binder")
    lhs = sum(int(s[i, c[i] - 1]) for i in range(N))
    na = sum(int(v) ** 2 for v in np.bincount(c))
    nt = sum(int(v) ** 2 for row in z for v in np.bincount(row))
    twice = S * na + nt - sum(d2)
    assert twice % 2 == 0 and lhs == twice // 2


def test_distances_of_a_visited_centre():
    z, _ = psr.make_trace(4, 50, 6, 0.3, 5)
    for crit in ("binder", "vi"):
        d2, D, k = cbr.distances(z[2], z, 4, crit)
        assert d2[2] == 0 and D[2] == 0
        assert all(kk == len(set(row)) for kk, row in zip(k, z))
        assert [v == 0 for v in d2] == [v == 0 for v in D]


def test_membership_leaves_the_row_out_and_marks_what_is_undefined():
    z = np.array([[1, 1, 2, 2, 3], [1, 1, 1, 2, 3]])
    c = np.array([1, 1, 2, 2, 3])
    s = cbr.sim(c, z, 4)
    m = cbr.membership(s, c, 2)
    assert m[0, 0] == 1.0 and m[2, 0] == 0.5 and m[2, 1] == 0.5
    assert np.isnan(m[4, 2]) and np.isnan(m[:, 3]).all()  # alone in its cluster; an empty slot
