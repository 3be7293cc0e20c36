"""The NumPy restatement of the partition summaries (tests/partition_ref.py) against the definitions themselves:
Binder's distance as a count over all pairs, VI from the entropies, and Dahl's least-squares identity in exact
integers.  No library, no device."""
import numpy as np
import pytest

import partition_ref as ref


def _inputs():
    rng = np.random.default_rng(5)
    out = []
    for N, Kc in ((1, 1), (2, 2), (17, 3), (40, 5), (33, 1), (25, 8)):
        out.append((rng.integers(1, Kc + 1, N), rng.integers(1, Kc + 1, N), Kc))
    N = 30
    out.append((np.ones(N, dtype=int), rng.integers(1, 5, N), 4))             # one cluster
    out.append((np.arange(1, N + 1), rng.integers(1, 5, N), N))               # N singletons
    out.append((np.arange(1, N + 1), np.ones(N, dtype=int), N))               # the two extremes
    out.append((rng.integers(1, 3, N), rng.integers(4, 7, N), 9))             # labels unused in one row
    out.append((rng.integers(1, 4, N),) * 2 + (3,))                           # a row against itself
    return out


@pytest.mark.parametrize("c,z,Kc", _inputs())
def test_binder_is_the_count_of_disagreeing_pairs(c, z, Kc):
    assert ref.binder2(c, z, Kc) % 2 == 0
    assert ref.binder(c, z, Kc) == ref.binder_brute(c, z)
    assert ref.binder(z, c, Kc) == ref.binder(c, z, Kc)


@pytest.mark.parametrize("c,z,Kc", _inputs())
def test_vi_is_the_entropy_form(c, z, Kc):
    assert abs(ref.vi(c, z, Kc) - ref.vi_from_entropies(c, z)) <= 1e-12
    assert ref.vi(c, z, Kc) == ref.vi(z, c, Kc) or abs(ref.vi(c, z, Kc) - ref.vi(z, c, Kc)) <= 1e-15


def test_a_relabelled_row_is_the_same_partition():
    rng = np.random.default_rng(6)
    z = rng.integers(1, 6, 50)
    perm = rng.permutation(5) + 1
    assert ref.binder(z, perm[z - 1], 5) == 0 and ref.vi(z, perm[z - 1], 5) == 0.0


@pytest.mark.parametrize("S,N,Kc", [(1, 9, 2), (5, 24, 3), (12, 31, 6)])
def test_dahl_identity_exactly(S, N, Kc):
    """sum_{i<j} (S delta_ij - cnt_ij)^2 = S sum_t B(c, z_t) + sum_{i<j} cnt_ij^2 - S sum_{i<j} cnt_ij"""
    z = ref.make_rows(Kc, N, S, False, 100 + S)
    cnt = ref.similarity(z, np.arange(N))
    assert np.array_equal(cnt, cnt.T) and np.all(np.diag(cnt) == S)
    iu = np.triu_indices(N, 1)
    up = [int(x) for x in cnt[iu]]
    tot = ref.binder2_totals(z, Kc)
    for c in range(S):
        assert ref.dahl_least_squares(z[c], cnt, S) == S * (tot[c] // 2) + sum(x * x for x in up) - S * sum(up)
    # hence both criteria name the same row
    ls = [ref.dahl_least_squares(z[c], cnt, S) for c in range(S)]
    assert min(range(S), key=lambda i: (ls[i], i)) == ref.point_estimate(z, Kc)


def test_point_estimate_ties_go_to_the_lowest_row_and_stride_selects_candidates():
    rng = np.random.default_rng(8)
    a, b = rng.integers(1, 4, 20), rng.integers(1, 4, 20)
    z = np.stack([a, b, a, b])
    assert ref.point_estimate(z, 3) == 0 and ref.point_estimate(z, 3, "vi") == 0
    assert ref.candidates(7, 3) == [0, 3, 6] and ref.candidates(7, 7) == [0]
    z = np.stack([b, b, a, a, a])
    assert ref.point_estimate(z, 3) == 2 and ref.point_estimate(z, 3, stride=3) == 3
