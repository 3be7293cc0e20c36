"""The pairwise local-dependence check without a GPU: the hypergeometric reference the statistic
rests on, by enumeration; the host statement (bmm_spec.h) against the NumPy restatement; calibration and power of the
restatement on planted dependence; the wrappers' refusals and the pair numbering."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_check_host as host  # noqa: E402
import pair_check_ref as ref  # noqa: E402

import bmm_mcmc_amd as bm  # noqa: E402
from bmm_mcmc_amd import _capi  # noqa: E402


# ---- 1. the reference distribution, by enumeration
def test_hypergeometric_moments_by_enumeration():
    """N = 6, P = 3, every allocation into 2 labels: over all data sets with the per-label margins of a drawn X, the
    restatement's a_k = c_k - E_k has mean 0 and mean square v_k, per label, to 1e-12"""
    N, P, feat = 6, 3, np.arange(3)
    rng = np.random.default_rng(5)
    worst = 0.0
    for bits in range(1 << N):
        z0 = np.array([(bits >> i) & 1 for i in range(N)])
        X = rng.integers(0, 2, (N, P))
        _, s, n = ref.counts(X, z0, 2, feat)
        rows = [np.nonzero(z0 == k)[0] for k in range(2)]
        # every placement of the ones of features 0 and 1 inside each label; feature 2 stays as drawn
        per_label = [list(itertools.product(itertools.combinations(rows[k], int(s[k, 0])), itertools.combinations(rows[k], int(s[k, 1]))))
                     for k in range(2)]
        a_all, v_ref = [], None
        for choice in itertools.product(*per_label):
            Y = X.copy()
            Y[:, :2] = 0
            for k in range(2):
                Y[list(choice[k][0]), 0] = 1
                Y[list(choice[k][1]), 1] = 1
            c, s2, n2 = ref.counts(Y, z0, 2, feat)
            assert np.array_equal(s2, s) and np.array_equal(n2, n)
            a, v = ref.terms(c, s2, n2)
            a_all.append(a[:, 0])  # pair (0, 1)
            v_ref = v[:, 0]
        a_all = np.array(a_all)
        worst = max(worst, float(np.abs(a_all.mean(axis=0)).max()), float(np.abs((a_all ** 2).mean(axis=0) - v_ref).max()))
    print("enumeration: largest deviation of the mean and the variance %.3e" % worst)
    assert worst <= 1e-12


# ---- 2. the host statement against the restatement
def _state(rng, N, P, K, M, spread=True, constant=False, lone=False):
    X = rng.integers(0, 2, (N, P))
    if constant:
        X[:, 0] = 1
    z0 = rng.integers(0, K, N) if spread else rng.integers(0, min(K, 2), N)
    if lone and K >= 2 and N >= 3:
        z0[z0 == K - 1] = 0
        z0[0] = K - 1  # a label of one row
    feat = rng.permutation(P)[:M]
    if constant:
        feat[0] = 0
        feat[1:] = rng.permutation(np.arange(1, P))[:M - 1]
    return ref.counts(X, z0, K, feat)


@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 32, 33, 65])
def test_host_against_restatement(K):
    rng = np.random.default_rng(100 + K)
    for spread, constant, lone in ((True, False, False), (False, False, False), (True, True, False), (True, False, True)):
        c, s, n = _state(rng, 300, 12, K, 7, spread, constant, lone)
        got = host.run(c, s, n)
        host.check(got, c, s, n, "K=%d spread=%s constant=%s lone=%s" % (K, spread, constant, lone))
        if constant:  # V = 0 for the labels' terms with the constant feature: df drops, and with every label so, no Z
            assert np.all(got["df"][:6] == 0) and np.all(np.isnan(got["z"][:6]))
        if not spread and K > 2:
            assert np.count_nonzero(n) <= 2  # empty labels
        if lone and K >= 2:
            assert n[K - 1] == 1


def test_host_all_rows_in_one_label():
    rng = np.random.default_rng(7)
    X = rng.integers(0, 2, (200, 6))
    c, s, n = ref.counts(X, np.full(200, 3), 5, np.arange(6))
    got = host.run(c, s, n)
    host.check(got, c, s, n, "one label")
    assert np.all(got["df"] == 1)


def test_host_c5_scale_integers():
    """n = 1e7 rows in all: c n and s_d s_e reach 1e13 and pd pe 1e27; the int64 products and their single conversion"""
    rng = np.random.default_rng(11)
    K, M = 5, 6
    n = rng.multinomial(10_000_000, rng.dirichlet(np.ones(K)))
    s = rng.binomial(n[:, None], rng.uniform(0.1, 0.9, (K, M)))
    i, j = ref.pairs(M)
    c = rng.hypergeometric(s[:, i], n[:, None] - s[:, i], s[:, j])
    got = host.run(c, s, n)
    host.check(got, c, s, n, "C5 scale")
    assert np.abs(got["z"]).max() < 6.0  # drawn from the reference distribution itself


# ---- 3. calibration and power, the restatement alone
def test_planted_dependence_restatement():
    X, z0 = ref.planted(ref.PLANTED_SEED)
    st = ref.stats(X, z0, 3, np.arange(37))
    ref.check_planted(st["z"], st["x2"])


# ---- 4. the wrappers' refusals and the pair numbering
def test_pair_numbering():
    for M in (2, 3, 9, 128):
        p = bm.pair_check_pairs(M)
        i, j = np.triu_indices(M, 1)
        assert p.shape == (M * (M - 1) // 2, 2) and np.array_equal(p[:, 0], i) and np.array_equal(p[:, 1], j)
    # the host statement's order is that order: counts that name their pair come back in place
    M, K = 9, 2
    i, j = ref.pairs(M)
    n = np.array([1000, 1000])
    s = np.full((K, M), 500)
    c = np.stack([250 + np.arange(i.size), np.full(i.size, 250)])
    got = host.run(c, s, n)
    want = ref.stats_from_counts(c, s, n)
    assert np.array_equal(np.argsort(got["A"]), np.argsort(want["A"])) and np.all(np.diff(got["A"]) > 0)


def test_wrapper_refusals():
    X = np.zeros((10, 130), dtype=np.int32)
    with pytest.raises(ValueError, match="list of feature"):
        bm.gibbs_collapsed(X, 5, 2, pair_check=True)
    with pytest.raises(ValueError, match="per chain"):
        bm.gibbs_collapsed(X[:, :5], 5, 2, pair_check=True, chains=2)
    with pytest.raises(ValueError, match="per chain"):
        bm.gibbs_dp(X[:, :5], 5, pair_check=[0, 1], chains=2)
    for bad in ([0], [0, 0], [0, 130], [-1, 2], list(range(129))):
        with pytest.raises(ValueError):
            bm.gibbs_full(X, 5, 2, pair_check=bad)
    with pytest.raises(ValueError, match="stride"):
        bm.gibbs_stickbreaking(X, 5, 2, pair_check=[0, 1], pair_check_stride=0)
    with pytest.raises(ValueError):
        bm.pair_check(X, np.ones((1, 10), dtype=np.int32), 2)  # all 130 features


def _armed_run(feat, M, stride, P=5):
    """a run armed by hand, past the wrapper: the C entry's own refusal, before a device is touched"""
    L = _capi.lib()
    N, K, S = 10, 2, 3
    X = np.zeros((N, P), dtype=np.int32, order="F")
    f = None if feat is None else np.ascontiguousarray(feat, dtype=np.int32)
    s = bm._PairCheckOut(None if f is None else f.ctypes.data, M, stride, None, None, None, None, None, None, None, None, None)
    _capi.check(L.bmm_set_pair_check(C.byref(s)))
    z0 = np.ones(N, dtype=np.int32)
    z, th, al = np.empty((S, N), dtype=np.int32, order="F"), np.zeros((K, P, S), order="F"), np.zeros((S, 1), order="F")
    rc = L.bmm_collapsed_run(_capi.vp(X), C.c_int64(N), C.c_int(P), _capi.vp(z0), C.c_int(S), C.c_int(K), C.c_double(1.0),
                             C.c_double(0.5), C.c_double(0.5), C.c_double(1.0), C.c_double(1.0), C.c_int(0), C.c_int64(0),
                             C.c_uint64(1), C.c_int(0), _capi.vp(z), _capi.vp(th), _capi.vp(al))
    return rc, L.bmm_last_error().decode()


@pytest.mark.parametrize("feat,M,stride,word", [([0], 1, 1, "2 to 128"), (list(range(5)) * 26, 130, 1, "2 to 128"),
                                                ([0, 5], 2, 1, "not a feature"), ([0, -1], 2, 1, "not a feature"),
                                                ([1, 2, 1], 3, 1, "distinct"), ([0, 1], 2, 0, "stride"), (None, 2, 1, "null")])
def test_c_entry_refuses_a_run_armed_by_hand(feat, M, stride, word):
    rc, msg = _armed_run(feat, M, stride)
    assert rc == 1 and word in msg, (rc, msg)  # BMM_E_ARG


def test_plan_is_bookkeeping():
    p = bm.pair_check_plan(4096 * 2 + 5, 9, 128)
    assert p["tiles"] == 10 and p["label_blocks"] == -(-9 // p["ka"]) and p["threads"] * p["pairs_per_lane"] == 1024
    assert p["chunks"] == (4096 * 2 + 5 + 63) // 64 and p["chunks_per_slice"] % p["chunks_per_round"] == 0
    assert p["row_slices"] == -(-p["chunks"] // p["chunks_per_slice"])
    assert p["bytes_slices"] == 128 * p["chunks"] * 8 and p["bytes_counts"] == 9 * (8128 + 128 + 1) * 4
    assert bm.pair_check_plan(10, 65, 2)["label_blocks"] == -(-65 // p["ka"]) and bm.pair_check_plan(10, 8, 33)["tiles"] == 3
    for bad in ((0, 2, 2), (10, 0, 2), (10, 2, 1), (10, 2, 129)):
        with pytest.raises(_capi.BmmError):
            bm.pair_check_plan(*bad)
