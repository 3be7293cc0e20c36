"""The pairwise local-dependence check on the device (include/bmm_mcmc.h "pairwise local-dependence check", DESIGN.md
section 22).  The counts are held to the NumPy restatement's integers exactly, at the shapes where the counting kernel
takes another path; the statistics to the host statement of bmm_spec.h (tests/pair_check/pair_check_host.cpp) bit for
bit from the device's own counts, and to the restatement within its rounding bound; the fold to its own trace; the run
option, the resident calls and the stand-alone call to each other; an armed chain to an unarmed one, byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_check_host as host  # noqa: E402
import pair_check_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bmm():
    import importlib
    return importlib.import_module("bmm_mcmc_amd")


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _data(N, P, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray((rng.random((N, P)) < rng.uniform(0.15, 0.85, P)).astype(np.int32)), rng


def _labels(rng, N, Kc, spread):
    """1-based labels: spread over all Kc labels (the last one holds a row), or concentrated in at most two"""
    if spread:
        z = rng.integers(1, Kc + 1, N)
        z[rng.integers(0, N)] = Kc
        return z.astype(np.int32)
    return rng.integers(1, min(Kc, 2) + 1, N).astype(np.int32)


def _chain(bmm, sampler, X, K, seed=3, batch=None, z1=None):
    N, P = X.shape
    c = bmm.Chain(sampler, N, P, K, alpha=1.0, seed=seed, batch=batch)
    c.set_data(X)
    rng = np.random.default_rng(seed)
    if sampler == "collapsed":
        c.set_initial_labels(rng.integers(1, K + 1, N).astype(np.int32) if z1 is None else z1)
    elif sampler in ("stickbreaking", "full"):
        pi = rng.random(K) + 0.1
        c.set_initial_params(pi / pi.sum(), rng.random((K, P)) * 0.8 + 0.1)
    return c


# ---------------------------------------------------------------- (a) the counts, exact
# (N, P, Kc, features, spread): N = 1, 63, 64, 65, 300 and one with two row slices of two rounds each; P = 2, 33, 37, 130
# (a word index of 4); features 31 with 32 and 63 with 64; M = 2, 8, 9, 33, 128 (unordered, non-contiguous, on P = 130:
# diagonal, off-diagonal and partial tiles); Kc = 1, 8, 9, 32, 33, 65 (one label block, a full one, and up to nine)
def _f128():
    return [int(v) for v in np.random.default_rng(2).permutation(130)[:128]]


COUNT_CASES = [
    (1, 2, 1, [0, 1], True), (63, 2, 8, [1, 0], True), (64, 33, 9, [31, 32], True), (65, 37, 32, list(range(8)), True),
    (300, 130, 33, [63, 64, 129, 0, 31, 32, 5, 128, 100], True), (300, 37, 65, list(range(36, 3, -1)), True),
    (300, 37, 65, list(range(33)), False), (300, 130, 9, _f128(), True), (300, 130, 1, _f128(), True),
    (4096 * 2 + 77, 37, 33, list(range(37)), True), (4096 * 2 + 77, 37, 8, [0, 36, 7], False),
]


@pytest.mark.parametrize("N,P,Kc,feat,spread", COUNT_CASES)
def test_counts_exact(bmm, N, P, Kc, feat, spread):
    X, rng = _data(N, P, 10 + N + Kc)
    z = _labels(rng, N, Kc, spread)
    M = len(feat)
    if N > 4096:
        plan = bmm.pair_check_plan(N, Kc, M)
        assert plan["row_slices"] >= 2 and plan["chunks_per_slice"] >= 2 * plan["chunks_per_round"], plan
    out = bmm.pair_check(X, z, Kc, features=feat, counts=True)
    c, s, n = ref.counts(X, z - 1, Kc, np.asarray(feat))
    assert out["counts"].shape == (1, Kc, M * (M - 1) // 2)
    assert np.array_equal(out["counts"][0].astype(np.int64), c)
    assert np.array_equal(out["n11"].astype(np.int64), c.sum(axis=0))
    if spread and Kc >= 33:
        assert n[32:].sum() > 0  # a label at index 32 or above holds rows
    if not spread:
        assert np.count_nonzero(n) <= 2
    # the statistics of the same state: the host statement bit for bit, the restatement within its bound
    want = host.run(c, s, n)
    assert np.array_equal(_bits(out["z"][0]), _bits(want["z"])) and np.array_equal(_bits(out["x2"][0]), _bits(want["x2"]))
    host.check({"z": out["z"][0], "x2": out["x2"][0]}, c, s, n, "stand-alone N=%d Kc=%d M=%d" % (N, Kc, M))


def test_margins_equal_chain_counts(bmm):
    X, rng = _data(300, 37, 4)
    feat = [36, 0, 31, 32, 5]
    with _chain(bmm, "collapsed", X, 33, z1=_labels(rng, 300, 33, True)) as c:
        c.set_pair_check(feat)
        for sweeps in (0, 2):  # the starting allocation (label 33 holds a row), then a sampled state
            c.sweeps(sweeps)
            cnt, marg, rows = c.pair_counts(margins=True)
            Nk, S = c.counts()
            if sweeps == 0:
                assert Nk[32:].sum() > 0  # a label at index 32 or above holds rows
            rc, rs, rn = ref.counts(X, c.labels() - 1, 33, np.asarray(feat))
            assert np.array_equal(cnt.astype(np.int64), rc)
            assert np.array_equal(rs, S[:, feat]) and np.array_equal(rn, Nk)  # the restatement's diagonal is the chain's counts
            assert np.array_equal(marg.astype(np.int64), rs) and np.array_equal(rows.astype(np.int64), rn)
            assert np.array_equal(c.pair_counts(), cnt)  # one state gives the same integers twice


# ---------------------------------------------------------------- (b) the statistics of a resident chain
def _check_state(c, X, feat, Kc):
    cnt, marg, rows = c.pair_counts(margins=True)
    st = c.pair_check_state()
    want = host.run(cnt, marg, rows)
    for key in ("z", "x2"):
        assert np.array_equal(_bits(st[key]), _bits(want[key])), key
    assert np.array_equal(st["df"], want["df"])
    rc, rs, rn = ref.counts(X, c.labels() - 1, Kc, np.asarray(feat))
    assert np.array_equal(cnt.astype(np.int64), rc)
    host.check(st, rc, rs, rn, "resident")
    again = c.pair_check_state()
    assert np.array_equal(_bits(again["z"]), _bits(st["z"])) and np.array_equal(_bits(again["x2"]), _bits(st["x2"]))
    return st, rn


@pytest.mark.parametrize("sampler,K", [("collapsed", 5), ("dp", 30), ("stickbreaking", 6), ("full", 4)])
def test_state_against_host_and_restatement(bmm, sampler, K):
    X, _ = _data(700, 20, 21)
    X[:, 3] = 1  # a constant feature: V = 0 in every label, no Z, df 0
    feat = [3, 0, 19, 7, 8]
    with _chain(bmm, sampler, X, K) as c:
        c.set_pair_check(feat)
        c.sweeps(3)
        st, n = _check_state(c, X, feat, K)
        assert np.all(np.isnan(st["z"][:4])) and np.all(st["df"][:4] == 0) and np.all(st["x2"][:4] == 0.0)
        if sampler == "dp":
            assert np.count_nonzero(n == 0) > 0  # empty labels after sweeps


def test_state_with_a_cluster_of_one_row(bmm):
    X, rng = _data(200, 9, 8)
    z1 = rng.integers(1, 3, 200).astype(np.int32)
    z1[17] = 4  # label 4 holds one row, label 3 none
    with _chain(bmm, "collapsed", X, 4, z1=z1) as c:
        c.set_pair_check(True)
        st, n = _check_state(c, X, list(range(9)), 4)
        assert n[3] == 1 and n[2] == 0 and st["df"].max() <= 2


# ---------------------------------------------------------------- (c) the fold
def _fold_of(z, x2):
    """the fold of trace rows in sweep order, one add per pair per state"""
    sz, sz2, sx = np.zeros(z.shape[1]), np.zeros(z.shape[1]), np.zeros(z.shape[1])
    nz, n = np.zeros(z.shape[1], dtype=np.int64), 0
    for r in range(z.shape[0]):
        if np.all(np.isnan(x2[r])):
            continue
        ok = ~np.isnan(z[r])
        sz[ok] = sz[ok] + z[r][ok]
        sz2[ok] = sz2[ok] + z[r][ok] * z[r][ok]
        nz += ok
        sx = sx + x2[r]
        n += 1
    return sz, sz2, sx, nz, n


def test_fold_equals_its_trace_stride_and_reset(bmm):
    X, _ = _data(500, 12, 31)
    X[:, 2] = 0
    feat = [2, 0, 1, 11, 5, 6]
    with _chain(bmm, "collapsed", X, 4) as c:
        c.set_pair_check(feat)
        tr = c.sweeps_pair_check(30, trace=True)
        assert tr["z"].shape == (30, 15) and not np.any(np.isnan(tr["x2"]))
        f = c.pair_check()
        sz, sz2, sx, nz, n = _fold_of(tr["z"], tr["x2"])
        assert f["n_folded"] == 30 == n and np.array_equal(f["n_z"], nz)
        assert np.array_equal(_bits(f["sum_z"]), _bits(sz)) and np.array_equal(_bits(f["sum_z2"]), _bits(sz2))
        assert np.array_equal(_bits(f["sum_x2"]), _bits(sx))
        cnt = c.pair_counts()
        assert np.array_equal(f["n11"], cnt.sum(axis=0)) and np.array_equal(f["n11"], ref.counts(X, c.labels() - 1, 4, np.asarray(feat))[0].sum(axis=0))
        np.testing.assert_allclose(f["z_mean"][5:], sz[5:] / 30)
        assert np.all(np.isnan(f["z_mean"][:5])) and np.all(f["n_z"][:5] == 0)  # the pairs of the constant feature
        c.pair_check_reset()
        g = c.pair_check()
        assert g["n_folded"] == 0 and not g["sum_x2"].any() and not g["n_z"].any() and not g["sum_df"].any()
        # stride 3: sweeps 0, 3, 6, ... of the folded ones, the rest NaN; arming again empties the fold
        c.sweeps_pair_check(2)
        assert c.pair_check()["n_folded"] == 2
        c.set_pair_check(feat, stride=3)
        assert c.pair_check()["n_folded"] == 0 and not c.pair_check()["sum_x2"].any()
        tr = c.sweeps_pair_check(8, trace=True)
        done = ~np.isnan(tr["x2"]).all(axis=1)
        assert np.array_equal(np.nonzero(done)[0], [0, 3, 6]) and np.all(np.isnan(tr["z"][~done]))
        f = c.pair_check()
        assert f["n_folded"] == 3 and np.array_equal(_bits(f["sum_x2"]), _bits(_fold_of(tr["z"], tr["x2"])[2]))
        c.set_pair_check(None)
        with pytest.raises(bmm._capi.BmmError):
            c.pair_check()


# ---------------------------------------------------------------- (d) the routes
@pytest.mark.parametrize("burnin", [0, 4])
def test_run_rows_equal_stand_alone_and_resident(bmm, burnin):
    X, _ = _data(900, 16, 41)
    feat = [15, 0, 3, 4, 9]
    kw = dict(alpha=1.0, burnin=burnin, seed=9, pair_check=feat, pair_check_trace=True)
    a = bmm.gibbs_collapsed(X, 12, 3, **kw)
    b = bmm.gibbs_collapsed(X, 12, 3, **kw)
    pa, pb = a["pair_check"], b["pair_check"]
    S = 12 - burnin
    first = 0 if burnin else 1  # without burn-in row 0 is the start: NaN
    assert pa["z"].shape == (S, 10) and np.array_equal(pa["features"], feat) and np.array_equal(pa["pairs"], bmm.pair_check_pairs(5))
    if not burnin:
        assert np.all(np.isnan(pa["z"][0])) and np.all(np.isnan(pa["x2"][0]))
    assert pa["n_folded"] == S - first
    for key in ("z", "x2", "sum_z", "sum_z2", "sum_x2"):  # same seed, same bits, twice
        assert np.array_equal(_bits(pa[key]), _bits(pb[key])), key
    alone = bmm.pair_check(X, a["z"][first:], 3, features=feat)
    assert np.array_equal(_bits(alone["z"]), _bits(pa["z"][first:])) and np.array_equal(_bits(alone["x2"]), _bits(pa["x2"][first:]))
    for key in ("sum_z", "sum_z2", "sum_x2"):
        assert np.array_equal(_bits(alone[key]), _bits(pa[key])), key
    assert np.array_equal(alone["sum_df"], pa["sum_df"]) and np.array_equal(alone["n11"], pa["n11"]) and alone["n_folded"] == pa["n_folded"]
    # the resident route: a chain given a row of the run's trace scores it to the same bits
    with _chain(bmm, "collapsed", X, 3, z1=np.ascontiguousarray(a["z"][S - 1])) as c:
        c.set_pair_check(feat)
        st = c.pair_check_state()
        assert np.array_equal(_bits(st["z"]), _bits(pa["z"][S - 1])) and np.array_equal(_bits(st["x2"]), _bits(pa["x2"][S - 1]))


def test_run_stride_and_the_other_samplers(bmm):
    X, _ = _data(600, 10, 43)
    for fn, args in ((bmm.gibbs_dp, dict(maxK=12)), (bmm.gibbs_stickbreaking, dict(maxK=5)), (bmm.gibbs_full, dict(K=4))):
        K = args.get("maxK", args.get("K"))
        out = fn(X, 11, burnin=3, seed=2, pair_check=True, pair_check_stride=3, pair_check_trace=True, **args)
        p = out["pair_check"]
        done = ~np.isnan(p["x2"]).all(axis=1)
        assert np.array_equal(np.nonzero(done)[0], [0, 3, 6]) and p["n_folded"] == 3, fn.__name__
        alone = bmm.pair_check(X, out["z"][done], K)
        assert np.array_equal(_bits(alone["z"]), _bits(p["z"][done])) and np.array_equal(_bits(alone["sum_x2"]), _bits(p["sum_x2"])), fn.__name__


def test_under_temper_the_rows_are_rung_zeros(bmm):
    X, _ = _data(800, 14, 47)
    # powers close enough that exchanges are accepted: the row of a kept sweep must be the state behind the exchange
    out = bmm.gibbs_collapsed(X, 12, 3, alpha=1.0, burnin=2, seed=5, temper=[1, 0.98, 0.96], pair_check=[0, 5, 13, 2],
                              pair_check_trace=True)
    p = out["pair_check"]
    alone = bmm.pair_check(X, out["z"], 3, features=[0, 5, 13, 2])
    print("temper: proposed", out["temper"]["proposed"], "accepted", out["temper"]["accepted"], "walker at rung 0", out["temper"]["walker_cold"])
    assert p["n_folded"] == 10 and out["temper"]["accepted"][0] > 0  # rung 0 took another rung's state at least once
    assert np.array_equal(_bits(alone["z"]), _bits(p["z"])) and np.array_equal(_bits(alone["x2"]), _bits(p["x2"]))


# ---------------------------------------------------------------- (e) it changes nothing
@pytest.mark.parametrize("sampler,K,env", [("collapsed", 4, {}), ("dp", 20, {}), ("collapsed", 4, {"BMM_DEBUG_GENERIC": "1"}),
                                           ("dp", 20, {"BMM_DEBUG_GENERIC": "1"})])
def test_an_armed_chain_is_an_unarmed_chain(bmm, dbg_lib, sampler, K, env):
    for k, v in env.items():
        dbg_lib.setenv(k, v)
    X, _ = _data(1500, 18, 51)
    states = []
    for armed in (False, True):
        with bmm.Chain(sampler, 1500, 18, K, alpha=None, seed=6) as c:
            c.set_data(X)
            if sampler == "collapsed":
                c.set_initial_labels(np.random.default_rng(1).integers(1, K + 1, 1500).astype(np.int32))
            if armed:
                c.set_pair_check(True, stride=2)
                c.sweeps_pair_check(10)
                c.sweeps(5)  # armed, not folding
                c.sweeps_pair_check(5)
                assert c.pair_check()["n_folded"] == 5 + 3
            else:
                c.sweeps(20)
            Nk, S = c.counts()
            states.append((c.labels().tobytes(), Nk.tobytes(), S.tobytes(), np.float64(c.alpha()).tobytes()))
    assert states[0] == states[1]


# ---------------------------------------------------------------- (f) planted dependence
def test_planted_dependence_on_the_device(bmm):
    X, z0 = ref.planted(ref.PLANTED_SEED)
    X = np.asfortranarray(X)
    out = bmm.gibbs_collapsed(X, 60, 3, alpha=1.0, burnin=20, seed=1, initial_K=(z0 + 1).astype(np.int32), pair_check=True)
    p = out["pair_check"]
    assert p["n_folded"] == 40
    # the restatement first, on the device's own label trace
    zs, xs = [], []
    for row in out["z"]:
        st = ref.stats(X, row - 1, 3, np.arange(37))
        zs.append(st["z"])
        xs.append(st["x2"])
    z_ref, x_ref = np.mean(zs, axis=0), np.mean(xs, axis=0)
    ref.check_planted(z_ref, x_ref)
    np.testing.assert_allclose(p["z_mean"], z_ref, rtol=0, atol=1e-9)
    np.testing.assert_allclose(p["x2_mean"], x_ref, rtol=1e-12, atol=1e-9)
    ref.check_planted(p["z_mean"], p["x2_mean"])


# ---------------------------------------------------------------- (g) the refusals
def test_refusals(bmm):
    E_ARG, E_UNSUPPORTED, E_STATE = 1, 2, 5
    X, _ = _data(100, 130, 61)

    def code(fn, *a, **k):
        with pytest.raises(bmm._capi.BmmError) as e:
            fn(*a, **k)
        assert str(e.value)  # a message that says why
        return e.value.code

    L = bmm._capi.lib()

    def arm_raw(c, feat, M, stride):
        f = np.ascontiguousarray(feat, dtype=np.int32)
        rc = L.bmm_chain_set_pair_check(c._h, bmm._capi.vp(f), C.c_int(M), C.c_int(stride))
        return rc, L.bmm_last_error().decode()

    with _chain(bmm, "collapsed", X, 3) as c:
        for feat, M, stride, word in (([0], 1, 1, "2 to 128"), ([0] * 129, 129, 1, "2 to 128"), ([0, 130], 2, 1, "not a feature"),
                                      ([0, -1], 2, 1, "not a feature"), ([4, 4], 2, 1, "distinct"), ([0, 1], 2, 0, "stride")):
            rc, msg = arm_raw(c, feat, M, stride)
            assert rc == E_ARG and word in msg, (rc, msg)
        assert code(c.pair_check_reset) == E_STATE and code(c.sweeps_pair_check, 1) == E_STATE  # not armed
        c.set_features(np.ones(130, dtype=np.uint8))  # a feature mask
        assert code(c.set_pair_check, [0, 1]) == E_UNSUPPORTED
    with bmm.Chain("collapsed", 100, 130, 600, alpha=1.0, seed=1) as c:  # 600 labels x 8128 pairs x 4 bytes: above the cap
        c.set_data(X)
        rc, msg = arm_raw(c, np.arange(128), 128, 1)
        assert rc == E_ARG and "cap" in msg, (rc, msg)
    with bmm.Chain("collapsed", 100, 130, 3, alpha=1.0, seed=1, x_layout="int32") as c:
        c.set_data(X)
        assert code(c.set_pair_check, [0, 1]) == E_UNSUPPORTED
    for arm_first in (False, True):  # a sharded chain (one device suffices), armed after or before it was sharded
        with bmm.Chain("full", 100, 130, 3, alpha=1.0, seed=1) as c:
            c.set_data(X)
            if arm_first:
                c.set_pair_check([0, 1, 2])
            c.set_shard(200, 0)
            if not arm_first:
                rc, msg = arm_raw(c, [0, 1, 2], 3, 1)
                assert rc == E_UNSUPPORTED and "sharded" in msg, (rc, msg)
                assert code(c.set_pair_check, [0, 1, 2]) == E_UNSUPPORTED
            else:
                assert code(c.pair_check_state) == E_UNSUPPORTED and code(c.pair_counts) == E_UNSUPPORTED
                assert code(c.sweeps_pair_check, 1) == E_UNSUPPORTED
    with _chain(bmm, "collapsed", X, 3) as c:  # new data under an armed check: the slices are of the old matrix
        c.set_pair_check([0, 1])
        assert code(c.set_data, X) == E_STATE
        c.set_pair_check(None)
        c.set_data(X)
        c.set_pair_check([0, 1])
        c.pair_check_state()
    with _chain(bmm, "dp", X, 10) as c:  # unseated rows before the first sweep
        c.set_pair_check([0, 1, 2])
        assert code(c.pair_check_state) == E_STATE and code(c.pair_counts) == E_STATE
        c.sweeps(1)
        c.pair_check_state()
    # the stand-alone call: labels outside 1..Kc, before a device is touched
    z = np.ones((1, 100), dtype=np.int32)
    z[0, 7] = 4
    assert code(bmm.pair_check, X, z, 3, features=[0, 1]) == E_ARG
    z[0, 7] = 0
    assert code(bmm.pair_check, X, z, 3, features=[0, 1]) == E_ARG
    # a run with a feature mask: refused by the C entry
    assert code(bmm.gibbs_collapsed, X[:, :20], 6, 3, seed=1, select_features=True, pair_check=[0, 1]) == E_UNSUPPORTED
