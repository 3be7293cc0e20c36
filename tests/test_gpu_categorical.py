"""Categorical features on the device (include/bmm_mcmc.h "categorical features") against the NumPy
restatement (tests/categorical_ref.py), against the plain chain the oracle pins, and against the exact posterior by
enumeration."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref as cr  # noqa: E402
import split_merge_checks as chk  # noqa: E402
import split_merge_ref as smr  # noqa: E402

pytestmark = pytest.mark.gpu

BETA = 0.5
ALPHA = 1.3
E_ARG, E_UNSUPPORTED = 1, 2


@pytest.fixture(scope="module")
def bmm():
    import importlib
    return importlib.import_module("bmm_mcmc_amd")  # (the module the dbg_lib fixture steers)


def _gamma(sampler):
    return BETA if sampler == "dp" else 0.8  # (the DP chain takes beta == gamma only; the blocks read beta alone)


def _chain(bmm, sampler, X, K, batch, seed, levels=None, initial=None):
    N, P = X.shape
    c = bmm.Chain(sampler, N, P, K, alpha=ALPHA, beta=BETA, gamma=_gamma(sampler), batch=batch, seed=seed)
    c.set_data(X)
    if levels is not None:
        c.set_categorical(levels)
    if sampler == "collapsed":
        if initial is None:
            initial = np.random.default_rng(seed).integers(1, K + 1, N).astype(np.int32)
        c.set_initial_labels(initial)
    return c


def _rows(N):
    return np.unique(np.concatenate([np.arange(0, min(N, 130)), np.arange(max(0, N - 70), N), np.arange(1000, N, 997)]))


def _agree(got, want, tol=1e-12):
    big = want > 1e-300
    rel = np.abs(got[big] - want[big]) / want[big]
    assert rel.max() <= tol, rel.max()
    assert np.all(got[~big] <= 1e-300)
    return rel.max()


# ---------------------------------------------------------------- 1. the conditionals
# a partial group; a block over columns 28 .. 32 (a plane word, a W-group and an own-cluster group boundary); P = 130 (the
# generic path and the second chunk, a block across column 120); more than 32 categories; many workgroups
SHAPES = [(300, [3, 1], 3), (300, [1] * 28 + [5] + [1] * 4, 5), (300, [4] * 29 + [6] + [1] * 8, 4), (300, [5] * 4, 40),
          (70_000, [3, 4, 1, 5], 5)]


@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
@pytest.mark.parametrize("N,levels,K", SHAPES, ids=["partial", "word", "generic", "K40", "N70000"])
def test_probabilities_equal_the_restatement(bmm, N, levels, K, sampler):
    """batch = N: the probabilities of a sweep are a pure function of the labels before it"""
    X, lev = cr.expand(cr.draw(N, levels, 3)[0], levels)
    rows = _rows(N)
    plan = bmm.categorical_plan(sampler, N, K, levels, batch=N)
    with _chain(bmm, sampler, X, K, N, 11, levels) as c:
        np.testing.assert_array_equal(c.categorical(), levels)
        c.sweeps(2)
        z = c.labels() - 1
        probs = c.sweep_probs()
        want = cr.z_conditional(X, z, K, ALPHA, BETA, _gamma(sampler), lev, sampler, rows=rows)
        worst = _agree(probs[rows], want)
        print("%s N=%d P=%d K=%d %s plan packed=%s worst relative %.2e" % (sampler, N, X.shape[1], K, c.kernel_shape(), plan["packed"], worst))
        assert not c.kernel_shape()["builds_own_tables"]
        # the counts a categorical chain reports are the level counts
        Nk, S = c.counts()
        zn = c.labels() - 1
        Nk_ref, S_ref = cr.counts(X, zn, K)
        np.testing.assert_array_equal(Nk, Nk_ref)
        np.testing.assert_array_equal(S, S_ref)


# ---------------------------------------------------------------- 2. against code the oracle already pins
@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
@pytest.mark.parametrize("N,P,K", [(300, 37, 5), (300, 130, 4)])
def test_blocks_of_two_are_the_plain_chain_with_gamma_equal_beta(bmm, N, P, K, sampler):
    rng = np.random.default_rng(5)
    comp = rng.integers(3, size=N)
    Xb = np.asfortranarray((rng.random((N, P)) < np.array([0.2, 0.5, 0.8])[comp][:, None]).astype(np.int32))
    X2, _ = cr.expand(Xb, [2] * P)
    z1 = rng.integers(1, K, N).astype(np.int32)  # (the last label stays free: the DP's new cluster has a place)

    def probs(X, levels):
        c = bmm.Chain(sampler, N, X.shape[1], K, alpha=ALPHA, beta=BETA, gamma=BETA, batch=N, seed=3)
        with c:
            c.set_data(X)
            if levels is not None:
                c.set_categorical(levels)
            if sampler == "collapsed":
                c.set_initial_labels(z1)
            else:
                c.sweeps(1)
                c.set_labels(z1)
            return c.sweep_probs()

    plain, cat = probs(Xb, None), probs(X2, [2] * P)
    print(sampler, N, P, K, "worst relative %.2e" % _agree(cat, plain))


# ---------------------------------------------------------------- 3. no block is the plain build
def _state(c):
    Nk, S = c.counts()
    return c.labels().tobytes(), np.asarray(Nk).tobytes(), np.asarray(S).tobytes(), np.float64(c.alpha()).tobytes()


def _five_sweeps(bmm, sampler, X, K, levels):
    out = []
    N, P = X.shape
    c = bmm.Chain(sampler, N, P, K, beta=BETA, gamma=BETA, seed=17)  # alpha sampled, the default batch
    with c:
        c.set_data(X)
        if levels is not None:
            c.set_categorical(levels)
        if sampler == "collapsed":
            c.set_initial_labels(np.random.default_rng(2).integers(1, K + 1, N).astype(np.int32))
        for _ in range(4):
            c.sweeps(1)
            out.append(_state(c))
        out.append(c.sweep_probs().tobytes())
        out.append(_state(c))
        shape = c.kernel_shape()
        packed = None
        if hasattr(bmm._capi.lib(), "bmm_dbg_kernel_packed"):
            packed = bool(bmm._capi.lib().bmm_dbg_kernel_packed(c._h))
    return out, shape, packed


@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
def test_levels_of_all_one_are_the_unarmed_chain_unpacked(bmm, sampler):
    X = np.asfortranarray((np.random.default_rng(1).random((5000, 37)) < 0.4).astype(np.int32))
    plain, _, _ = _five_sweeps(bmm, sampler, X, 6, None)
    armed, shape, _ = _five_sweeps(bmm, sampler, X, 6, [1] * 37)
    assert not shape["builds_own_tables"]
    assert plain == armed


@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
def test_levels_of_all_one_are_the_unarmed_chain_packed(bmm, dbg_lib, sampler):
    """the test variant sees one compute unit, so that the default batch of a test-sized chain is a long launch and the
    chain runs the packed kernel: k_count_tables<TAB_CAT> writes its image"""
    dbg_lib.setenv("BMM_DEBUG_CUS", "1")
    dbg_lib.setenv("BMM_DEBUG_PK", "1")
    X = np.asfortranarray((np.random.default_rng(1).random((80_000, 24)) < 0.4).astype(np.int32))
    plain, _, pk_plain = _five_sweeps(bmm, sampler, X, 12, None)
    armed, shape, pk_armed = _five_sweeps(bmm, sampler, X, 12, [1] * 24)
    assert pk_plain and pk_armed and not shape["builds_own_tables"]
    assert plain == armed


def test_a_packed_chain_with_blocks_equals_the_restatement(bmm, dbg_lib):
    """the packed image of a chain with blocks: the draw and the emitted probabilities rest on it"""
    dbg_lib.setenv("BMM_DEBUG_CUS", "1")
    dbg_lib.setenv("BMM_DEBUG_PK", "1")
    N, levels, K = 6000, [3, 4, 1, 5, 1, 1, 6], 12
    X, lev = cr.expand(cr.draw(N, levels, 8)[0], levels)
    for sampler in ("collapsed", "dp"):
        with _chain(bmm, sampler, X, K, N, 5, levels) as c:
            assert bmm._capi.lib().bmm_dbg_kernel_packed(c._h)
            c.sweeps(2)
            z = c.labels() - 1
            probs = c.sweep_probs()
            _agree(probs, cr.z_conditional(X, z, K, ALPHA, BETA, _gamma(sampler), lev, sampler))
            # the labels the packed kernel drew are draws from rows it emitted: none at probability 0
            zn = c.labels() - 1
            assert np.all(probs[np.arange(N), zn] > 0)


# ---------------------------------------------------------------- 4. exactness
def test_batch_1_chain_samples_the_exact_posterior_and_not_the_bernoulli_one(bmm):
    Xc, levels = cr.seven_rows()
    X1h, _ = cr.expand(Xc, levels)
    D = bmm.categorical(Xc, levels=[3, 4, 2])
    np.testing.assert_array_equal(np.asarray(D), X1h)
    np.testing.assert_array_equal(D.chain_levels, levels)
    parts, w = cr.exact_posterior(Xc, levels, ALPHA, BETA)
    out = bmm.gibbs_dp(D, 30_001, alpha=ALPHA, beta=BETA, gamma=BETA, burnin=1, maxK=30, batch=1, seed=9)
    visited = [smr.canon(r) for r in out["z"]]
    chk.check_against_enumeration(visited, parts, w)
    # the check tells the two models apart: the Bernoulli posterior of the same columns lies outside its margin
    F, exact = cr.compared_quantities(parts, w)
    _, exact_b = cr.compared_quantities(parts, chk.exact_posterior(X1h, ALPHA, BETA, BETA)[1])
    apart = np.abs(exact - exact_b) > cr.margins(visited, parts, F, exact)
    print("quantities on which the Bernoulli posterior lies outside the margin: %d of %d" % (apart.sum(), len(apart)))
    assert apart.any()


# ---------------------------------------------------------------- 5. k_cat_check
def _refused(bmm, fn, row, feature):
    with pytest.raises(bmm.BmmError) as e:
        fn()
    assert e.value.code == E_ARG, str(e.value)
    assert "row %d " % row in str(e.value) and "feature %d " % feature in str(e.value), str(e.value)


@pytest.mark.parametrize("data_first", [True, False])
def test_one_hot_check_names_the_first_bad_row_and_its_feature(bmm, data_first):
    levels = [1] * 28 + [5] + [3] + [1]  # the block of 5 over columns 28 .. 32, across a plane word; the block of 3 behind it
    N = 70_001
    Xc = cr.draw(N, levels, 6)[0]
    X, _ = cr.expand(Xc, levels)

    def hand_over(Xbad):
        c = bmm.Chain("dp", N, X.shape[1], 5, alpha=ALPHA, beta=BETA, gamma=BETA, seed=1)
        with c:
            if data_first:
                c.set_data(Xbad)
                c.set_categorical(levels)
            else:
                c.set_categorical(levels)
                c.set_data(Xbad)
            c.sweeps(1)

    hand_over(X)  # a clean matrix passes
    # two bits in a block, in the word behind the boundary; none; the first row; the last row
    for row, col, value, feature in ((4321, 28 + (Xc[4321, 28] + 1) % 5, 1, 28), (777, 28 + Xc[777, 28], 0, 28),
                                     (0, 33 + Xc[0, 29], 0, 29), (N - 1, 33 + (Xc[N - 1, 29] + 1) % 3, 1, 29)):
        Xbad = X.copy(order="F")
        Xbad[row, col] = value
        _refused(bmm, lambda: hand_over(Xbad), row, feature)
    # two bad rows: the first is named; two bad blocks in a row: its first
    Xbad = X.copy(order="F")
    Xbad[60_000, 28:33] = 0
    Xbad[123, 33:36] = 1
    Xbad[123, 28:33] = 1
    _refused(bmm, lambda: hand_over(Xbad), 123, 28)
    # a Bernoulli column may hold anything
    Xok = X.copy(order="F")
    Xok[:, 5] = 1 - Xok[:, 5]
    hand_over(Xok)


def test_a_chain_refuses_every_other_likelihood_in_either_order(bmm):
    levels = [3, 1, 4]
    N, K = 400, 4
    X, _ = cr.expand(cr.draw(N, levels, 2)[0], levels)
    P = X.shape[1]
    options = {
        "temper": lambda c: c.set_temper(0.5),
        "feature_select": lambda c: c.set_feature_select(True, 0.5),
        "split_merge": lambda c: c.set_split_merge(1, 2),
        "missing": lambda c: c.set_missing(rows=[1], cols=[2]),
        "newdata": lambda c: c.set_newdata(X[:5]),
        "loo": lambda c: c.set_loo(True),
        "logpost": lambda c: c.set_logpost(True),
        "pair_check": lambda c: c.set_pair_check([0, 1, 2]),
        "init_labels": lambda c: c.init_labels("kmodes"),
    }
    for name, arm in options.items():
        for levels_first in (True, False):
            if name == "init_labels" and not levels_first:
                continue  # (a start leaves nothing armed behind it)
            with bmm.Chain("dp", N, P, K, alpha=ALPHA, beta=BETA, gamma=BETA, seed=1) as c:
                c.set_data(X)
                c.sweeps(1)
                first, second = (lambda: c.set_categorical(levels), lambda: arm(c))
                if not levels_first:
                    first, second = second, first
                first()
                with pytest.raises(bmm.BmmError) as e:
                    second()
                assert e.value.code == E_UNSUPPORTED, (name, levels_first, str(e.value))
    for sampler in ("stickbreaking", "full"):
        with bmm.Chain(sampler, N, P, K, alpha=ALPHA, beta=BETA, gamma=BETA, seed=1) as c:
            with pytest.raises(bmm.BmmError) as e:
                c.set_categorical(levels)
            assert e.value.code == E_UNSUPPORTED
    with bmm.Chain("dp", N, P, K, alpha=ALPHA, beta=BETA, gamma=BETA, seed=1, x_layout="int32") as c:
        with pytest.raises(bmm.BmmError) as e:
            c.set_categorical(levels)
        assert e.value.code == E_UNSUPPORTED
    with bmm.Chain("collapsed", N, P, K, alpha=ALPHA, beta=BETA, gamma=BETA, seed=1) as c:
        c.set_categorical(levels)
        with pytest.raises(bmm.BmmError) as e:
            c.set_shard(2 * N, 0)
        assert e.value.code == E_UNSUPPORTED
        for bad in ([3, 1, 3], [3, 0, 5], [9], [300, 1, 1]):
            with pytest.raises(bmm.BmmError) as e:
                c.set_categorical(bad)
            assert e.value.code == E_ARG
        np.testing.assert_array_equal(c.categorical(), levels)  # a refused vector changes nothing
        assert c.set_categorical(None) == 0 and c.categorical().size == 0  # withdrawn


# ---------------------------------------------------------------- 6. through a run
def test_whole_route(bmm):
    N, K = 600, 3
    Xc, comp = cr.draw(N, [3, 2, 4, 5], 4)
    D = bmm.categorical(Xc)
    known = np.zeros(N, dtype=np.int64)
    known[:6] = comp[:6] + 1
    kw = dict(K=K, seed=1, partition="vi", known=known)
    out = bmm.gibbs_collapsed(D, 300, **kw)
    assert list(out["categorical"]) == ["levels", "columns"]
    np.testing.assert_array_equal(out["categorical"]["levels"], [3, 2, 4, 5])
    assert out["categorical"]["columns"] == D.columns
    X = np.asarray(D)
    z, theta = out["z"], out["theta"]
    S = z.shape[0]
    for s in (0, S // 2, S - 1):  # theta = counts / sizes recomputed from the returned labels
        Nk, Sk = cr.counts(X, z[s] - 1, K)
        with np.errstate(invalid="ignore", divide="ignore"):
            np.testing.assert_array_equal(theta[:, :, s], Sk / Nk[:, None].astype(np.float64))
    for dec in D.decode(theta):  # level proportions: every feature's sum to 1 in every class and sweep
        tot = dec.sum(axis=1)
        np.testing.assert_allclose(tot[~np.isnan(tot)], 1.0, rtol=0, atol=1e-12)
    assert (z[:, :6] == known[:6]).all()  # known= holds its rows
    alone = bmm.partition_distances(z, criterion="vi", Kc=K)  # the partition= result: the stand-alone call on the trace
    assert out["partition"]["best"] == alone["best"] and np.array_equal(out["partition"]["loss"], alone["loss"])
    np.testing.assert_array_equal(out["partition"]["z"], z[alone["best"]])
    again = bmm.gibbs_collapsed(D, 300, **kw)  # the same seed gives the same bytes twice
    for k in ("z", "theta", "alpha"):
        assert out[k].tobytes() == again[k].tobytes()
    # ... and the plain chain over the same columns is another chain
    plain = bmm.gibbs_collapsed(X, 300, **kw)
    assert "categorical" not in plain and plain["z"].tobytes() != out["z"].tobytes()
