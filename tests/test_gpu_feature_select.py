"""Feature selection on the device (include/bmm_mcmc.h "feature selection") against the NumPy
restatement (tests/feature_select_ref.py) and against the exact joint posterior by enumeration."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feature_select_ref as fsr  # noqa: E402
import split_merge_checks as chk  # noqa: E402
import split_merge_ref as smr  # noqa: E402
from test_split_merge_ref import seven_observations  # noqa: E402

pytestmark = pytest.mark.gpu

BETA = GAMMA = 0.5
ALPHA = 1.3


@pytest.fixture(scope="module")
def bmm():
    import importlib
    return importlib.import_module("bmm_mcmc_amd")  # (the module the dbg_lib fixture steers)


def _mixture(N, P, thetas, seed):
    rng = np.random.default_rng(seed)
    comp = rng.integers(len(thetas), size=N)
    X = (rng.random((N, P)) < np.asarray(thetas)[comp][:, None]).astype(np.int32)
    return np.asfortranarray(X), comp


def _masks(P, W):
    """all ones; group 0 out; a middle group out; alternating; all zeros"""
    G = (P + W - 1) // W
    g0, mid = np.ones(P, dtype=np.uint8), np.ones(P, dtype=np.uint8)
    g0[:W] = 0
    mid[(G // 2) * W:(G // 2) * W + W] = 0
    return {"ones": np.ones(P, dtype=np.uint8), "group0": g0, "middle": mid, "alternating": (np.arange(P) % 2).astype(np.uint8),
            "zeros": np.zeros(P, dtype=np.uint8)}


def _chain(bmm, sampler, X, K, batch, seed, layout=None, labels=None, initial=None):
    N, P = X.shape
    c = bmm.Chain(sampler, N, P, K, alpha=ALPHA, beta=BETA, gamma=GAMMA, batch=batch, seed=seed, x_layout=layout)
    c.set_data(X)
    if sampler == "collapsed":
        if initial is None:
            initial = np.random.default_rng(seed).integers(1, (labels or K) + 1, N).astype(np.int32)
        c.set_initial_labels(initial)
    return c


# ---------------------------------------------------------------- 1. the masked tables
# (N, P, K): one partial group; a partial last group; the generic path; more than 32 categories (two lanes share an
# observation); more than one workgroup
SHAPES = [(300, 4, 3), (300, 37, 5), (300, 130, 4), (300, 20, 40), (70_000, 37, 5)]


@pytest.mark.parametrize("layout", ["bits", "int32"])
@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
@pytest.mark.parametrize("N,P,K", SHAPES)
def test_masked_probabilities_equal_the_restatement(bmm, N, P, K, sampler, layout):
    """batch = N: the probabilities of a sweep are a pure function of the labels before it.  A fixed mask, no step."""
    X, _ = _mixture(N, P, [0.2, 0.5, 0.8], 3)
    W = bmm._capi.lib().bmm_spec_group_width_for(bmm._capi.SAMPLER_CODE[sampler], K, P)
    rows = np.unique(np.concatenate([np.arange(0, min(N, 130)), np.arange(max(0, N - 70), N), np.arange(1000, N, 997)]))
    with _chain(bmm, sampler, X, K, N, 11, layout) as c:
        c.sweeps(2)
        for name, mask in _masks(P, W).items():
            c.set_features(mask)
            np.testing.assert_array_equal(c.features(), mask)
            z = c.labels() - 1
            probs = c.sweep_probs()
            want = fsr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, mask, sampler, rows=rows)
            got = probs[rows]
            big = want > 1e-300
            rel = np.abs(got[big] - want[big]) / want[big]
            print("%s %s %s N=%d P=%d K=%d %-11s worst relative %.2e" % (sampler, layout, c.kernel_shape(), N, P, K, name, rel.max()))
            assert rel.max() <= 1e-12
            assert np.all(got[~big] <= 1e-300)
            if name == "zeros":  # the prior term alone
                Nk = np.bincount(z, minlength=K).astype(np.float64)
                for r, i in enumerate(rows[:50]):
                    n = Nk.copy()
                    n[z[i]] -= 1
                    w = np.where(n > 0, n + (ALPHA / K if sampler == "collapsed" else 0.0), 0.0)
                    if sampler == "dp":
                        w[np.flatnonzero(n == 0)[0]] = ALPHA
                    np.testing.assert_allclose(got[r], w / w.sum(), rtol=1e-12, atol=0)
        assert not c.kernel_shape()["builds_own_tables"]


def _state(c):
    Nk, S = c.counts()
    return c.labels().tobytes(), Nk.tobytes(), S.tobytes(), np.float64(c.alpha()).tobytes()


# the switches of tests/test_gpu_chunks.py and tests/test_gpu_layouts.py, and the shapes that take another form under them
FORMS = [({}, "collapsed", 3000, 37, 20, 400), ({"BMM_DEBUG_NOSPLIT": "1"}, "collapsed", 3000, 37, 20, 400),
         ({"BMM_DEBUG_SPLIT": "1"}, "dp", 3000, 37, 19, 400), ({"BMM_DEBUG_NOSPLIT": "1"}, "dp", 3000, 37, 40, 400),
         ({}, "dp", 3000, 37, 40, 400), ({"BMM_DEBUG_GENERIC": "1"}, "dp", 1500, 37, 6, 200),
         ({"BMM_DEBUG_THREADS": "512"}, "collapsed", 3000, 37, 8, 400), ({"BMM_DEBUG_CUS": "4"}, "collapsed", 6000, 37, 8, 1500),
         ({"BMM_X_LAYOUT_INT32": "1"}, "dp", 3000, 37, 6, 400), ({"BMM_DEBUG_NOSELF": "1"}, "collapsed", 6000, 20, 3, 750),
         ({}, "collapsed", 6000, 20, 3, 750), ({}, "collapsed", 1500, 130, 4, 200)]
SWITCHES = ("BMM_DEBUG_NOSPLIT", "BMM_DEBUG_SPLIT", "BMM_DEBUG_GENERIC", "BMM_DEBUG_THREADS", "BMM_DEBUG_CUS", "BMM_X_LAYOUT_INT32",
            "BMM_DEBUG_NOSELF", "BMM_DEBUG_SMALL")


@pytest.mark.parametrize("env,sampler,N,P,K,batch", FORMS)
def test_every_form_all_ones_is_the_unarmed_chain_and_a_mask_is_the_same_chain_on_every_form(bmm, dbg_lib, env, sampler, N, P, K, batch):
    for k in SWITCHES:
        dbg_lib.delenv(k, raising=False)
    X, _ = _mixture(N, P, [0.2, 0.5, 0.8], 5)
    mixed = (np.arange(P) % 3 != 1).astype(np.uint8)
    mixed[:5] = 0
    W = bmm._capi.lib().bmm_spec_group_width_for(bmm._capi.SAMPLER_CODE[sampler], K, P)
    masks = dict(_masks(P, W), mixed=mixed)
    # the plain form of the shape first (no switch): what every other form must reproduce
    def run(m):
        with _chain(bmm, sampler, X, K, batch, 23) as c:
            if sampler == "dp":
                c.sweeps(1)
            if m is not None:
                c.set_features(m)
            c.sweeps(5)
            return _state(c), c.kernel_shape()
    plain_unarmed, _ = run(None)
    plain = {name: run(m)[0] for name, m in masks.items()}
    assert plain["mixed"] != plain_unarmed and plain["zeros"] != plain_unarmed and plain["group0"] != plain["middle"]
    for k, v in env.items():
        dbg_lib.setenv(k, v)
    unarmed, shape = run(None)
    assert unarmed == plain_unarmed          # (which form runs never changes a chain's values)
    for name, m in masks.items():            # every mask of the table test meets this form
        state, shape_m = run(m)
        print(env, sampler, name, "unarmed:", shape, "masked:", shape_m)
        assert state == plain[name], name
        assert not shape_m["builds_own_tables"]
    assert plain["ones"] == unarmed          # labels, counts and alpha, byte for byte


def test_theta_of_a_run_with_the_all_ones_mask_never_drawn_is_the_unarmed_run(bmm):
    """rho so close to 1 that no indicator is ever 0 in 5 sweeps: labels, theta and alpha of the whole route, byte for byte"""
    X, _ = _mixture(2000, 37, [0.2, 0.5, 0.8], 2)
    for fn, kw in ((bmm.gibbs_collapsed, dict(K=4)), (bmm.gibbs_dp, dict(maxK=12))):
        a = fn(X, 6, burnin=0, seed=5, **kw)
        b = fn(X, 6, burnin=0, seed=5, select_features=True, rho=1.0 - 2.0 ** -40, **kw)
        assert b["features"]["gamma"].all()
        for k in ("z", "theta", "alpha"):
            assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---------------------------------------------------------------- 2. the gamma-step
def _spread_labels(comp, K):
    """labels over all of 3 .. K: the rows of generating component 2 under label K, a cluster that lasts, every other
    row dealt out over 3 .. K - 1; labels 1 and 2 stay empty"""
    z = 3 + np.arange(len(comp)) % (K - 3)
    return np.where(comp == 2, K, z).astype(np.int32)


# K = 8 and 40: one trip of the lane walk `for k = lane; k <= K; k += 64` and of the integer butterfly's.  K = 63: the
# all-rows entry K on lane 63; 64: on lane 0 of the second trip; 65: one cluster and the entry in the second trip; 130:
# a third trip; 1024 (collapsed) and 1023 (dp): the most categories a chain takes, 17 trips.  P = 1, 32, 33, 64: one
# feature; a full mask word; a second workgroup that owns one feature (its other 15 waves leave the loop); two full
# words.  P = 2000: 63 workgroups, half a word in the last.
STEP_SHAPES = [("dp", 37, 8), ("dp", 130, 8), ("collapsed", 37, 40),
               ("collapsed", 37, 63), ("collapsed", 37, 64), ("collapsed", 37, 65), ("collapsed", 37, 130), ("collapsed", 37, 1024),
               ("dp", 37, 130), ("dp", 37, 1023),
               ("dp", 1, 8), ("dp", 32, 8), ("dp", 33, 8), ("dp", 64, 8), ("dp", 2000, 8)]


@pytest.mark.parametrize("sampler,P,K", STEP_SHAPES)
def test_thirty_steps_replayed_from_the_counts(bmm, sampler, P, K):
    wide = K >= 63                          # (the shapes of the lane walk: N = 2000 and labels spread over all of them)
    N, seed, rho = 2000 if wide else 300, 17, 0.3
    X, comp = _mixture(N, P, [0.2, 0.5, 0.8], 4)
    if P >= 6:
        X[:, 3] = X[:, 0]                   # (a feature that clusters as well as another)
        X[:, 5] = np.arange(N) % 2          # (and one that does not)
    initial = _spread_labels(comp, K) if wide else None
    batch = 250 if wide else 16             # (eight launches a sweep at N = 2000: a sweep over 1024 categories is slow)
    with _chain(bmm, sampler, X, K, batch, seed, labels=K - 2, initial=initial) as c:  # (collapsed: the last two labels stay empty)
        if wide and sampler == "dp":
            c.sweeps(1)                     # (seated: a DP chain takes labels from here on)
            c.set_labels(initial)
            c.sweeps(1)
        else:
            c.sweeps(2)
        c.set_feature_select(True, rho)
        acc, draws, empties, high, worst = np.zeros(P), np.zeros(P), 0, 0, 0.0
        for step in range(30):
            if step % 2:
                row = c.sweeps_features(1)[0]
            else:
                c.sweeps(1)
                row = None
            Nk, S = c.counts()
            empties += int(np.sum(Nk == 0) > 0)
            if K > 64 and high == step:     # a cluster in the second trip of the walk or later, in every step so far
                high += int(Nk[64:].sum() > 0)
            d = c.feature_step()
            assert d["sweep"] == 3 + step == c.sweep_index
            lam, mag, n = fsr.gamma_logit(Nk, S, BETA, GAMMA, rho, with_terms=True)
            u = np.array([fsr.fs_uniform(seed, f, d["sweep"]) for f in range(P)])
            np.testing.assert_array_equal(d["u"], u)
            # every lgamma_ within LGAMMA_ULPS ulps of max(1, |value|), the two logs within LOG_ULPS, n additions: as
            # tests/test_gpu_split_merge.py builds its bounds
            bound = 2.0 * (chk.LGAMMA_ULPS + n) * chk.EPS * (mag + n)
            err = np.abs(d["lambda"] - lam)
            print("step %d: Lambda worst %.3e (bound there %.3e)" % (step, err.max(), bound[np.argmax(err)]))
            assert np.all(err <= bound)
            worst = max(worst, float(np.max(err / bound)))
            # p and the draw, on the device's own numbers
            with np.errstate(over="ignore"):
                p_host = 1.0 / (1.0 + np.exp(-d["lambda"]))
            np.testing.assert_allclose(d["p"], p_host, rtol=8 * chk.EPS, atol=1e-300)
            np.testing.assert_array_equal(d["gamma"], (d["u"] < d["p"]).astype(np.uint8))
            np.testing.assert_array_equal(c.features(), d["gamma"])
            if row is not None:
                np.testing.assert_array_equal(row, d["gamma"])
            acc = acc + d["p"]
            draws = draws + d["gamma"]
        print("%s P=%d K=%d: worst Lambda error as a share of its bound %.3g" % (sampler, P, K, worst))
        sm = c.feature_summary()
        assert sm["n_folded"] == 30
        np.testing.assert_array_equal(sm["inclusion_rb"].view(np.uint64), (acc / 30.0).view(np.uint64))
        np.testing.assert_array_equal(sm["inclusion"], draws / 30.0)
        assert empties == 30                 # every state: unused labels (dp), empty clusters (collapsed)
        if K > 64:                           # (K = 64: index 64 of the walk is the all-rows entry itself)
            print("%s K=%d: a non-empty cluster at index >= 64 in the first %d of 30 steps" % (sampler, K, high))
            assert high == 30
        c.feature_reset()
        assert c.feature_summary()["n_folded"] == 0
        c.set_feature_select(False)
        before = c.features()
        c.sweeps(2)
        np.testing.assert_array_equal(c.features(), before)   # no step any more, the mask stays


def word_data():
    """N = 300, P = 64: every third feature is noise of one rate, so that both mask words come out mixed"""
    X, _ = _mixture(300, 64, [0.2, 0.5, 0.8], 4)
    X[:, ::3] = np.random.default_rng(0).random((300, 22)) < 0.4
    return X


def test_the_packed_word_the_next_sweep_reads_agrees_with_the_indicator_bytes(bmm):
    """The step stores the indicators twice: a byte each (what features() and feature_step() return) and packed, 32 to
    a word, with one plain store per workgroup (what the next sweep's tables read).  batch = N: the probabilities of
    the sweep behind a step are a pure function of the labels and of the word, as in section 1."""
    N, P, K, seed, rho = 300, 64, 8, 17, 0.3
    X = word_data()
    with _chain(bmm, "dp", X, K, N, seed) as c:
        c.sweeps(2)
        c.set_feature_select(True, rho)
        for step in range(3):
            c.sweeps(1)
            g = c.feature_step()["gamma"]
            np.testing.assert_array_equal(c.features(), g)
            assert 0 < g[:32].sum() < 32 and 0 < g[32:].sum() < 32, g   # both words mixed: a lost or misplaced bit shows
            z = c.labels() - 1
            got = c.sweep_probs()                                        # (one more sweep, and its own step behind it)
            want = fsr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, g, "dp")
            big = want > 1e-300
            rel = np.abs(got[big] - want[big]) / want[big]
            print("step %d: %d of 64 features in, worst relative %.2e" % (step, g.sum(), rel.max()))
            assert rel.max() <= 1e-12
            assert np.all(got[~big] <= 1e-300)
            # and the check can tell: under the mask with the two words exchanged the conditional is another one
            other = fsr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, np.concatenate([g[32:], g[:32]]), "dp")
            assert np.array_equal(g[32:], g[:32]) or np.abs(other - want).max() > 1e-6


# ---------------------------------------------------------------- 3. the joint chain against the exact posterior
def seven_by_four():
    X = np.zeros((7, 4), dtype=np.int32)
    X[:, :3] = seven_observations()
    X[:, 3] = [1, 1, 1, 1, 1, 1, 0]  # a constant-ish column
    return X


def test_batch_1_chain_samples_the_exact_joint_posterior(bmm):
    rho, n_batches = 0.3, 100
    X = seven_by_four()
    parts, ms, W = fsr.joint_posterior(X, ALPHA, BETA, GAMMA, rho)
    assert len(parts) == 877 and len(ms) == 16
    M = np.array(ms, dtype=np.float64)
    nclus = np.array(parts).max(axis=1) + 1
    out = bmm.gibbs_dp(np.asfortranarray(X), 30_001, alpha=ALPHA, beta=BETA, gamma=GAMMA, burnin=1, maxK=30, batch=1, seed=9,
                       select_features=True, rho=rho)
    g = out["features"]["gamma"].astype(np.float64)
    k_used = np.array([len(set(row)) for row in out["z"]])
    n = len(g) // n_batches * n_batches
    series = [("P(gamma_%d = 1)" % d, g[:n, d], float(W.sum(axis=0) @ M[:, d])) for d in range(4)]
    series += [("clusters=%d" % k, (k_used[:n] == k).astype(np.float64), float(W.sum(axis=1)[nclus == k].sum())) for k in range(1, 8)]
    for name, s, p in series:
        bm = s.reshape(n_batches, -1).mean(axis=1)
        se = max(bm.std(ddof=1) / np.sqrt(n_batches), np.sqrt(max(p * (1.0 - p), 0.0) / n))
        dev = abs(s.mean() - p)
        print("%-18s exact %.5f chain %.5f  dev/se %.2f" % (name, p, s.mean(), dev / se))
        assert dev <= 4.0 * se, (name, p, s.mean(), se)
    np.testing.assert_allclose(out["features"]["inclusion"], g.mean(axis=0), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(out["features"]["n_selected"], out["features"]["gamma"].sum(axis=1))


# ---------------------------------------------------------------- 4. planted noise
def planted(seed):
    """N = 4096, P = 37: twelve informative features under three well-separated components, 25 noise features of one rate each"""
    rng = np.random.default_rng(seed)
    N = 4096
    comp = rng.integers(3, size=N)
    rates = np.array([[0.9] * 4 + [0.1] * 8, [0.1] * 4 + [0.9] * 4 + [0.1] * 4, [0.1] * 8 + [0.9] * 4])
    noise = rng.uniform(0.1, 0.9, size=25)
    theta = np.concatenate([rates[comp], np.broadcast_to(noise, (N, 25))], axis=1)
    return np.asfortranarray((rng.random((N, 37)) < theta).astype(np.int32)), comp


PLANT_SEED = 1  # (the restatement over seeds 0 .. 7: DESIGN.md section 16 has the extremes)


def test_planted_noise_features_are_excluded_and_informative_ones_kept(bmm):
    """One data set, of a seed on which the restatement itself meets both bounds (six of the eight tried do; on the
    other two the posterior includes one chance-associated noise feature about a third of the time): noise features are
    usually excluded, not always."""
    X, comp = planted(PLANT_SEED)
    out = bmm.gibbs_collapsed(X, 60, 3, alpha=1.0, burnin=20, seed=3, initial_K=comp + 1, select_features=True, rho=0.5)
    inc, rb = out["features"]["inclusion"], out["features"]["inclusion_rb"]
    print("informative: min inclusion %.3f (rb %.3f); noise: max inclusion %.3f (rb %.3g)" % (inc[:12].min(), rb[:12].min(), inc[12:].max(), rb[12:].max()))
    assert out["features"]["n_folded"] == 40
    assert np.all(inc[:12] >= 0.9) and np.all(inc[12:] <= 0.1)


# ---------------------------------------------------------------- 5. reproducibility, the whole route, refusals
def test_same_seed_same_bits(bmm):
    X, _ = _mixture(1500, 45, [0.2, 0.5, 0.8], 6)
    X[:, ::2] = (np.random.default_rng(0).random((1500, 23)) < 0.4)
    runs = []
    for _ in range(2):
        with _chain(bmm, "dp", X, 20, None, 77) as c:
            c.set_feature_select(True, 0.5)
            tr = c.sweeps_features(8)
            sm, d = c.feature_summary(), c.feature_step()
            runs.append((tr.tobytes(), sm["inclusion"].tobytes(), sm["inclusion_rb"].tobytes(), d["lambda"].tobytes(), _state(c)))
    assert runs[0] == runs[1]
    assert 0 < np.frombuffer(runs[0][0], dtype=np.uint8).sum() < 8 * 45


@pytest.mark.parametrize("burnin", [0, 10])
def test_whole_route(bmm, burnin):
    N, P = 600, 24
    X, _ = _mixture(N, P, [0.2, 0.8], 12)
    X[:, 12:] = (np.random.default_rng(3).random((N, 12)) < 0.5)
    for out in (bmm.gibbs_collapsed(X, 40, 3, burnin=burnin, seed=4, select_features=True, rho=0.4),
                bmm.gibbs_dp(X, 40, burnin=burnin, maxK=12, seed=4, select_features=True, rho=0.4, relabel=True, stephens="device")
                if burnin else bmm.gibbs_dp(X, 40, burnin=burnin, maxK=12, seed=4, select_features=True, rho=0.4)):
        f = out["features"]
        S = 40 - burnin
        assert f["gamma"].shape == (S, P) and f["gamma"].dtype == np.uint8 and f["rho"] == 0.4
        first = 1 if burnin == 0 else 0     # without burn-in row 0 is the starting state: the initial mask, not folded
        if first:
            assert f["gamma"][0].all()
        assert f["n_folded"] == S - first
        np.testing.assert_array_equal(f["n_selected"], f["gamma"].sum(axis=1))
        np.testing.assert_allclose(f["inclusion"], f["gamma"][first:].mean(axis=0), rtol=0, atol=1e-15)
        assert np.all((f["inclusion_rb"] >= 0) & (f["inclusion_rb"] <= 1))
        assert f["inclusion"][:12].min() > f["inclusion"][12:].max()


def test_refusals(bmm):
    _capi = bmm._capi
    X, _ = _mixture(64, 8, [0.3, 0.7], 1)
    z0 = np.ones(64, dtype=np.int32)

    def code(call):
        with pytest.raises(_capi.BmmError) as e:
            call()
        assert len(str(e.value)) > 20       # says why
        return e.value.code

    for sampler in ("stickbreaking", "full"):
        with bmm.Chain(sampler, 64, 8, 5, alpha=1.0, seed=1) as c:
            assert code(lambda: c.set_feature_select(True, 0.5)) == 2          # BMM_E_UNSUPPORTED: they carry theta
            assert code(lambda: c.set_features(np.ones(8))) == 2
            c.set_shard(128, 0)
            assert code(lambda: c.set_feature_select(True, 0.5)) == 5          # BMM_E_STATE: sharded
    with bmm.Chain("dp", 64, 8, 5, alpha=1.0, seed=1) as c:
        assert code(lambda: c.set_feature_select(True, 0.5)) == 5              # no data: no rows to seat
        c.set_data(X)
        for rho in (0.0, 1.0, -0.5, 1.5, float("nan")):
            assert code(lambda: c.set_feature_select(True, rho)) == 1          # BMM_E_ARG
        assert code(lambda: c.sweeps_features(1)) == 5                         # not armed
        assert code(lambda: c.feature_step()) == 5                             # no step yet
        np.testing.assert_array_equal(c.features(), np.ones(8, dtype=np.uint8))
        c.set_feature_select(True, 0.5)
        c.sweeps(2)
        assert code(lambda: c.set_newdata(X[:4])) == 2
        assert code(lambda: c.set_loo(True)) == 2
        assert code(lambda: c.set_split_merge(1, 2)) == 2
        assert code(lambda: c.split_merge(1)) == 2
        c.sweeps(1)                                                            # and the chain stays usable
    with bmm.Chain("collapsed", 64, 8, 3, alpha=1.0, seed=1) as c:
        c.set_data(X)
        assert code(lambda: c.set_feature_select(True, 0.5)) == 5              # no labels yet
        c.set_initial_labels(z0)
        c.set_loo(True)
        assert code(lambda: c.set_feature_select(True, 0.5)) == 2              # armed the other way round
    with bmm.Chain("dp", 64, 8, 5, alpha=1.0, seed=1) as c:
        c.set_data(X)
        c.sweeps(1)
        c.set_split_merge(1, 2)
        assert code(lambda: c.set_feature_select(True, 0.5)) == 2
    with bmm.Chain("dp", 64, 8, 5, alpha=1.0, seed=1) as c:
        c.set_data(X)
        c.set_newdata(X[:4])
        assert code(lambda: c.set_features(np.ones(8))) == 2
    # a DP chain with beta != gamma does not exist (bmm_chain_create: BMM_E_ARG), so no resident call can meet one
    assert code(lambda: bmm.Chain("dp", 64, 8, 5, alpha=1.0, beta=0.5, gamma=0.7, seed=1)) == 1
    # a run armed for a sampler that carries theta: refused, and disarmed whatever it returned
    fs = bmm._Features(0.5, 8, 5)
    fs.arm()
    assert code(lambda: bmm.gibbs_stickbreaking(X, 5, 4, burnin=0, seed=1)) == 2
    bmm.gibbs_stickbreaking(X, 5, 4, burnin=0, seed=1)
    # ... and the C entry's own refusals of an armed run, past the wrapper's: armed by hand, then a call that does
    # not name select_features
    for kw in (dict(beta=0.5, gamma=0.7), dict(loo=True), dict(split_merge=1), dict(newdata=X[:4])):
        fs.arm()
        assert code(lambda: bmm.gibbs_dp(X, 5, maxK=5, burnin=0, seed=1, **kw)) == 2, kw
        assert "features" not in bmm.gibbs_dp(X, 5, maxK=5, burnin=0, seed=1)     # disarmed by the refused call
    fs.arm()
    assert code(lambda: bmm.gibbs_collapsed(X, 5, 3, burnin=0, seed=1, loo=True)) == 2
    for rho in (0.0, 1.0):
        bad = bmm._Features(rho, 8, 5)
        bad.arm()
        assert code(lambda: bmm.gibbs_dp(X, 5, maxK=5, burnin=0, seed=1)) == 1    # BMM_E_ARG
    with pytest.raises(ValueError):
        bmm.gibbs_dp(X, 10, maxK=5, select_features=True, chains=2)
