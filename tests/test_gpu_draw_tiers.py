"""The two-tier draw of k_resample on the device.  The plain one-lane kernels take the draw's count from binary32
weights wherever that is proven to be the definition's count, and from the binary64 definition otherwise
(bmm_spec.h, draw_tier1).  The same chains are run three ways -- the product library, the test variant with every
wave sent to the definition (BMM_DEBUG_DRAW_FALLBACK), and the oracle -- and must be identical: labels, theta, alpha.

Test-sized launches of 16 to 32 accumulators run two lanes per observation, a form that has no binary32 tier; the
one-lane kernels of those counts (what the benchmark's long launches run) are reached through BMM_DEBUG_NOSPLIT, so
the test variant runs every shape with it and without it.

Last, the band around the CDF entries is what keeps the labels right: with a band of width zero
(BMM_DEBUG_DRAW_NOEPS, test variant only) a long chain on the bundled overlapping K3 mixture must LEAVE the oracle's
chain."""
import numpy as np
import pytest

import bmm_mcmc_amd as bm
from util import load_dataset, synth

pytestmark = pytest.mark.gpu

SWITCHES = ("BMM_DEBUG_DRAW_FALLBACK", "BMM_DEBUG_DRAW_NOEPS", "BMM_DEBUG_NOSPLIT")


def _set(mp, **on):
    for k in SWITCHES:
        mp.delenv(k, raising=False)
    for k, v in on.items():
        if v:
            mp.setenv("BMM_DEBUG_" + k, "1")


def _z0(N, K, seed):
    return np.random.default_rng(seed).integers(1, K + 1, N).astype(np.int32)


def _same(got, want, keys, what):
    for k in keys:
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, what)


# (N, P, K, batch): own-cluster tables in LDS, one word of bit planes to four; 4 to 64 accumulators
COLLAPSED = [(3000, 5, 3, 500), (5000, 20, 3, 625), (4000, 50, 20, 512), (3000, 100, 20, 700), (2500, 33, 12, 2500),
             (2000, 40, 40, 500), (1500, 20, 64, 1500)]


def _data(shape):
    N, P, K, _ = shape
    return synth(N, P, 4, 7 * K + P)[0], _z0(N, K, 3)


def _collapsed(shape):
    X, z0 = _data(shape)
    return bm.gibbs_collapsed(X, 8, shape[2], burnin=0, seed=19, batch=shape[3], initial_K=z0)


def test_product_forced_fallback_and_oracle_run_the_same_chains(oracle, monkeypatch):
    keys = ("z", "theta", "alpha")
    # the product library first (no switch reaches it), then the test variant in its place
    product = [_collapsed(s) for s in COLLAPSED]
    Xd, _, _, _ = synth(4000, 24, 5, 9)
    product_dp = bm.gibbs_dp(Xd, 8, burnin=0, maxK=12, seed=31, batch=333)
    rng = np.random.default_rng(1)
    pi0 = rng.dirichlet(np.ones(10))
    th0 = rng.random((10, 50))
    Xs, _, _, _ = synth(4000, 50, 4, 3)
    product_sb = bm.gibbs_stickbreaking(Xs, 6, 10, burnin=0, seed=8, initial_pi=pi0, initial_theta=th0)

    want = []
    for s in COLLAPSED:
        X, z0 = _data(s)
        want.append(oracle.collapsed(X, z0, 8, s[2], 0.0, 0.5, 0.5, 1, 1, 0, seed=19, batch=s[3]))
    want_dp = oracle.dp(Xd, 8, 0.0, 0.5, 0.5, 1, 1, 0, 12, seed=31, batch=333)
    want_sb = oracle.stickbreaking(Xs, pi0, th0, 6, 10, 0.0, 0.5, 0.5, 1, 1, 0, seed=8)
    for s, g, w in zip(COLLAPSED, product, want):
        _same(g, w, keys, ("product", s))
    _same(product_dp, want_dp, keys, "product dp")
    _same(product_sb, want_sb, keys + ("pi",), "product stick-breaking")

    from bmm_mcmc_amd import _capi, build
    if build.stale(build.LIB_DBG):
        build.build(debug_variant=True)
    monkeypatch.setattr(_capi, "_LIB", _capi.load(build.LIB_DBG))
    for nosplit in (False, True):
        for fallback in (False, True):
            _set(monkeypatch, NOSPLIT=nosplit, DRAW_FALLBACK=fallback)
            what = "test variant, one lane forced %s, definition forced %s" % (nosplit, fallback)
            for s, w in zip(COLLAPSED, want):
                _same(_collapsed(s), w, keys, (what, s))
            _same(bm.gibbs_dp(Xd, 8, burnin=0, maxK=12, seed=31, batch=333), want_dp, keys, what)
            _same(bm.gibbs_stickbreaking(Xs, 6, 10, burnin=0, seed=8, initial_pi=pi0, initial_theta=th0), want_sb,
                  keys + ("pi",), what)


def test_a_band_of_width_zero_leaves_the_oracles_chain(oracle, dbg_lib):
    """K3_N1000_P5 (three overlapping components, five features: every draw has two CDF entries well inside (0, tot)),
    K = 3, batches of 125.  With no band tier 1 answers for every draw that is not an exact tie, and is wrong whenever
    u * tot lies nearer to a CDF entry than the binary32 weights are good for.  How often that is was measured on the
    host with this very function (random scores of unit spread, random u): 5 in 2e8 draws at K = 3 (2.5e-8).  2e5 sweeps
    of 1000 observations are 2e8 draws, five such draws expected.

    What is compared is the cluster sizes after EVERY sweep, not the final labels: two chains driven by the same
    uniforms coalesce -- the oracle started from two allocations that differ in one label ends on identical labels
    after one sweep -- so a label drawn wrongly is gone from the state a sweep later (final labels after 3e5 and 4e5
    sweeps at K = 3 and 1.5e5 at K = 20 were the oracle's with and without the band), but it moves one observation
    between two clusters in the sweep it happens in.  With the band in place every sweep has the oracle's sizes
    (measured on an MI355X: 0 of the 2e5 sweeps differ with the band, 89 with a band of width zero)."""
    X = load_dataset("K3_N1000_P5")
    N, P = X.shape
    K, sweeps, batch = 3, 200_000, 125
    z0 = _z0(N, K, 11)
    z = oracle.collapsed(X, z0, sweeps + 1, K, 0.0, 0.5, 0.5, 1, 1, 1, seed=23, batch=batch)["z"]
    assert z.shape == (sweeps, N)
    want = np.stack([(z == k + 1).sum(axis=1) for k in range(K)], axis=1).astype(np.int32)
    del z

    def sizes():
        with bm.Chain("collapsed", N, P, K, batch=batch, seed=23) as c:
            assert c.kernel_shape()["lanes_per_observation"] == 1, c.kernel_shape()
            c.set_data(X)
            c.set_initial_labels(z0)
            return np.concatenate([c.sweeps_counts(sweeps // 8) for _ in range(8)])

    _set(dbg_lib)
    with_band = sizes()
    _set(dbg_lib, DRAW_NOEPS=True)
    without = sizes()
    ndiff = int((without != want).any(axis=1).sum())
    print("sweeps of %d whose cluster sizes differ from the oracle's: with the band %d, with a band of width zero %d"
          % (sweeps, int((with_band != want).any(axis=1).sum()), ndiff))
    assert np.array_equal(with_band, want)
    assert ndiff > 0, "a band of width zero gave the oracle's chain: the hook does not exercise the ambiguity check"
