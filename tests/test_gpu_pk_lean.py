"""k_resample_pk with a lean steady state: an observation is a 32-bit offset from the launch's first (the batch's
first observation is folded into the base pointers on the host), the blocks beside the steady state -- the definition
for an uncertain lane, the DP's books, the movers, the flush -- re-read their arguments from the kernel argument
segment where they run, the draw works on pairs of scores (pk_draw2) and the Philox key of a launch whose
observations all lie below 2^32 is a scalar.  None of this may change a label.

The test variant runs with BMM_DEBUG_NOSPLIT, BMM_DEBUG_NOSELF, BMM_DEBUG_PK and BMM_DEBUG_CUS=1 as in
tests/test_gpu_pk_inline.py, and every chain is asked whether its kernel is the packed one.

Oracle chains, z, theta and alpha bit for bit, eight sweeps:
  collapsed N=5000 P=100 K=20, batch 2500     40 chunks over 16 waves, a ragged last chunk, the second launch of a
                                              sweep with lo > 0 (folded bases, the draw's counter base)
  collapsed N=1500 P=128 K=4                  the largest P the packed kernel takes (asked of the library): four
                                              words, the 4-accumulator form
  collapsed N=2500 P=33 K=12                  a field across a word boundary, two words
  collapsed N=3000 P=61 K=32                  width 4, 16 pair accumulators in two read chunks
  dp N=4000 P=24 maxK=12 and 30, batch 333    first sweep with zo = -1, the new-cluster branch (its books are now
                                              made where it is drawn), many lo offsets
Both Philox forms: BMM_DEBUG_PK_GENKEY forces the general, per-lane key for a whole run; that run and the default run
(the scalar key: every index of these launches is below 2^32) equal the oracle at the first shape.
Mixed waves: with BMM_DEBUG_PK_DEFER_EVERY=3 the first shape still equals the oracle -- every wave runs the
definition on arguments it re-read, between chunks of the steady state.

The draw: k_test_pk_draw (test variant) runs the kernel's draw and bmm_spec.h's draw_pk on the same scores and
uniforms (a kernel each, so that the compiler cannot share work between them): random scores down to -3000, some
categories -inf, one row all -inf, one row with a NaN, u including 0 and 1 - 2^-52 and uniforms placed on the
boundaries of the row's CDF, at 4, 12, 20 and 32 accumulators.  Counts and verdicts are equal for every row."""
import ctypes

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi
from util import synth

pytestmark = pytest.mark.gpu

SWITCHES = ("DRAW_FALLBACK", "DRAW_NOEPS", "NOSPLIT", "NOSELF", "CUS", "PK_QUEUE", "PK_DEFER_EVERY", "PK_GENKEY", "NOPK",
            "PK")
SWEEPS = 8
KEYS = ("z", "theta", "alpha")


def _largest_packed_p(K):
    f = _capi.lib().bmm_spec_pk_image_bytes
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_int] * 4
    g = _capi.lib().bmm_spec_group_width_for
    return max(P for P in range(1, 129) if f(0, K, P, g(0, K, P)) > 0)


def _cases():
    # (sampler, N, P, K or maxK, batch)
    return [("collapsed", 5000, 100, 20, 2500), ("collapsed", 1500, _largest_packed_p(4), 4, 1500),
            ("collapsed", 2500, 33, 12, 2500), ("collapsed", 3000, 61, 32, 700), ("dp", 4000, 24, 12, 333),
            ("dp", 4000, 24, 30, 333)]


def _set(mp, **on):
    for k in SWITCHES:
        mp.delenv("BMM_DEBUG_" + k, raising=False)
    for k, v in dict(NOSPLIT=1, NOSELF=1, PK=1, CUS=1, **on).items():
        if v:
            mp.setenv("BMM_DEBUG_" + k, str(int(v)))


def _data(case):
    sampler, N, P, K = case[:4]
    X = synth(N, P, 4, 11 * K + P)[0]
    z0 = np.random.default_rng(5).integers(1, K + 1, N).astype(np.int32)
    return X, z0


def _run(case):
    sampler, N, P, K, batch = case
    X, z0 = _data(case)
    if sampler == "dp":
        return bm.gibbs_dp(X, SWEEPS, burnin=0, maxK=K, seed=47, batch=batch)
    return bm.gibbs_collapsed(X, SWEEPS, K, burnin=0, seed=53, batch=batch, initial_K=z0)


def _want(oracle, case):
    sampler, N, P, K, batch = case
    X, z0 = _data(case)
    if sampler == "dp":
        return oracle.dp(X, SWEEPS, 0.0, 0.5, 0.5, 1, 1, 0, K, seed=47, batch=batch)
    return oracle.collapsed(X, z0, SWEEPS, K, 0.0, 0.5, 0.5, 1, 1, 0, seed=53, batch=batch)


def _packed(case):
    sampler, N, P, K, batch = case
    with bm.Chain(sampler, N, P, K, batch=batch, seed=53) as c:
        return bool(_capi.lib().bmm_dbg_kernel_packed(c._h))


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, what)


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture(scope="module")
def wanted(oracle, cases):
    return [_want(oracle, c) for c in cases]


def test_the_largest_p_is_four_words(cases):
    assert cases[1][2] > 96, cases[1]


@pytest.mark.parametrize("i", range(6))
def test_variant_matches_the_oracle(wanted, cases, dbg_lib, i):
    _set(dbg_lib)
    assert _packed(cases[i]), cases[i]
    _same(_run(cases[i]), wanted[i], cases[i])


@pytest.mark.parametrize("how", ["general key form", "every third lane deferred",
                                 "general key form, every third lane deferred"])
def test_first_shape_matches_the_oracle(wanted, cases, dbg_lib, how):
    _set(dbg_lib, PK_GENKEY="general" in how, PK_DEFER_EVERY=3 if "third" in how else 0)
    assert _packed(cases[0]), how
    _same(_run(cases[0]), wanted[0], how)


def _draw_rows(KT, rng):
    n = 4096
    sc = (-3000.0 * rng.random((n, KT)) ** 3).astype(np.float32)   # many near 0, some down to -3000
    close = rng.random(n) < 0.5                                    # rows whose scores lie within a few units
    sc[close] = (sc[close, :1] - 4.0 * rng.random((int(close.sum()), KT))).astype(np.float32)
    sc[rng.random((n, KT)) < 0.1] = -np.inf
    sc[0, :] = -np.inf
    sc[1, KT // 2] = np.nan
    sc[2, :] = 0.0
    u = rng.random(n)
    u[:8:2] = 0.0
    u[1:8:2] = 1.0 - 2.0 ** -52
    u[8], u[9] = 0.0, 1.0 - 2.0 ** -52
    # uniforms right at a boundary of the row's CDF: ties and near-ties, where the verdict must be "uncertain"
    w = np.exp((sc[10:600].astype(np.float64).T - np.nanmax(sc[10:600], axis=1)).T)
    cdf = np.cumsum(np.nan_to_num(w), axis=1)
    k = rng.integers(0, KT, 590)
    with np.errstate(invalid="ignore", divide="ignore"):
        edge = cdf[np.arange(590), k] / cdf[:, -1]
    u[10:600] = np.clip(np.nan_to_num(edge, nan=0.5), 0.0, 1.0 - 2.0 ** -52)
    return np.ascontiguousarray(sc), np.ascontiguousarray(u)


@pytest.mark.parametrize("KT", [4, 12, 20, 32])
def test_the_kernels_draw_is_draw_pk(dbg_lib, KT):
    sc, u = _draw_rows(KT, np.random.default_rng(100 + KT))
    n = sc.shape[0]
    f = _capi.lib().bmm_dbg_pk_draw
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                  ctypes.c_int64, ctypes.c_void_p]
    for G in (1, 20, 32):
        kernel, spec = np.full((n, 2), -7, dtype=np.int32), np.full((n, 2), -7, dtype=np.int32)
        _capi.check(f(0, KT, 0, sc.ctypes.data, u.ctypes.data, G, n, kernel.ctypes.data))
        _capi.check(f(0, KT, 1, sc.ctypes.data, u.ctypes.data, G, n, spec.ctypes.data))
        print("KT %d G %d: %d of %d rows certain, counts %d..%d" % (KT, G, int(spec[:, 1].sum()), n, spec[:, 0].min(),
                                                                     spec[:, 0].max()))
        assert np.array_equal(kernel[:, 0], spec[:, 0]), (KT, G, np.flatnonzero(kernel[:, 0] != spec[:, 0])[:8])
        assert np.array_equal(kernel[:, 1], spec[:, 1]), (KT, G, np.flatnonzero(kernel[:, 1] != spec[:, 1])[:8])
        assert spec[0, 1] == 0 and spec[1, 1] == 0, (KT, G, spec[:2])   # all -inf, and a NaN: never certain
        assert 0 < spec[:, 1].sum() < n, (KT, G)                        # both verdicts occur
        assert 0 <= spec[:, 0].min() and spec[:, 0].max() <= KT, (KT, G)
