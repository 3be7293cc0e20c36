"""k_resample_pk on the device: the plain bit-plane kernel with the scores summed in binary32 from the packed table
image (two categories per 64-bit lookup), the draw by draw_pk (bmm_spec.h), and the binary64 definition for the
observations whose draw the packed tier cannot prove -- queued in LDS and scored by the workgroup after its tile loop,
or on the spot by the wave when the queue is full.

Every shape is run by the product library, by the test variant as it comes (the packed tier deciding), with every
observation deferred (BMM_DEBUG_DRAW_FALLBACK), with every observation deferred and a queue of eight
(BMM_DEBUG_PK_QUEUE=8: the overflow path), and by the oracle: identical labels, theta and alpha.  Test-sized launches
would otherwise run two lanes per observation or build their own tables, forms that have no packed kernel, and the
packed kernel is handed out only to launches that give a wave four chunks or more, so the test variant runs with
BMM_DEBUG_NOSPLIT, BMM_DEBUG_NOSELF and BMM_DEBUG_PK (the packed kernel whatever the length of a launch) and every
chain is asked whether its kernel is the packed one (bmm_dbg_kernel_packed).  The product's packed kernel is held
to the oracle on one launch long enough for that rule.

The counters exist in the test variant only (bmm_dbg_pk_counts): the run with the packed tier deciding must have
deferred fewer observations than it drew.

Last, the band is what keeps the labels right: with a band of width zero (BMM_DEBUG_DRAW_NOEPS) a long chain on the
bundled K3 mixture leaves the oracle's per-sweep cluster sizes."""
import ctypes

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi
from util import load_dataset, synth

pytestmark = pytest.mark.gpu

SWITCHES = ("DRAW_FALLBACK", "DRAW_NOEPS", "NOSPLIT", "NOSELF", "CUS", "PK_QUEUE", "NOPK", "PK")

# (sampler, N, P, K or maxK, batch, compute units the kernel choice sees or 0): one group; a field across a word
# boundary; one CU -- 40 chunks over 16 waves, a ragged last chunk; 32 accumulators; the DP sampler with an odd
# category count in an even accumulator count (maxK = 12: 13 of 16, maxK = 30: 31 of 32) and its new-label
# bookkeeping in the exact pass
CASES = [("collapsed", 3000, 5, 3, 500, 0), ("collapsed", 2500, 33, 12, 2500, 0), ("collapsed", 5000, 100, 20, 2500, 1),
         ("collapsed", 3000, 64, 32, 700, 0), ("dp", 4000, 24, 12, 333, 0), ("dp", 4000, 24, 30, 333, 0)]
SWEEPS = 8
KEYS = ("z", "theta", "alpha")


def _set(mp, cus=0, **on):
    for k in SWITCHES:
        mp.delenv("BMM_DEBUG_" + k, raising=False)
    for k, v in on.items():
        if v:
            mp.setenv("BMM_DEBUG_" + k, str(int(v)))
    if cus:
        mp.setenv("BMM_DEBUG_CUS", str(cus))


def _data(case):
    sampler, N, P, K, _, _ = case
    X = synth(N, P, 4, 7 * K + P)[0]
    z0 = np.random.default_rng(3).integers(1, K + 1, N).astype(np.int32)
    return X, z0


def _run(case):
    sampler, N, P, K, batch, _ = case
    X, z0 = _data(case)
    if sampler == "dp":
        return bm.gibbs_dp(X, SWEEPS, burnin=0, maxK=K, seed=31, batch=batch)
    return bm.gibbs_collapsed(X, SWEEPS, K, burnin=0, seed=19, batch=batch, initial_K=z0)


def _want(oracle, case):
    sampler, N, P, K, batch, _ = case
    X, z0 = _data(case)
    if sampler == "dp":
        return oracle.dp(X, SWEEPS, 0.0, 0.5, 0.5, 1, 1, 0, K, seed=31, batch=batch)
    return oracle.collapsed(X, z0, SWEEPS, K, 0.0, 0.5, 0.5, 1, 1, 0, seed=19, batch=batch)


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, what)


def _chain_counts(case, sweeps):
    """(packed?, observations drawn, observations deferred) of a chain of the case's shape after `sweeps` sweeps"""
    sampler, N, P, K, batch, _ = case
    X, z0 = _data(case)
    with bm.Chain(sampler, N, P, K, batch=batch, seed=19) as c:
        c.set_data(X)
        if sampler != "dp":
            c.set_initial_labels(z0)
        c.sweeps(sweeps)
        draws, deferred = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
        _capi.check(_capi.lib().bmm_dbg_pk_counts(c._h, ctypes.byref(draws), ctypes.byref(deferred)))
        return bool(_capi.lib().bmm_dbg_kernel_packed(c._h)), draws.value, deferred.value


@pytest.fixture(scope="module")
def wanted(oracle):
    return [_want(oracle, c) for c in CASES]


def test_product_at_test_sizes_matches_the_oracle(wanted):
    """the product library at the shapes of this file: launches this short run k_resample, not the packed kernel -- a
    control for the runs of the test variant below, not coverage of k_resample_pk"""
    for case, w in zip(CASES, wanted):
        _same(_run(case), w, ("product", case))


def test_product_runs_the_packed_kernel_on_a_long_launch_and_matches_the_oracle(oracle, monkeypatch):
    """One launch long enough for plan_kernel's rule (a wave gets four chunks or more): N = batch = 4 x 256 CUs x 1024
    threads + 999, a ragged last chunk, K = 3, P = 5, three sweeps.  The product has no accessor for its kernel, so
    the test variant with no switch set -- the same plan_kernel on the same arguments -- says that the shape gets the
    packed kernel; the results compared are the product's."""
    N, P, K = 4 * 256 * 1024 + 999, 5, 3
    X = synth(N, P, 3, 77)[0]
    z0 = np.random.default_rng(5).integers(1, K + 1, N).astype(np.int32)
    got = bm.gibbs_collapsed(X, 4, K, burnin=0, seed=19, batch=N, initial_K=z0)
    want = oracle.collapsed(X, z0, 4, K, 0.0, 0.5, 0.5, 1, 1, 0, seed=19, batch=N)
    _same(got, want, "product, one long launch")
    from bmm_mcmc_amd import build
    if build.stale(build.LIB_DBG):
        build.build(debug_variant=True)
    monkeypatch.setattr(_capi, "_LIB", _capi.load(build.LIB_DBG))
    _set(monkeypatch)
    with bm.Chain("collapsed", N, P, K, batch=N, seed=19) as c:
        assert _capi.lib().bmm_dbg_kernel_packed(c._h) == 1, c.kernel_shape()


@pytest.mark.parametrize("how", ["packed tier deciding", "everything deferred", "everything deferred, queue of 8", "packed kernel off"])
def test_variant_matches_the_oracle(wanted, dbg_lib, how):
    for case, w in zip(CASES, wanted):
        _set(dbg_lib, cus=case[5], NOSPLIT=1, NOSELF=1, DRAW_FALLBACK=how.startswith("everything"),
             PK_QUEUE=8 if how.endswith("8") else 0, NOPK=how == "packed kernel off", PK=1)
        _same(_run(case), w, (how, case))
        packed, draws, deferred = _chain_counts(case, 2)
        sweep_draws = 2 * case[1]
        print("%s %s: packed %s, %d draws, %d deferred" % (how, case, packed, draws, deferred))
        if how == "packed kernel off":
            assert not packed and draws == 0 and deferred == 0, (case, packed, draws, deferred)
            continue
        assert packed, (how, case)
        assert draws == sweep_draws, (how, case, draws)
        if how == "packed tier deciding":
            assert deferred < draws, (case, draws, deferred)   # the packed tier has decided something
        else:
            assert deferred == draws, (how, case, draws, deferred)


# The zero-band wrong-draw rate per draw on K3_N1000_P5, measured on the host with draw_pk itself: tests/score_pk/pk_check.cpp,
# `pk_check rate X z 3 2000`, over 400 allocations the oracle's chain below passes through (every tenth of its first
# 4000 sweeps: 26 520 CDFs, 1.06e8 uniforms drawn within 1.5 bands of a CDF boundary and weighted by that window):
# 1.098e-8 with the exponential as the host rounds it, 1.434e-8 with it an ulp off either way; 0 wrong with the band.
ZERO_BAND_RATE = 1.098e-8


def test_a_band_of_width_zero_leaves_the_oracles_chain(oracle, dbg_lib):
    """K3_N1000_P5, K = 3, batches of 125, per-sweep cluster sizes (why sizes and not final labels:
    tests/test_gpu_draw_tiers.py).  With a band of width zero draw_pk answers for every draw that is not an exact
    binary32 tie, and a long enough chain must leave the oracle's.

    The chain is sized from ZERO_BAND_RATE so that ten wrong draws are expected: 10 / (1000 x 1.098e-8) = 910 000
    sweeps.  At one lookup group and three categories the binary32 CDF is within an ulp or two of the definition's and a
    uniform that close to an entry is nearly always an exact binary32 tie, which is never certain: hence the low rate
    and the long chain.  The oracle keeps every label of every sweep it returns (3.6 GB for this chain), so it runs
    the first 20 000 sweeps; the chain with the band in place must equal it there, and is the reference from there on
    (that it equals the oracle is what every other test of this file holds it to).

    Printed: the wrong draws expected, the sweeps whose sizes differ, and the episodes -- sweeps that differ after one
    that did not, each of which needs at least one wrong draw.  Measured on an MI355X: see profiles/r05/README.md."""
    X = load_dataset("K3_N1000_P5")
    N, P = X.shape
    K, batch, head = 3, 125, 20_000
    sweeps = int(np.ceil(10.0 / (N * ZERO_BAND_RATE) / 8)) * 8  # at least ten expected, a multiple of 8
    z0 = np.random.default_rng(11).integers(1, K + 1, N).astype(np.int32)
    z = oracle.collapsed(X, z0, head + 1, K, 0.0, 0.5, 0.5, 1, 1, 1, seed=23, batch=batch)["z"]
    want = np.stack([(z == k + 1).sum(axis=1) for k in range(K)], axis=1).astype(np.int32)
    del z

    def sizes():
        with bm.Chain("collapsed", N, P, K, batch=batch, seed=23) as c:
            assert _capi.lib().bmm_dbg_kernel_packed(c._h) == 1, c.kernel_shape()
            c.set_data(X)
            c.set_initial_labels(z0)
            return np.concatenate([c.sweeps_counts(sweeps // 8) for _ in range(8)])

    _set(dbg_lib, NOSELF=1, PK=1)
    with_band = sizes()
    assert np.array_equal(with_band[:head], want)
    _set(dbg_lib, NOSELF=1, PK=1, DRAW_NOEPS=1)
    differs = (sizes() != with_band).any(axis=1)
    ndiff = int(differs.sum())
    episodes = int(differs[0]) + int((differs[1:] & ~differs[:-1]).sum())
    print("zero band, %d sweeps of %d draws: %.1f wrong draws expected from the host rate; %d sweeps differ from the chain "
          "with the band, in %d episodes" % (sweeps, N, sweeps * N * ZERO_BAND_RATE, ndiff, episodes))
    assert ndiff > 0, "a band of width zero gave the oracle's chain: the hook does not exercise the ambiguity check"
