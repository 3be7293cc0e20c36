"""k_resample_pk's own-cluster score on the device: read per lookup group from Tm32 -- the "observation removed"
entries at the shape's group width, binary32, written by k_count_tables behind the packed image -- and summed in
binary32 inside the scoring loop; the exact pass reads the width-3 binary64 Tm from the global image.

Shapes are the smallest at which that path can go wrong and that tests/test_gpu_score_pk.py does not have:
  P = 1, K = 4              one group of one bit
  P = 128, K = 8            four words, 26 groups, the last three bits wide, two table chunks (120 + 8 features)
  P = 37, K = 32            32 accumulators in two chunks of reads, a field across words 0 and 1, P no multiple of the
                            width.  (The width rule gives this shape groups of FIVE -- read back below -- and no K up to
                            32 gives P = 37 groups of four: the whole binary64 image fits at five.  The next case is
                            the width-4 image.)
  P = 61, K = 32            the smallest P at which 32 labels take groups of four; 16 groups, the last one bit wide
  DP, maxK = 30, P = 24     N = 600 over 30 labels: many clusters of one row, so own rows with -inf in group 0, and
                            the new-label bookkeeping
  P = 100, K = 20, one CU   N = 64 x 16 x 3 + 5 in one launch: one workgroup, three chunks per wave and a ragged
                            last chunk -- the pipelined loop with the own read in it

Eight sweeps from a random allocation.  Every shape is run by the product library, by the test variant with the
packed tier deciding, with every observation deferred (BMM_DEBUG_DRAW_FALLBACK: the exact pass) and by the oracle:
identical z, theta and alpha.  The test variant runs with BMM_DEBUG_NOSPLIT, BMM_DEBUG_NOSELF and BMM_DEBUG_PK as in
tests/test_gpu_score_pk.py, and every chain is asked whether its kernel is the packed one.  With the packed tier
deciding fewer observations are deferred than drawn (bmm_dbg_pk_counts); the share is printed."""
import ctypes

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi
from util import synth

pytestmark = pytest.mark.gpu

SWITCHES = ("DRAW_FALLBACK", "DRAW_NOEPS", "NOSPLIT", "NOSELF", "CUS", "PK_QUEUE", "NOPK", "PK")

# (sampler, N, P, K or maxK, batch, compute units the kernel choice sees or 0, group width the rule gives)
CASES = [("collapsed", 2000, 1, 4, 500, 0, 5), ("collapsed", 3000, 128, 8, 1000, 0, 5), ("collapsed", 3000, 37, 32, 700, 0, 5),
         ("collapsed", 3000, 61, 32, 700, 0, 4), ("dp", 600, 24, 30, 100, 0, 5), ("collapsed", 64 * 16 * 3 + 5, 100, 20, 64 * 16 * 3 + 5, 1, 5)]
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
    sampler, N, P, K = case[:4]
    X = synth(N, P, 4, 11 * K + P)[0]
    z0 = np.random.default_rng(5).integers(1, K + 1, N).astype(np.int32)
    return X, z0


def _run(case):
    sampler, N, P, K, batch = case[:5]
    X, z0 = _data(case)
    if sampler == "dp":
        return bm.gibbs_dp(X, SWEEPS, burnin=0, maxK=K, seed=37, batch=batch)
    return bm.gibbs_collapsed(X, SWEEPS, K, burnin=0, seed=29, batch=batch, initial_K=z0)


def _want(oracle, case):
    sampler, N, P, K, batch = case[:5]
    X, z0 = _data(case)
    if sampler == "dp":
        return oracle.dp(X, SWEEPS, 0.0, 0.5, 0.5, 1, 1, 0, K, seed=37, batch=batch)
    return oracle.collapsed(X, z0, SWEEPS, K, 0.0, 0.5, 0.5, 1, 1, 0, seed=29, batch=batch)


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, what)


def _chain_counts(case):
    """(packed?, observations drawn, observations deferred) of a chain of the case's shape after SWEEPS sweeps"""
    sampler, N, P, K, batch = case[:5]
    X, z0 = _data(case)
    with bm.Chain(sampler, N, P, K, batch=batch, seed=29) as c:
        c.set_data(X)
        if sampler != "dp":
            c.set_initial_labels(z0)
        c.sweeps(SWEEPS)
        draws, deferred = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
        _capi.check(_capi.lib().bmm_dbg_pk_counts(c._h, ctypes.byref(draws), ctypes.byref(deferred)))
        return bool(_capi.lib().bmm_dbg_kernel_packed(c._h)), draws.value, deferred.value


@pytest.fixture(scope="module")
def wanted(oracle):
    return [_want(oracle, c) for c in CASES]


def test_the_shapes_take_the_widths_they_are_here_for():
    for case in CASES:
        sampler, N, P, K = case[:4]
        assert _capi.lib().bmm_spec_group_width_for(_capi.SAMPLER_CODE[sampler], K, P) == case[6], case


def test_product_matches_the_oracle(wanted):
    for case, w in zip(CASES, wanted):
        _same(_run(case), w, ("product", case))


@pytest.mark.parametrize("how", ["packed tier deciding", "everything deferred"])
def test_variant_matches_the_oracle(wanted, dbg_lib, how):
    for case, w in zip(CASES, wanted):
        _set(dbg_lib, cus=case[5], NOSPLIT=1, NOSELF=1, DRAW_FALLBACK=how.startswith("everything"), PK=1)
        _same(_run(case), w, (how, case))
        packed, draws, deferred = _chain_counts(case)
        print("%s %s: packed %s, %d draws, %d deferred (%.3f %%)" % (how, case, packed, draws, deferred, 100.0 * deferred / max(draws, 1)))
        assert packed, (how, case)
        assert draws == SWEEPS * case[1], (how, case, draws)
        if how == "packed tier deciding":
            assert deferred < draws, (case, draws, deferred)
        else:
            assert deferred == draws, (how, case, draws, deferred)
