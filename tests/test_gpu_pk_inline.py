"""k_resample_pk settles the lanes its packed tier cannot prove inside the tile loop: right behind the draw the wave
runs the binary64 definition on each of them (pk_exact_count: the observation's words, label and uniform come from
the lane by readlane) and puts the count into that lane; certain and settled lanes then share one count_movers and
one pipelined store.  There is no queue and no pass behind the loop.

What the existing files do not reach is the MIX: with the packed tier deciding a handful of lanes are settled, with
BMM_DEBUG_DRAW_FALLBACK all of them are.  BMM_DEBUG_PK_DEFER_EVERY=n (test variant) treats every lane whose
observation index is a multiple of n as uncertain: n = 3 mixes every wave, n = 64 settles one lane of every full
wave.  Each shape runs those two ways and with everything deferred, eight sweeps from a random allocation, and must
give the oracle's z, theta and alpha bit for bit.  The test variant runs with BMM_DEBUG_NOSPLIT, BMM_DEBUG_NOSELF and
BMM_DEBUG_PK as in tests/test_gpu_score_pk.py, and every chain is asked whether its kernel is the packed one.

Shapes, the smallest at which each thing can go wrong:
  collapsed N=5000 P=100 K=20, batch 2500, one CU   40 chunks over 16 waves, a ragged last chunk: a lane is settled in
                                                    the middle of a wave's chunks while the next chunk's words and
                                                    label are already prefetched; the invalid lanes of the last chunk
                                                    are neither settled nor counted
  collapsed N=3000 P=5 K=3, batch 500               one lookup group, many short launches
  collapsed N=2500 P=33 K=12                        a field across a word boundary, from words read by readlane
  collapsed N=3000 P=37 K=32                        32 accumulators, two chunks of reads
  collapsed N=3000 P=61 K=32                        the width-4 image
  dp N=4000 P=24 maxK=12, batch 333                 odd category count; first sweep without labels (zo = -1); a
                                                    new-cluster draw made by the definition
  dp N=4000 P=24 maxK=30, batch 333                 the same at 31 of 32 accumulators

Counters of a two-sweep chain (bmm_dbg_pk_counts): draws == 2 N; everything deferred: deferred == draws.  With the
switch at n the kernel settles the selected lanes AND the lanes the packed tier leaves uncertain by itself, and the
test variant counts the latter apart where the switch did not select them (bmm_dbg_pk_unselected).  Asserted, exactly:
deferred - unselected == 2 (floor((N - 1) / n) + 1), the valid observation indices the switch selects -- an invalid
lane of a ragged last chunk that was settled or counted would break it -- and unselected <= the count of the same chain
with the switch unset.

BMM_DEBUG_PK_QUEUE sized the queue the kernel no longer has.  It is still accepted: a run with it set must equal the
oracle and settle exactly as many lanes as the run with nothing set."""
import ctypes

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi
from util import synth

pytestmark = pytest.mark.gpu

SWITCHES = ("DRAW_FALLBACK", "DRAW_NOEPS", "NOSPLIT", "NOSELF", "CUS", "PK_QUEUE", "PK_DEFER_EVERY", "NOPK", "PK")

# (sampler, N, P, K or maxK, batch, compute units the kernel choice sees or 0)
CASES = [("collapsed", 5000, 100, 20, 2500, 1), ("collapsed", 3000, 5, 3, 500, 0), ("collapsed", 2500, 33, 12, 2500, 0),
         ("collapsed", 3000, 37, 32, 700, 0), ("collapsed", 3000, 61, 32, 700, 0), ("dp", 4000, 24, 12, 333, 0),
         ("dp", 4000, 24, 30, 333, 0)]
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
    X = synth(N, P, 4, 13 * K + P)[0]
    z0 = np.random.default_rng(7).integers(1, K + 1, N).astype(np.int32)
    return X, z0


def _run(case):
    sampler, N, P, K, batch = case[:5]
    X, z0 = _data(case)
    if sampler == "dp":
        return bm.gibbs_dp(X, SWEEPS, burnin=0, maxK=K, seed=41, batch=batch)
    return bm.gibbs_collapsed(X, SWEEPS, K, burnin=0, seed=43, batch=batch, initial_K=z0)


def _want(oracle, case):
    sampler, N, P, K, batch = case[:5]
    X, z0 = _data(case)
    if sampler == "dp":
        return oracle.dp(X, SWEEPS, 0.0, 0.5, 0.5, 1, 1, 0, K, seed=41, batch=batch)
    return oracle.collapsed(X, z0, SWEEPS, K, 0.0, 0.5, 0.5, 1, 1, 0, seed=43, batch=batch)


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, what)


def _chain_counts(case):
    """(packed?, observations drawn, lanes settled by the definition, of them uncertain by themselves and not selected
    by the switch) of a two-sweep chain of the case's shape"""
    sampler, N, P, K, batch = case[:5]
    X, z0 = _data(case)
    with bm.Chain(sampler, N, P, K, batch=batch, seed=43) as c:
        c.set_data(X)
        if sampler != "dp":
            c.set_initial_labels(z0)
        c.sweeps(2)
        draws, deferred = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
        _capi.check(_capi.lib().bmm_dbg_pk_counts(c._h, ctypes.byref(draws), ctypes.byref(deferred)))
        unselected = ctypes.c_ulonglong(0)
        _capi.check(_capi.lib().bmm_dbg_pk_unselected(c._h, ctypes.byref(unselected)))
        return bool(_capi.lib().bmm_dbg_kernel_packed(c._h)), draws.value, deferred.value, unselected.value


@pytest.fixture(scope="module")
def wanted(oracle):
    return [_want(oracle, c) for c in CASES]


@pytest.mark.parametrize("how", ["every third lane deferred", "every 64th lane deferred", "everything deferred",
                                 "queue switch set"])
def test_variant_matches_the_oracle(wanted, dbg_lib, how):
    every = {"every third lane deferred": 3, "every 64th lane deferred": 64}.get(how, 0)
    for case, w in zip(CASES, wanted):
        N = case[1]
        base = dict(cus=case[5], NOSPLIT=1, NOSELF=1, PK=1)
        _set(dbg_lib, **base)
        packed, draws, natural, unselected = _chain_counts(case)
        assert unselected == natural, (case, natural, unselected)   # nothing selected: all of them
        assert packed and draws == 2 * N, (case, packed, draws)
        _set(dbg_lib, PK_DEFER_EVERY=every, DRAW_FALLBACK=how == "everything deferred",
             PK_QUEUE=8 if how == "queue switch set" else 0, **base)
        _same(_run(case), w, (how, case))
        packed, draws, deferred, unselected = _chain_counts(case)
        selected = 2 * ((N - 1) // every + 1) if every else 0
        print("%s %s: packed %s, %d draws, %d deferred (selected %d, uncertain and not selected %d, uncertain with the switch unset %d)"
              % (how, case, packed, draws, deferred, selected, unselected, natural))
        assert packed, (how, case)
        assert draws == 2 * N, (how, case, draws)
        if every:
            assert deferred - unselected == selected, (how, case, deferred, unselected, selected)
            assert unselected <= natural, (how, case, unselected, natural)
        elif how == "everything deferred":
            assert deferred == draws, (how, case, draws, deferred)
        else:
            assert deferred == natural, (how, case, deferred, natural)
