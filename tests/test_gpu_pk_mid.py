"""k_resample_pk settles a lane its packed tier cannot prove in two steps: first the middle tier (pk_mid_count: the
binary32 entries of the LDS image summed in binary64, draw_mid of bmm_spec.h), and only where that is not certain either
the binary64 definition (pk_exact_count).  A lane the middle tier settles takes the middle tier's count, which is proven
to be the definition's, so every chain must still be the oracle's bit for bit, and the same chain with the middle tier
switched off (BMM_DEBUG_PK_NOMID: the definition settles every uncertain lane, as before there was a middle tier).

The test variant runs with BMM_DEBUG_PK, BMM_DEBUG_NOSPLIT, BMM_DEBUG_NOSELF and BMM_DEBUG_CUS=1 as in
tests/test_gpu_chunks.py and tests/test_gpu_pk_inline.py: test-sized batches reach the 1024-thread packed forms with
several chunks per wave.  Shapes, the smallest at which each thing can go wrong:
  collapsed K=20 P=100 N=3*1024+17     C5's form: 49 chunks over 16 waves, three and four to a wave, a ragged last one
  collapsed K=2  P=100                 two of four accumulators live, the padding categories impossible; groups of five
  collapsed K=32 P=37 / P=61           every lane of the scan a category; groups of five / groups of four
  collapsed K=3  P=1                   one group: less than a first round, the rolled reads alone
  collapsed K=11 P=128                 26 groups: the compile-time round and a rolled one, a field across every word boundary
  dp maxK=12 P=24 N=2003, batch 333    the oracle's DP chain takes no initial allocation: it starts unassigned (zo = -1)
                                       and its first sweep doubles its launches from one observation, so the first rows
                                       sit in clusters of one and two rows and are drawn against own-cluster entries at
                                       their edge (-inf for a cluster of one); rows planted far from every component keep
                                       small clusters alive, and new-cluster draws are made by either tier.  Asserted
                                       on the trace: after the first sweep one cluster holds one row and one holds two
                                       (their rows meet own entries at the edge in the second), and several labels are
                                       in use, each opened by a new-cluster draw
(K = 2 at groups of four does not exist: the width rule gives four only where the tables of five do not fit, which two
categories never reach -- asserted below through bmm_spec_group_width_for.)

Each shape runs three ways, two sweeps each: as it comes; BMM_DEBUG_PK_DEFER_EVERY=3, every third lane through the
middle tier; BMM_DEBUG_DRAW_FALLBACK with BMM_DEBUG_PK_MID_FAIL_EVERY=5, every lane through the middle tier and every
fifth of them on to the definition, so that both settle tiers meet in one wave.

Counters of a two-sweep chain (bmm_dbg_pk_counts, bmm_dbg_pk_tier_counts): mid_tried == deferred,
exact_runs == mid_tried - mid_settled; with NOMID mid_tried == 0 and exact_runs == deferred; with DEFER_EVERY=3 on the
K = 20 shape mid_settled > 0 and exact_runs < mid_tried; with MID_FAIL_EVERY=5 exact_runs is at least the number of
valid observation indices that are multiples of five."""
import ctypes

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi
from util import synth

pytestmark = pytest.mark.gpu

SWITCHES = ("DRAW_FALLBACK", "DRAW_NOEPS", "NOSPLIT", "NOSELF", "CUS", "PK_DEFER_EVERY", "PK_NOMID", "PK_MID_FAIL_EVERY",
            "PK_NOPIPE", "NOPK", "PK")

# (sampler, N, P, K or maxK, batch, group width the rule gives)
CASES = [("collapsed", 3 * 1024 + 17, 100, 20, 3 * 1024 + 17, 5), ("collapsed", 2500, 100, 2, 2500, 5),
         ("collapsed", 3000, 37, 32, 1500, 5), ("collapsed", 3000, 61, 32, 1500, 4), ("collapsed", 2500, 1, 3, 2500, 5),
         ("collapsed", 2500, 128, 11, 2500, 5), ("dp", 2003, 24, 12, 333, 5)]
K20 = CASES[0]
SWEEPS = 3   # rows of the trace: the start and two sweeps
KEYS = ("z", "theta", "alpha")
WAYS = {"as it comes": {}, "every third lane deferred": {"PK_DEFER_EVERY": 3},
        "everything deferred, every fifth past the middle tier": {"DRAW_FALLBACK": 1, "PK_MID_FAIL_EVERY": 5}}


def _set(mp, **on):
    for k in SWITCHES:
        mp.delenv("BMM_DEBUG_" + k, raising=False)
    for k, v in dict(on, NOSPLIT=1, NOSELF=1, PK=1, CUS=1).items():
        if v:
            mp.setenv("BMM_DEBUG_" + k, str(int(v)))


def _data(case):
    sampler, N, P, K = case[:4]
    X = synth(N, P, 4, 17 * K + P)[0]
    if sampler == "dp":
        # rows far from every component, alone and in pairs: clusters of one and two rows that last
        X = np.array(X, order="F")
        for r, row in enumerate((0, 1, 2, 2, 3, 3)):
            X[7 + 311 * r, :] = [(j * (row + 2) // 3 + row) % 2 for j in range(P)]
    z0 = np.random.default_rng(11).integers(1, K + 1, N).astype(np.int32)
    return X, z0


def _run(case):
    sampler, N, P, K, batch = case[:5]
    X, z0 = _data(case)
    if sampler == "dp":
        return bm.gibbs_dp(X, SWEEPS, burnin=0, maxK=K, seed=47, batch=batch)
    return bm.gibbs_collapsed(X, SWEEPS, K, burnin=0, seed=53, batch=batch, initial_K=z0)


def _want(oracle, case):
    sampler, N, P, K, batch = case[:5]
    X, z0 = _data(case)
    if sampler == "dp":
        return oracle.dp(X, SWEEPS, 0.0, 0.5, 0.5, 1, 1, 0, K, seed=47, batch=batch)
    return oracle.collapsed(X, z0, SWEEPS, K, 0.0, 0.5, 0.5, 1, 1, 0, seed=53, batch=batch)


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, what)


def _counts(case):
    """(packed?, draws, deferred, mid_tried, mid_settled, exact_runs) of a two-sweep chain of the case's shape"""
    sampler, N, P, K, batch = case[:5]
    X, z0 = _data(case)
    L = _capi.lib()
    with bm.Chain(sampler, N, P, K, batch=batch, seed=53) as c:
        c.set_data(X)
        if sampler != "dp":
            c.set_initial_labels(z0)
        c.sweeps(2)
        v = [ctypes.c_ulonglong(0) for _ in range(5)]
        _capi.check(L.bmm_dbg_pk_counts(c._h, ctypes.byref(v[0]), ctypes.byref(v[1])))
        _capi.check(L.bmm_dbg_pk_tier_counts(c._h, ctypes.byref(v[2]), ctypes.byref(v[3]), ctypes.byref(v[4])))
        return (bool(L.bmm_dbg_kernel_packed(c._h)),) + tuple(x.value for x in v)


@pytest.fixture(scope="module")
def wanted(oracle):
    return [_want(oracle, c) for c in CASES]


def test_the_width_rule_gives_the_shapes_their_widths(dbg_lib):
    L = _capi.lib()
    for sampler, N, P, K, batch, gw in CASES:
        assert L.bmm_spec_group_width_for(_capi.SAMPLER_CODE[sampler], K, P) == gw, (sampler, K, P)
    assert L.bmm_spec_group_width_for(0, 2, 128) == 5   # two categories never get groups of four


@pytest.mark.parametrize("way", list(WAYS))
def test_chains_match_the_oracle_and_the_chain_without_the_middle_tier(wanted, dbg_lib, way):
    for case, w in zip(CASES, wanted):
        N = case[1]
        _set(dbg_lib, **WAYS[way])
        got = _run(case)
        _same(got, w, (way, case, "oracle"))
        if case[0] == "dp":
            sizes = np.bincount(got["z"][1], minlength=case[3] + 1)[1:]
            assert (sizes == 1).any() and (sizes == 2).any() and (sizes > 0).sum() >= 3, (way, case, sizes)
        packed, draws, deferred, tried, settled, exact = _counts(case)
        print("%s %s: %d draws, %d deferred, middle tier tried %d settled %d, definition %d" % (way, case, draws, deferred, tried,
                                                                                               settled, exact))
        assert packed and draws == 2 * N, (way, case, packed, draws)
        assert tried == deferred, (way, case, tried, deferred)
        assert exact == tried - settled, (way, case, exact, tried, settled)
        if "DRAW_FALLBACK" in WAYS[way]:
            assert deferred == draws, (way, case, deferred, draws)
            assert exact >= 2 * ((N - 1) // 5 + 1), (way, case, exact)
        if "PK_DEFER_EVERY" in WAYS[way]:
            assert deferred >= 2 * ((N - 1) // 3 + 1), (way, case, deferred)
        if case is K20 and WAYS[way]:
            assert settled > 0 and exact < tried, (way, case, settled, exact, tried)
        _set(dbg_lib, PK_NOMID=1, **WAYS[way])
        _same(_run(case), got, (way, case, "without the middle tier"))
        packed, draws0, deferred0, tried0, settled0, exact0 = _counts(case)
        assert packed and draws0 == draws and deferred0 == deferred, (way, case, draws0, deferred0)
        assert tried0 == 0 and settled0 == 0 and exact0 == deferred0, (way, case, tried0, settled0, exact0)
