"""Greedy search for the clustering point estimate (include/bmm_mcmc.h "greedy search"): what can
be checked without a GPU.  The restatement tests/partition_search_ref.py against the definitions it rests on (the
scores against differences of full totals, passes that never raise the total, converged results against a brute
force), and the library's plan and refusals, which touch no device."""
import ctypes as C
import math

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi
import partition_ref as pr
import partition_search_ref as ref

NEW = ["bmm_device_partition_search", "bmm_partition_search_plan", "bmm_set_partition_search"]
SMALL = [c for c in ref.CASES if c[1] <= 1000]


def test_entry_points_are_exported():
    L = _capi.lib()
    for s in NEW:
        assert s in _capi.SYMBOLS
        getattr(L, s)
    assert bm.PARTITION_SEARCH_MAX_K == 64
    assert "partition_search" in bm.__all__ and "partition_search_plan" in bm.__all__


def _state_with_an_empty_slot_and_a_singleton(seed):
    """Kc = 5 draws, Ka = 7 slots: slot 6 (0-based) empty, row 0 alone in slot 5"""
    z, _ = ref.make_trace(5, 120, 7, ref.EPS, seed)
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 6, 120)
    c[0] = 6
    return z, c


@pytest.mark.parametrize("criterion", ["binder", "vi"])
def test_score_differences_are_differences_of_totals(criterion):
    z, c = _state_with_an_empty_slot_and_a_singleton(3)
    st = ref.State(z, c, 5, 7)
    assert st.n[6] == 0 and st.n[5] == 1
    rows = [0] + list(np.random.default_rng(4).choice(np.arange(1, 120), 19, replace=False))
    for i in rows:
        g = st.scores(i, criterion)
        a0 = st.c[i]
        # an empty slot, and the own cluster of a row that is alone, score 0 by the formula
        assert g[6] == 0
        if i == 0:
            assert g[5] == 0 and a0 == 5
        base = st.total(criterion)
        for a in range(7):
            moved = ref.State(z, np.where(np.arange(120) == i, a + 1, st.c + 1), 5, 7)
            diff = moved.total(criterion) - base
            if criterion == "binder":
                # binder2 counts ordered pairs: the row's move changes it by twice the score difference
                assert 2 * (g[a] - g[a0]) == diff
                # ... and the totals are those of partition_ref, draw by draw (labels of c up to 7: a 7-wide table)
                assert base == sum(pr.binder2(st.c + 1, z[t], 7) for t in range(7))
            else:
                assert abs((g[a] - g[a0]) - diff) <= 1e-9 * max(1.0, abs(base))


def test_vi_total_is_the_sum_of_partition_ref_distances():
    z, c = _state_with_an_empty_slot_and_a_singleton(5)
    st = ref.State(z, c, 5, 7)
    want = math.fsum(pr.vi(c, z[t], 7) for t in range(7)) * 120
    assert abs(st.vi_tot() - want) <= 1e-9 * want
    assert abs(ref.expected_vi(c, z, 7) - st.vi_tot() / (7 * 120)) <= 1e-12


@pytest.mark.parametrize("criterion", ["binder", "vi"])
def test_a_sequential_pass_never_raises_the_total(criterion):
    z, _ = ref.make_trace(6, 150, 9, ref.EPS, 8)
    st = ref.State(z, np.random.default_rng(9).integers(1, 7, 150), 6, 6)
    tot = st.total(criterion)
    for _ in range(4):
        moved = st.one_pass(1, criterion)
        new = st.total(criterion)
        assert new <= tot + (0 if criterion == "binder" else 1e-9 * abs(tot))
        assert (new < tot) or moved == 0 or criterion == "vi"
        tot = new
        chk = ref.State(z, st.labels(), 6, 6)  # the tables kept up to date equal the tables rebuilt
        assert np.array_equal(chk.T, st.T) and np.array_equal(chk.n, st.n)


def _brute_force_no_move_lowers(z, c, Kc, Ka):
    st = ref.State(z, c, Kc, Ka)
    base = st.binder2()
    for i in range(st.N):
        for a in range(Ka):
            if a != st.c[i]:
                lab = st.labels()
                lab[i] = a + 1
                assert ref.State(z, lab, Kc, Ka).binder2() >= base, (i, a)


@pytest.mark.parametrize("case", [c for c in SMALL if c[1] <= 257], ids=ref.case_id)
def test_converged_results_pass_a_brute_force_check(case):
    Kc, N, S, batch, min_batch, _ = case
    z, _ = ref.make_trace(Kc, N, S, ref.EPS, 100 + Kc)
    res = ref.search(z, Kc, "binder", ref.start_of(case, z), batch, min_batch)
    assert res["binder2"] <= res["start_binder2"]
    if res["converged"]:
        _brute_force_no_move_lowers(z, res["z"], Kc, Kc)
    seq = ref.search(z, Kc, "binder", ref.start_of(case, z), 1, 1, max_passes=200)
    assert seq["converged"]  # batch 1 lowers the total with every move: it always ends
    _brute_force_no_move_lowers(z, seq["z"], Kc, Kc)


@pytest.mark.parametrize("case", SMALL, ids=ref.case_id)
def test_never_worse_than_the_start_at_any_batch(case):
    Kc, N, S, _, _, _ = case
    z, _ = ref.make_trace(Kc, N, S, ref.EPS, 100 + Kc)
    start = ref.start_of(case, z)
    for batch in sorted({1, 7, max(1, N // 8), N}):
        if batch == 1 and N > 300:
            continue
        res = ref.search(z, Kc, "binder", start, batch, 1)
        assert res["binder2"] <= res["start_binder2"] and res["total"] == res["binder2"]
        assert res["binder2"] == ref.State(z, res["z"], Kc, Kc).binder2()
        assert res["passes"] == len(res["batch"]) <= 50
    if N <= 65:
        res = ref.search(z, Kc, "vi", start, max(1, N // 8), 1)
        assert res["total"] <= res["start_total"]


def _plan(case, criterion):
    Kc, N, S, batch, _, _ = case
    return bm.partition_search_plan(S, N, Kc, criterion=criterion, batch=batch)


def test_plan_hand_derived():
    # Kc = Ka = 20, the north-star trace: 3 threads a row, 85 rows a workgroup, slot stride 28; a uint32 table is
    # 20 * 28 * 4 = 2240 B -> 21 draws per 48 KiB block, 10 blocks; batch N / 8 = 125 000 rows -> 1471 workgroups
    p = bm.partition_search_plan(200, 10 ** 6, 20)
    assert p == {"label_bytes": 1, "slot_stride": 28, "threads_per_row": 3, "rows_per_workgroup": 85, "draws_per_block": 21,
                 "draw_blocks": 10, "block_bound": 1, "lds_bytes": 21 * 2240, "workgroups": 1471, "batches": 8, "vi": 0,
                 "table_bytes": 200 * 2240}
    # VI: binary64 tables, 4480 B -> 10 draws a block; the counts and two phi tables in global memory
    p = bm.partition_search_plan(200, 10 ** 6, 20, criterion="vi")
    assert (p["draws_per_block"], p["draw_blocks"], p["lds_bytes"], p["vi"], p["table_bytes"]) == (10, 20, 44800, 1, 200 * 560 * 20)
    # Ka = 64: 8 threads a row, 32 rows; 64 * 68 * 4 = 17 408 B -> 2 draws a block
    p = bm.partition_search_plan(9, 4099, 64, batch=512)
    assert (p["threads_per_row"], p["rows_per_workgroup"], p["slot_stride"], p["draws_per_block"], p["workgroups"], p["batches"]) == \
        (8, 32, 68, 2, 16, 9)
    # a small shape: every draw in one block, and the LDS still holds the scores of 256 x 8 slots
    p = bm.partition_search_plan(3, 63, 2, batch=1)
    assert (p["draws_per_block"], p["block_bound"], p["lds_bytes"], p["workgroups"], p["batches"]) == (3, 0, 16384, 1, 63)
    # more slots than labels
    assert bm.partition_search_plan(3, 63, 2, max_clusters=9)["threads_per_row"] == 2
    # D N must stay below 2^32 for the 32-bit sums of a block: 200 draws of 3e7 rows -> 143
    p = bm.partition_search_plan(200, 30_000_000, 2)
    assert (p["draws_per_block"], p["block_bound"]) == (143, 2)
    assert bm.partition_search_plan(200, 30_000_000, 2, criterion="vi")["block_bound"] == 0


def test_the_cases_reach_every_form():
    """what the plan can name: the criterion x what bounds a block of draws (S, the LDS, the 32-bit sums -- the last
    for Binder alone), one thread a row or several"""
    got = set()
    for case in ref.CASES + ref.PLAN_ONLY:
        for crit in ("binder", "vi"):
            p = _plan(case, crit)
            got.add((p["vi"], p["block_bound"], p["threads_per_row"] > 1))
            assert p["draws_per_block"] * (8 if p["vi"] else 4) * case[0] * p["slot_stride"] <= 48 << 10
            assert p["lds_bytes"] <= 48 << 10 and p["rows_per_workgroup"] * p["threads_per_row"] <= 256
    assert {(v, b) for v, b, _ in got} == {(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)}
    assert {m for _, _, m in got} == {False, True}
    # the GPU cases alone reach every form but the 32-bit bound, which needs N D >= 2^32
    gpu = {(_plan(c, k)["vi"], _plan(c, k)["block_bound"]) for c in ref.CASES for k in ("binder", "vi")}
    assert gpu == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {_plan(c, "binder")["threads_per_row"] for c in ref.CASES} == {1, 3, 5, 8}


def _search_rc(z, S, N, Kc, crit=0, start=None, opts=None, out=True):
    L = _capi.lib()
    so = bm._Search("binder", N, bm._SearchOpts(1, 1, 50, 1))
    return L.bmm_device_partition_search(
        C.c_int(0), _capi.vp(z) if z is not None else None, C.c_int(S), C.c_int64(N), C.c_int(Kc), C.c_int(crit),
        _capi.vp(start) if start is not None else None, C.byref(opts) if opts is not None else None,
        C.byref(so.s) if out else None)


def test_refusals_come_before_a_device_is_touched():
    """(this machine has no device: a call that reached one would fail with another code)"""
    L = _capi.lib()
    z = np.asfortranarray(np.random.default_rng(0).integers(1, 4, (5, 40)), dtype=np.int32)
    E_ARG = 1

    def refused(rc, word):
        assert rc == E_ARG, rc
        assert word in L.bmm_last_error().decode(), L.bmm_last_error().decode()

    refused(_search_rc(z, 5, 40, 65), "Kc = 65")
    refused(_search_rc(z, 5, 40, 3, opts=bm._SearchOpts(8, 1, 50, 65)), "max_clusters")
    refused(_search_rc(z, 5, 40, 3, opts=bm._SearchOpts(8, 1, 50, 0)), "max_clusters")
    refused(_search_rc(z, 5, 40, 3, opts=bm._SearchOpts(0, 1, 50, 3)), "batch")
    refused(_search_rc(z, 5, 40, 3, opts=bm._SearchOpts(8, 0, 50, 3)), "batch")
    refused(_search_rc(z, 5, 40, 3, opts=bm._SearchOpts(8, 1, 0, 3)), "max_passes")
    refused(_search_rc(z, 5, 40, 3, opts=bm._SearchOpts(8, 1, 50, 2)), "max_clusters >= Kc")  # no start: a draw has 3 labels
    refused(_search_rc(z, 5, 40, 3, crit=2), "criterion")
    refused(_search_rc(z, 0, 40, 3), "S must be")
    refused(_search_rc(z, 5, 0, 3), "N must be")
    refused(_search_rc(z, 5, 2 ** 31, 3), "2^63")
    refused(_search_rc(None, 5, 40, 3), "null")
    refused(_search_rc(z, 5, 40, 3, out=False), "null output")
    start = np.ones(40, dtype=np.int32)
    start[17] = 4
    refused(_search_rc(z, 5, 40, 3, start=start), "observation 17")
    start[17] = 0
    refused(_search_rc(z, 5, 40, 3, start=start), "observation 17")
    start[17] = 3
    refused(_search_rc(z, 5, 40, 3, start=start, opts=bm._SearchOpts(8, 1, 50, 2)), "observation 17")  # Ka = 2 < 3
    zbad = z.copy(order="F")
    zbad[2, 7] = 4
    refused(_search_rc(zbad, 5, 40, 3), "observation 7")
    # the plan refuses the same
    out = (C.c_int64 * 12)()
    L.bmm_partition_search_plan.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p]
    for args in ((5, 40, 65, 65, 0, 5), (5, 40, 3, 65, 0, 5), (5, 40, 3, 3, 0, 0), (5, 2 ** 31, 3, 3, 0, 5), (5, 40, 3, 3, 7, 5)):
        assert L.bmm_partition_search_plan(*args, out) == E_ARG
    assert L.bmm_partition_search_plan(5, 40, 3, 3, 0, 5, None) == E_ARG
    # ... and the wrappers, before the library is asked
    with pytest.raises(ValueError):
        bm.partition_search(z, "binder", batch=0)
    with pytest.raises(ValueError):
        bm.partition_search(z, "binder", max_clusters=65)
    with pytest.raises(ValueError):
        bm.partition_search(z, "hamming")
    with pytest.raises(ValueError):
        bm.partition_search(z, "binder", start=np.ones(39, dtype=np.int32))
    X = np.zeros((40, 3), dtype=np.int32)
    with pytest.raises(ValueError, match="needs partition"):
        bm.gibbs_collapsed(X, 5, 2, seed=1, partition_search=True)
    with pytest.raises(ValueError, match="unknown option"):
        bm.gibbs_collapsed(X, 5, 2, seed=1, partition="binder", partition_search={"passes": 3})
    with pytest.raises(ValueError, match="at most 64"):
        bm.gibbs_dp(X, 5, seed=1, maxK=65, partition="binder", partition_search=True)


def test_arming_needs_a_partition_summary():
    """bmm_set_partition_search without bmm_set_partition_summary: the run refuses before a device is touched, and
    the refusal disarms"""
    L = _capi.lib()
    X = np.asfortranarray(np.zeros((40, 3), dtype=np.int32))
    so = bm._Search("binder", 40, bm._search_opts(40, 2))
    so.arm()
    z0 = np.ones(40, dtype=np.int32)
    z = np.zeros((4, 40), dtype=np.int32, order="F")
    th = np.zeros((2, 3, 4), order="F")
    al = np.zeros((4, 1), order="F")
    rc = L.bmm_collapsed_run_probs(_capi.vp(X), C.c_int64(40), C.c_int(3), _capi.vp(z0), C.c_int(5), C.c_int(2),
                                   C.c_double(0.0), C.c_double(0.5), C.c_double(0.5), C.c_double(1.0), C.c_double(1.0),
                                   C.c_int(1), C.c_int64(0), C.c_uint64(1), C.c_int(0), _capi.vp(z), _capi.vp(th),
                                   _capi.vp(al), None)
    assert rc == 1 and "needs an armed partition summary" in L.bmm_last_error().decode()
