"""Greedy search for the clustering point estimate (include/bmm_mcmc.h "greedy search"): what can
be checked without a GPU.  The restatement tests/partition_search_ref.py against the definitions it rests on (the
scores against differences of full totals, passes that never raise the total, converged results against a brute
force), and the library's plan and refusals, which touch no device."""
import ctypes as C
import functools
import hashlib
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


# ---- the VI search held to a restatement, decision by decision: the reference side (no device) --------------------
# make_trace(Kc, N, S, EPS, 100 + Kc) of CASES before the decay= keyword: sha256 of z (column-major) + truth
TRACE_DIGESTS = [
    "64ed86b909d6d0502b64b28db0ea1272ffb358e20e9b1d88b63ccb07fa900cf5",
    "0626b0fd2a02d8b8669a58368385f587a54a13b0156682565ad15664004ab752",
    "115e2bf210c04ee3a742984ee23430ffc4b35e55b8d21445a3cc1a8438f700b2",
    "076d66b2637cd2d191477b303011c77c69665853bfc90f0c104a5a79c83132b4",
    "bdf1fbed6b8553869eb7b72ba72e642b9a13acca376125a58d1807cb892bc5a7",
    "5a0029f025f516c1d5032b051be0ee111adc4050e12cf6cc83e63a6c24514f9f",
    "bda6c303cf50549e3f7773357092684e200c040034fdca4bd31f714f4d894663",
    "5a0387d469555b0ecfc3c017de5716b39c288ac2eaaa0bd312e5a212f19f026b",
    "ed870f8b0201c53d0f2f74b3cb2ad42d401a4c0fb6410d811e119ff441dec1a6",
    "3028173d2a63b7edc52dbd0ca0e8a6aa43c216c0a46751e7732ac56c552aebf6",
    "f4ba450299573c7e3df50cc6a7821a3776047dbc042d97cea83872db6801e23c",
]


def test_the_default_decay_leaves_every_trace_byte_equal():
    assert len(TRACE_DIGESTS) == len(ref.CASES)
    for case, want in zip(ref.CASES, TRACE_DIGESTS):
        z, truth = ref.make_trace(case[0], case[1], case[2], ref.EPS, 100 + case[0])
        assert z.dtype == np.int32 and truth.dtype == np.int32 and z.flags.f_contiguous
        assert hashlib.sha256(z.tobytes(order="F") + truth.tobytes()).hexdigest() == want, ref.case_id(case)
    a = ref.make_trace(5, 100, 3, ref.EPS, 7)
    b = ref.make_trace(5, 100, 3, ref.EPS, 7, decay=0.7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    flat = ref.make_trace(5, 4000, 1, 0.0, 7, decay=1.0)[1]
    assert np.bincount(flat)[1:].min() > 700  # decay = 1: a flat truth


@functools.lru_cache(maxsize=None)
def _vi_ref(case):
    return ref.vi_reference(case)


@functools.lru_cache(maxsize=None)
def _vi_first_pass(case):
    return ref.vi_reference(case, batch=case[1], min_batch=case[1], max_passes=1)


def test_vi_case_list_is_well_formed():
    assert len(set(ref.VI_CASES)) == len(ref.VI_CASES) <= 16 and max(c[1] for c in ref.VI_CASES) <= 4100
    assert len({ref.vi_case_id(c) for c in ref.VI_CASES}) == len(ref.VI_CASES)
    assert set(ref.VI_MAX_PASSES) <= set(ref.VI_CASES) and set(ref.VI_FIRST_PASS) <= set(ref.VI_CASES)
    for case in ref.VI_CASES:
        Kc, N, S, batch, min_batch, start, Ka, decay, seed = case
        z = ref.vi_trace(case)
        st = ref.vi_start(case, z)
        assert z.shape == (S, N) and z.min() >= 1 and z.max() <= Kc
        assert st.shape == (N,) and st.dtype == np.int32 and st.min() >= 1 and st.max() <= Ka
        if start == "rand":
            assert np.array_equal(st, np.random.default_rng(seed + 50).integers(1, Ka + 1, N))


@pytest.mark.parametrize("case", [c for c in ref.VI_CASES if c[1] <= 600], ids=ref.vi_case_id)
def test_the_margin_restatement_follows_the_search(case):
    """the vectorised np.longdouble search against the row-by-row binary64 one: the same course, the totals within
    the project's bound for a VI total"""
    Kc, N, S, batch, min_batch, _, Ka, _, _ = case
    z, start, got = _vi_ref(case)
    want = ref.search(z, Kc, "vi", start, batch, min_batch, ref.VI_MAX_PASSES.get(case, 50), Ka)
    for k in ("passes", "batch", "moved", "converged", "n_clusters", "binder2", "start_binder2"):
        assert got[k] == want[k], k
    assert np.array_equal(got["z"], want["z"]) and got["z"].dtype == np.int32
    bound = pr.vi_bound(max(Kc, Ka), N) * S * N
    assert len(got["pass_total"]) == len(want["pass_total"])
    for a, b in zip(got["pass_total"] + [got["total"], got["start_total"]], want["pass_total"] + [want["total"], want["start_total"]]):
        assert abs(a - b) <= bound
    assert got["loss"] == got["total"] / (S * N) and got["start_loss"] == got["start_total"] / (S * N)


def test_structural_ties_are_left_out_and_nothing_else():
    """Ka = 6 slots, three of them empty, and row 0, which no draw puts with any other row, alone in slot 3: it stays,
    the three empty slots score 0 from the same cells as its own and are no margin.  An exact tie between two slots
    whose cells differ in their order is none of them"""
    z = np.asfortranarray(np.array([[2, 1, 1, 1, 1, 1, 1]] * 3, dtype=np.int32))
    c = np.array([3, 1, 1, 2, 2, 1, 2], dtype=np.int32)
    res = ref.search_vi_margins(z, 2, c, 7, 7, max_passes=1, Ka=6, keep_scores=True)
    G = res["first_scores"]
    assert G.dtype == np.longdouble and G.shape == (7, 6)
    assert np.all(G[:, 3:] == 0) and G[0, 2] == 0
    assert res["first_choice"][0] == 3 and G[0, :2].min() > 0
    assert res["structural_ties"] == 3 and res["score_margin"] > 0 and np.isfinite(res["score_margin"])
    st = ref.State(z, c, 2, 6)
    for i in range(7):
        g = st.scores(i, "vi")
        assert np.allclose(np.asarray(G[i], dtype=float), g, rtol=0, atol=1e-12)
        assert res["first_choice"][i] == ref.State.choose(g, st.c[i]) + 1
    # rows 0, 1 in slot 0, rows 2, 3 in slot 1, row 4 alone: the draws put 2 then 1 rows of slot 0 beside row 4 and 1
    # then 2 of slot 1 -- the same cells in another order, equal to the last bit in a sum of two yet no structural
    # tie, so the margin is 0 and such a case is refused
    z = np.asfortranarray(np.array([[1, 1, 1, 2, 1], [1, 2, 1, 1, 1]], dtype=np.int32))
    res = ref.search_vi_margins(z, 2, np.array([1, 1, 2, 2, 3], dtype=np.int32), 5, 5, max_passes=1, Ka=3, keep_scores=True)
    assert res["first_scores"][4, 0] == res["first_scores"][4, 1] < 0 and res["first_choice"][4] == 1
    assert res["score_margin"] == 0
    assert not ref.margins_hold(res, 2, 3, 5, 2)


@pytest.mark.parametrize("case", ref.VI_CASES, ids=ref.vi_case_id)
def test_vi_cases_meet_the_margin_condition(case):
    """No decision of the reference's course is within 2^10 x 2 error bounds of another: E_g for two scores,
    vi_bound S N for two totals -- so the device must follow it with ==.  A case that fails is replaced."""
    Kc, N, S, _, _, _, Ka, _, _ = case
    runs = [("search", _vi_ref(case)[2])]
    if case in ref.VI_FIRST_PASS:
        runs.append(("first pass", _vi_first_pass(case)[2]))
    for name, res in runs:
        print("%s %s: score_margin %.3g (E_g %.3g), total_margin %.3g (bound %.3g), %d structural ties; passes %d, batches %s, moved %s, %s"
              % (ref.vi_case_id(case), name, res["score_margin"], ref.score_error_bound(N, S), res["total_margin"],
                 pr.vi_bound(max(Kc, Ka), N) * S * N, res["structural_ties"], res["passes"], res["batch"], res["moved"], res["stopped"]))
        assert res["score_margin"] >= 2 ** 10 * 2 * ref.score_error_bound(N, S)
        assert res["total_margin"] >= 2 ** 10 * 2 * pr.vi_bound(max(Kc, Ka), N) * S * N
        assert ref.margins_hold(res, Kc, Ka, N, S)
    if case in ref.VI_FIRST_PASS:
        fp = _vi_first_pass(case)[2]
        assert fp["moved"][0] > 0 and fp["pass_total"][0] < fp["start_total"]  # the first pass improves: z is its choices
        assert np.array_equal(fp["z"], ref.vi_reference(case, batch=case[1], min_batch=case[1], max_passes=1, keep_scores=True)[2]["first_choice"])


def test_vi_cases_reach_every_path_of_the_vi_kernels():
    """from the library's plan and the reference's log: what k_ps_phi, k_ps_score<VI> and the host's keep-best can do
    differently, each reached by a case"""
    tpr, bound, last, stopped = set(), set(), [], set()
    seen = dict.fromkeys(("one_draw_blocks", "out_of_high", "into_high", "opened", "fewer_slots", "batches", "ragged",
                          "halved", "ties"), False)
    for case in ref.VI_CASES:
        Kc, N, S, batch, min_batch, start, Ka, _, _ = case
        res = _vi_ref(case)[2]
        p = bm.partition_search_plan(S, N, Kc, max_clusters=Ka, criterion="vi", batch=batch)
        assert p["vi"] == 1 and p["draws_per_block"] * 8 * Kc * p["slot_stride"] <= 48 << 10
        D = p["draws_per_block"]
        tpr.add(p["threads_per_row"])
        bound.add(p["block_bound"])
        last.append((D, S - (p["draw_blocks"] - 1) * D, res["score_margin"]))
        stopped.add(res["stopped"])
        seen["one_draw_blocks"] |= D == 1 and S > 1
        seen["out_of_high"] |= res["from_high"] > 0 and p["threads_per_row"] > 1
        seen["into_high"] |= res["into_high"] > 0 and p["threads_per_row"] > 1
        seen["opened"] |= Ka > Kc and res["opened_empty"] > 0
        seen["fewer_slots"] |= Ka < Kc and sum(res["moved"]) > 0
        seen["batches"] |= p["batches"] > 1 and res["moved"][0] > 0  # the phi tables refreshed inside a pass
        seen["ragged"] |= p["workgroups"] > 1 and min(batch, N) % p["rows_per_workgroup"] != 0
        seen["halved"] |= any(b < a for a, b in zip(res["batch"], res["batch"][1:]))  # no improvement, restore, halve
        seen["ties"] |= res["structural_ties"] > 0
    assert tpr == {1, 2, 3, 5, 8}
    assert bound == {0, 1}
    # the draw loop is unrolled by two: a last block with an odd number of draws, in one that is shorter than the
    # others (S % D != 0) and in a single block; the 48 KiB budget leaves one draw a block at Kc = Ka = 64
    # ... each in a case that decides some row by less than 2 phi(1), the least that one cell of one draw adds to a
    # score: where every gap is far above that, a draw left out changes nothing
    small = 2 * ref.phi(1)
    assert any(D >= 2 and n < D and n % 2 == 1 and g < small for D, n, g in last)
    assert any(D >= 2 and n < D and n % 2 == 0 for D, n, g in last)
    assert any(D >= 2 and n == D and n % 2 == 1 and g < small for D, n, g in last)
    assert stopped == {"converged", "min_batch", "max_passes"}
    assert all(seen.values()), seen
    assert bm.partition_search_plan(11, 2053, 64, criterion="vi")["draws_per_block"] == 1


@pytest.mark.parametrize("case", [c for c in ref.VI_CASES if c[1] <= 300], ids=ref.vi_case_id)
def test_converged_vi_cases_pass_the_brute_force(case):
    """what the device test asks of a converged result, asked of the reference's own"""
    Kc, N, S, _, _, _, Ka, _, _ = case
    z, _, res = _vi_ref(case)
    if case not in ref.VI_MAX_PASSES:
        assert res["converged"]
    if res["converged"]:
        st = ref.State(z, res["z"], Kc, Ka)
        for i in range(N):
            for a in range(Ka):
                assert st.move_delta_vi(i, a) / (S * N) >= -pr.vi_bound(max(Kc, Ka), N), (i, a)
