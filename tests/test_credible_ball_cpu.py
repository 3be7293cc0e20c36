"""Credible ball and row-to-cluster similarity (include/bmm_mcmc.h "credible ball"): the library's
plan and every refusal, which touch no device."""
import ctypes as C

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi
import credible_ball_ref as cbr

NEW = ["bmm_device_credible_ball", "bmm_credible_ball_plan", "bmm_set_credible_ball"]
E_ARG = 1


def _ball(opt, fn, *args, **kw):
    """fn(*args, **kw) with credible_ball=opt among the run's options"""
    with bm.run_options(credible_ball=opt):
        return fn(*args, **kw)


def test_entry_points_are_exported():
    L = _capi.lib()
    for s in NEW:
        assert s in _capi.SYMBOLS
        getattr(L, s)
    assert "credible_ball" in bm.__all__ and "credible_ball_plan" in bm.__all__ and "run_options" in bm.__all__


def test_plan_hand_derived():
    # Kc = Ka = 20, the north-star trace, all rows: 3 threads a row, 85 rows a workgroup, slot stride 28; a table is
    # 20 * 28 * 4 = 2240 B -> 21 draws per 48 KiB block, 10 blocks; ceil(1e6 / 85) = 11765 workgroups -- under either
    # criterion, the tables being the counts
    for crit, vi in (("binder", 0), ("vi", 1)):
        p = bm.credible_ball_plan(200, 10 ** 6, 20, criterion=crit)
        assert p == {"label_bytes": 1, "slot_stride": 28, "threads_per_row": 3, "rows_per_workgroup": 85, "draws_per_block": 21,
                     "draw_blocks": 10, "block_bound": 1, "lds_bytes": 21 * 2240, "workgroups": 11765, "gathered": 0, "vi": vi,
                     "table_bytes": 200 * 2240}
    # Ka = 64: 8 threads a row, 32 rows; 64 * 68 * 4 = 17 408 B -> 2 draws a block, 5 blocks of the 9 draws
    p = bm.credible_ball_plan(9, 1000, 64)
    assert (p["threads_per_row"], p["rows_per_workgroup"], p["slot_stride"], p["draws_per_block"], p["draw_blocks"],
            p["block_bound"], p["lds_bytes"], p["workgroups"]) == (8, 32, 68, 2, 5, 1, 2 * 17408, 32)
    # a small shape: every draw in one block, the LDS holds the tables and nothing else
    p = bm.credible_ball_plan(3, 63, 2)
    assert (p["draws_per_block"], p["block_bound"], p["lds_bytes"], p["workgroups"]) == (3, 0, 3 * 2 * 12 * 4, 1)
    # a subset is gathered; more slots than labels
    p = bm.credible_ball_plan(3, 63, 2, max_clusters=9, rows=5)
    assert (p["threads_per_row"], p["gathered"], p["workgroups"]) == (2, 1, 1)
    # D N must stay below 2^32 for the 32-bit sums of a block, under VI too
    for crit in ("binder", "vi"):
        p = bm.credible_ball_plan(200, 30_000_000, 2, criterion=crit)
        assert (p["draws_per_block"], p["block_bound"]) == (143, 2)


def test_the_gpu_cases_reach_every_form():
    """what the plan can name and a small shape can reach: one block of draws and several, one thread a row and
    several, all rows and a gathered subset, Binder and VI (the 32-bit bound needs N D >= 2^32: plan only, above)"""
    got = set()
    for case in cbr.CASES:
        Kc, Ka, N, S, m = case
        for crit in ("binder", "vi"):
            for rows in (None, m):
                p = bm.credible_ball_plan(S, N, Kc, Ka, crit, rows=rows)
                got.add((p["draw_blocks"] > 1, p["threads_per_row"] > 1, p["gathered"], p["vi"]))
                assert p["lds_bytes"] == p["draws_per_block"] * 4 * Kc * p["slot_stride"] <= 48 << 10
                assert p["rows_per_workgroup"] * p["threads_per_row"] <= 256
                assert p["workgroups"] == -(-(N if rows is None else rows) // p["rows_per_workgroup"])
    for dim in range(4):  # each of the four choices is taken both ways
        assert {bool(g[dim]) for g in got} == {False, True}
    # ... the gathered subset and both criteria at every shape
    assert {g[:2] for g in got} == {g[:2] for g in got if g[2] and g[3]} == {g[:2] for g in got if not g[2] and not g[3]}
    # the shapes do what the table of the test file says of them
    assert bm.credible_ball_plan(70, 4099, 20, 24)["threads_per_row"] == 3
    p = bm.credible_ball_plan(9, 1000, 64, 64)
    assert p["block_bound"] == 1 and p["draw_blocks"] > 1
    assert 257 % 16 and 257 % bm.credible_ball_plan(17, 257, 3, 5)["rows_per_workgroup"]


def _ball_rc(z, S, N, Kc, centre, Ka, crit=1, level=0.95, rows=None, out=True, sim=False):
    L = _capi.lib()
    b = bm._Ball("vi", 0.95, max(S, 1), max(min(N, 64), 1), max(min(Ka, 64), 1), sim, rows)
    return L.bmm_device_credible_ball(
        C.c_int(0), _capi.vp(z) if z is not None else None, C.c_int(S), C.c_int64(N), C.c_int(Kc), C.c_int(crit),
        _capi.vp(centre) if centre is not None else None, C.c_int(Ka), C.c_double(level), C.byref(b.s) if out else None)


def test_refusals_come_before_a_device_is_touched():
    """(this machine has no device: a call that reached one would fail with another code)"""
    L = _capi.lib()
    z = np.asfortranarray(np.random.default_rng(0).integers(1, 4, (5, 40)), dtype=np.int32)
    c = np.ascontiguousarray(z[0], dtype=np.int32)

    def refused(rc, word):
        assert rc == E_ARG, rc
        assert word in L.bmm_last_error().decode(), L.bmm_last_error().decode()

    refused(_ball_rc(z, 5, 40, 65, c, 3), "Kc = 65")
    refused(_ball_rc(z, 5, 40, 0, c, 3), "Kc")
    refused(_ball_rc(z, 5, 40, 3, c, 65), "Ka must be")
    refused(_ball_rc(z, 5, 40, 3, c, 0), "Ka must be")
    for level in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        refused(_ball_rc(z, 5, 40, 3, c, 3, level=level), "level")
    refused(_ball_rc(z, 5, 40, 3, c, 3, crit=2), "criterion")
    refused(_ball_rc(z, 0, 40, 3, c, 3), "S must be")
    refused(_ball_rc(z, 5, 0, 3, c, 3), "N must be")
    refused(_ball_rc(z, 5, 2 ** 31, 3, c, 3), "2^63")
    refused(_ball_rc(None, 5, 40, 3, c, 3), "null")
    refused(_ball_rc(z, 5, 40, 3, None, 3), "null")
    refused(_ball_rc(z, 5, 40, 3, c, 3, out=False), "null")
    bad = c.copy()
    bad[17] = 4
    refused(_ball_rc(z, 5, 40, 3, bad, 3), "observation 17")
    bad[17] = 0
    refused(_ball_rc(z, 5, 40, 3, bad, 5), "observation 17")
    refused(_ball_rc(z, 5, 40, 3, c, 2), "observation")  # Ka = 2 below a label of the centre
    for idx in ([0, 40], [-1], [3, 7, 2 ** 40]):
        refused(_ball_rc(z, 5, 40, 3, c, 3, rows=np.array(idx, dtype=np.int64)), "member_idx")
    zbad = z.copy(order="F")
    zbad[2, 7] = 4
    refused(_ball_rc(zbad, 5, 40, 3, c, 3), "observation 7")
    # the plan refuses the same
    out = (C.c_int64 * 12)()
    L.bmm_credible_ball_plan.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p]
    for args in ((5, 40, 65, 3, 0, 40), (5, 40, 3, 65, 0, 40), (5, 40, 3, 0, 0, 40), (5, 2 ** 31, 3, 3, 0, 5), (5, 40, 3, 3, 7, 5),
                 (5, 40, 3, 3, 0, 0), (0, 40, 3, 3, 0, 5)):
        assert L.bmm_credible_ball_plan(*args, out) == E_ARG
    assert L.bmm_credible_ball_plan(5, 40, 3, 3, 0, 5, None) == E_ARG


def test_the_wrappers_refuse_before_the_library_is_asked():
    z = np.asfortranarray(np.random.default_rng(0).integers(1, 4, (5, 40)), dtype=np.int32)
    c = z[0]
    for kw in (dict(level=0.0), dict(level=1.5), dict(level=float("nan")), dict(criterion="hamming"), dict(max_clusters=65),
               dict(max_clusters=0), dict(membership_of=[40]), dict(membership_of=[-1]), dict(membership_of=[])):
        with pytest.raises(ValueError):
            bm.credible_ball(z, c, **kw)
    with pytest.raises(ValueError):
        bm.credible_ball(z, c[:-1])
    with pytest.raises(ValueError):
        bm.credible_ball(z[0], c)
    X = np.zeros((40, 3), dtype=np.int32)
    for fn, args in ((bm.gibbs_collapsed, (X, 5, 2)), (bm.gibbs_dp, (X, 5)), (bm.gibbs_stickbreaking, (X, 5, 2)),
                     (bm.gibbs_full, (X, 5, 2)), (bm.gibbs_allocation, (X, 5, 3))):
        with pytest.raises(ValueError, match="needs partition"):
            _ball(True, fn, *args, seed=1)
        with pytest.raises(ValueError, match="unknown option"):
            _ball({"levle": 0.9}, fn, *args, seed=1, partition="vi")
        with pytest.raises(ValueError, match="level"):
            _ball(0.0, fn, *args, seed=1, partition="vi")
        with pytest.raises(ValueError, match="membership_of"):
            _ball({"membership_of": [40]}, fn, *args, seed=1, partition="vi")
    with pytest.raises(ValueError, match="keep_trace=False"):
        _ball(True, bm.gibbs_collapsed, X, 5, 2, seed=1, partition="vi", summary=True, keep_trace=False)
    with pytest.raises(ValueError, match="at most 64"):
        _ball(True, bm.gibbs_dp, X, 5, seed=1, maxK=65, partition="binder")
    with pytest.raises(ValueError, match="at most 64"):
        _ball(True, bm.gibbs_collapsed, X, 5, 65, seed=1, chains=2, partition="binder")


def _run_rc(L):
    X = np.asfortranarray(np.zeros((40, 3), dtype=np.int32))
    z0 = np.ones(40, dtype=np.int32)
    z = np.zeros((4, 40), dtype=np.int32, order="F")
    th = np.zeros((2, 3, 4), order="F")
    al = np.zeros((4, 1), order="F")
    return L.bmm_collapsed_run_probs(_capi.vp(X), C.c_int64(40), C.c_int(3), _capi.vp(z0), C.c_int(5), C.c_int(2),
                                     C.c_double(0.0), C.c_double(0.5), C.c_double(0.5), C.c_double(1.0), C.c_double(1.0),
                                     C.c_int(1), C.c_int64(0), C.c_uint64(1), C.c_int(0), _capi.vp(z), _capi.vp(th),
                                     _capi.vp(al), None)


def test_arming_needs_a_partition_summary():
    """bmm_set_credible_ball without bmm_set_partition_summary: the run refuses before a device is touched"""
    L = _capi.lib()
    bm._Ball("vi", 0.95, 4, 40, 2).arm()
    assert _run_rc(L) == E_ARG and "needs an armed partition summary" in L.bmm_last_error().decode()


def test_an_armed_run_refuses_a_bad_level_and_a_bad_row_before_a_device_is_touched():
    L = _capi.lib()
    for ball, word in ((bm._Ball("vi", 1.5, 4, 40, 2), "level"),
                       (bm._Ball("vi", 0.9, 4, 40, 2, rows=np.array([3, 40], dtype=np.int64)), "member_idx[1]")):
        pt = bm._Partition("vi", 1, None, 40, 4)
        pt.arm()
        ball.arm()
        assert _run_rc(L) == E_ARG and word in L.bmm_last_error().decode(), L.bmm_last_error().decode()
    # ... and the refusal disarmed both: a summary armed alone is not refused for the ball's sake
    bm._Ball("vi", 1.5, 4, 40, 2).arm()
    assert _run_rc(L) == E_ARG and "partition summary" in L.bmm_last_error().decode()
    pt = bm._Partition("vi", 1, None, 40, 4)
    pt.s.stride = 0
    pt.arm()
    assert _run_rc(L) == E_ARG and "stride" in L.bmm_last_error().decode()  # (the summary's own refusal: no ball is armed)


def test_run_options_hold_inside_the_block_only():
    """the wrappers' signatures stay as they are: the option reaches them through the block, and nothing outside it"""
    X = np.zeros((40, 3), dtype=np.int32)
    assert bm._run_option("credible_ball") is None
    with pytest.raises(ValueError, match="unknown option credible_bal "):
        bm.run_options(credible_bal=True)
    with bm.run_options(credible_ball=0.9):
        assert bm._run_option("credible_ball") == 0.9
        with bm.run_options(credible_ball={"level": 0.5}):
            assert bm._run_option("credible_ball") == {"level": 0.5}
        assert bm._run_option("credible_ball") == 0.9
        with bm.run_options():
            assert bm._run_option("credible_ball") == 0.9
    assert bm._run_option("credible_ball") is None
    with pytest.raises(ValueError, match="needs partition"):  # a refusal inside the block leaves nothing behind
        with bm.run_options(credible_ball=True):
            bm.gibbs_collapsed(X, 5, 2, seed=1)
    assert bm._run_option("credible_ball") is None
    import threading
    seen = []
    with bm.run_options(credible_ball=True):
        t = threading.Thread(target=lambda: seen.append(bm._run_option("credible_ball")))
        t.start()
        t.join()
    assert seen == [None]  # per thread, as the library's armed state
