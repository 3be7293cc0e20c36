"""Clustering point estimate and posterior similarity (include/bmm_mcmc.h): what can be checked
through the library without a GPU -- the entry points are exported, the plan against hand-derived values and its reach
over the GPU cases, and every refusal that comes before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi
import partition_ref as ref

NEW = ["bmm_device_partition_distances", "bmm_device_psm", "bmm_device_partition_plan", "bmm_set_partition_summary"]


def test_partition_entry_points_are_exported():
    L = _capi.lib()
    for s in NEW:
        assert s in _capi.SYMBOLS
        getattr(L, s)
    assert bm.PARTITION_MAX_K == 1024
    for name in ("partition_distances", "posterior_similarity", "partition_plan"):
        assert name in bm.__all__


def test_plan_hand_derived():
    # K = 20, the north star: a table is 20^2 * 4 = 1600 B > 1 KiB -> one copy; min(8, 48 KiB / 1600) = 8 draws per
    # workgroup, 25 blocks of draws, 200 x 25 workgroups, triangular
    p = bm.partition_plan(200, 10 ** 6, 20)
    assert p == {"label_bytes": 1, "lds": 1, "draws_per_workgroup": 8, "replicas": 1, "draw_blocks": 25,
                 "workgroups": 5000, "threads": 256, "lds_bytes": 8 * 1600, "triangular": 1, "vi": 0,
                 "generic_bytes": 0, "pitch": 10 ** 6}
    # K = 3: 36 B a table -> four copies (one per wave); T = min(8, S) = 5; N = 100 rounds up to 112 labels a row
    p = bm.partition_plan(5, 100, 3)
    assert (p["replicas"], p["draws_per_workgroup"], p["draw_blocks"], p["workgroups"], p["lds_bytes"], p["pitch"]) == \
        (4, 5, 1, 5, 5 * 4 * 36, 112)
    # K = 16 is the last with copies (1024 B), K = 17 the first without
    assert bm.partition_plan(9, 50, 16)["replicas"] == 4 and bm.partition_plan(9, 50, 17)["replicas"] == 1
    # K = 64: 16 KiB a table -> 3 draws per workgroup; 20 of 200 rows as candidates (stride 10): not triangular; VI
    p = bm.partition_plan(200, 10 ** 6, 64, 20, "vi")
    assert (p["lds"], p["draws_per_workgroup"], p["draw_blocks"], p["workgroups"], p["lds_bytes"], p["triangular"], p["vi"]) == \
        (1, 3, 67, 20 * 67, 3 * 16384, 0, 1)
    # K = 65: the generic form, bytes still; one table per workgroup in global memory, a workgroup per pair up to 1024
    p = bm.partition_plan(17, 1000, 65)
    assert (p["label_bytes"], p["lds"], p["workgroups"], p["lds_bytes"], p["generic_bytes"]) == (1, 0, 289, 0, 289 * 65 * 65 * 4)
    p = bm.partition_plan(200, 1000, 65)
    assert p["workgroups"] == 1024
    # K = 257: int32 labels; K = 1024: 4 MiB a table, 256 MiB of them -> 64 workgroups
    assert bm.partition_plan(3, 10, 256)["label_bytes"] == 1 and bm.partition_plan(3, 10, 257)["label_bytes"] == 4
    p = bm.partition_plan(200, 1000, 1024)
    assert (p["workgroups"], p["generic_bytes"]) == (64, 256 << 20)
    # a single row: nothing to pair, still a plan
    assert bm.partition_plan(1, 10, 2)["triangular"] == 1


def _form(p):
    return (p["label_bytes"], p["lds"], p["replicas"], p["triangular"], p["vi"])


def test_the_cases_reach_every_form():
    """every form the plan can name -- label width x LDS/generic x copies (what exists of them: copies only in LDS,
    int32 only in the generic form) x triangular x VI -- is run by one of the GPU cases"""
    want = {(el, lds, R, tri, vi) for (el, lds, R) in ((1, 1, 4), (1, 1, 1), (1, 0, 1), (4, 0, 1))
            for tri in (0, 1) for vi in (0, 1)}
    got = set()
    for Kc, N, S, stride, crit, _ in ref.CASES:
        got.add(_form(bm.partition_plan(S, N, Kc, -(-S // stride), crit)))
    assert got == want
    # and every value the contract lists appears in a case
    assert {c[0] for c in ref.CASES} == {1, 2, 3, 4, 5, 20, 21, 32, 33, 64, 65, 100, 300}
    assert {c[1] for c in ref.CASES} == {1, 63, 64, 65, 10 ** 4 + 7, 10 ** 6}
    assert {c[2] for c in ref.CASES} == {1, 2, 3, 17, 200}
    assert all(S <= 17 for _, N, S, _, _, _ in ref.CASES if N == 10 ** 6)
    assert any(c[3] == 3 for c in ref.CASES) and any(c[3] == c[2] and c[2] > 1 for c in ref.CASES)
    # draws per workgroup that do not divide S, and blocks cut by the diagonal, occur
    assert any(S % bm.partition_plan(S, N, Kc, -(-S // st), cr)["draws_per_workgroup"] for Kc, N, S, st, cr, _ in ref.CASES)


def _dist(z, S, N, Kc, crit=0, stride=1):
    L = _capi.lib()
    loss = np.zeros(S)
    best = C.c_int(-5)
    rc = L.bmm_device_partition_distances(C.c_int(0), _capi.vp(z), C.c_int(S), C.c_int64(N), C.c_int(Kc), C.c_int(crit),
                                          C.c_int(stride), _capi.vp(loss), None, C.byref(best), None)
    return rc, L.bmm_last_error()


def test_stand_alone_calls_refuse_before_touching_a_device():
    L = _capi.lib()
    z = np.ones((4, 6), dtype=np.int32, order="F")
    assert _dist(z, 0, 6, 2) == (1, b"partition: S must be >= 1")
    rc, msg = _dist(z, 4, 6, 2, stride=0)
    assert rc == 1 and b"stride" in msg
    for Kc in (0, 1025):
        rc, msg = _dist(z, 4, 6, Kc)
        assert rc == 1 and b"1 .. 1024" in msg
    rc, msg = _dist(z, 65536, 6, 2)   # the row count is a grid dimension of the launches
    assert rc == 1 and b"65535" in msg
    rc, msg = _dist(z, 4, 6, 2, crit=2)
    assert rc == 1 and b"criterion" in msg
    # S * N^2 >= 2^63: checked from the sizes alone, the matrix is never read
    rc, msg = _dist(z, 4, 2 ** 31, 2)
    assert rc == 1 and b"2^63" in msg
    z[2, 3] = 3
    rc, msg = _dist(z, 4, 6, 2)
    assert rc == 1 and b"label 3 at row 2, observation 3" in msg
    z[2, 3] = 0
    rc, msg = _dist(z, 4, 6, 2)
    assert rc == 1 and b"label 0 at row 2, observation 3" in msg
    z[1, 1] = -2147483648  # NA, the unwritten row of a run without burn-in; the first offender is named
    rc, msg = _dist(z, 4, 6, 2)
    assert rc == 1 and b"row 1, observation 1" in msg
    out = (C.c_int64 * 12)()
    assert L.bmm_device_partition_plan(C.c_int(10), C.c_int64(5), C.c_int(2), C.c_int(6), C.c_int(0), out) == 1  # no stride gives 6 of 10
    assert L.bmm_device_partition_plan(C.c_int(10), C.c_int64(5), C.c_int(2), C.c_int(5), C.c_int(0), out) == 0
    # similarity
    z = np.ones((4, 6), dtype=np.int32, order="F")
    cnt = np.zeros((2, 2), dtype=np.uint32)
    idx = np.array([0, 6], dtype=np.int64)
    assert L.bmm_device_psm(C.c_int(0), _capi.vp(z), C.c_int(4), C.c_int64(6), _capi.vp(idx), C.c_int64(2), _capi.vp(cnt)) == 1
    assert b"idx[1] = 6" in L.bmm_last_error()
    z[3, 5] = 0
    idx[1] = 5
    assert L.bmm_device_psm(C.c_int(0), _capi.vp(z), C.c_int(4), C.c_int64(6), _capi.vp(idx), C.c_int64(2), _capi.vp(cnt)) == 1
    assert b"row 3, observation 5" in L.bmm_last_error()


def test_python_front_end_refuses_before_touching_a_device():
    X = np.zeros((10, 3), dtype=np.int32)
    with pytest.raises(ValueError, match="criterion"):
        bm.gibbs_collapsed(X, 10, 2, partition="dahl")
    with pytest.raises(ValueError, match="stride"):
        bm.gibbs_dp(X, 10, partition="vi", partition_stride=0)
    with pytest.raises(ValueError, match="similarity"):
        bm.gibbs_full(X, 10, 2, partition="binder", similarity_of=[10])
    with pytest.raises(ValueError, match="partition="):
        bm.gibbs_stickbreaking(X, 10, 2, similarity_of=[1])
    with pytest.raises(ValueError, match="criterion"):
        bm.gibbs_collapsed(X, 10, 2, partition="dahl", chains=2)
    with pytest.raises(ValueError, match="stride"):
        bm.gibbs_dp(X, 10, partition="vi", partition_stride=0, chains=2)
    with pytest.raises(ValueError, match="similarity"):                  # several chains: refused before they run
        bm.gibbs_full(X, 10, 2, partition="binder", similarity_of=[10], chains=2)
    with pytest.raises(ValueError, match="partition="):
        bm.gibbs_collapsed(X, 10, 2, similarity_of=[1], chains=2)
    with pytest.raises(ValueError, match="criterion"):
        bm.partition_distances(np.ones((2, 3), dtype=np.int32), "dahl")
    with pytest.raises(ValueError, match="S x N"):
        bm.partition_distances(np.ones(3, dtype=np.int32))
    with pytest.raises(bm.BmmError, match="label 0 at row 1, observation 2"):
        bm.partition_distances(np.array([[1, 1, 1], [1, 1, 0]], dtype=np.int32))


class _Out(C.Structure):
    _fields_ = [("criterion", C.c_int), ("stride", C.c_int), ("loss", C.c_void_p), ("binder2", C.c_void_p),
                ("best", C.c_void_p), ("z_best", C.c_void_p), ("n_used", C.c_void_p), ("dist", C.c_void_p),
                ("psm_idx", C.c_void_p), ("psm_M", C.c_int64), ("psm_cnt", C.c_void_p)]


def test_the_setter_arms_one_run_and_is_disarmed_whatever_that_run_returns():
    """Runs without a device here fail when they reach it; on a machine with one they succeed.  Either way the
    summary belongs to exactly the one run after the setter."""
    L = _capi.lib()
    N, P, K, S = 10, 3, 2, 5
    X = np.zeros((N, P), dtype=np.int32, order="F")
    z0 = np.ones(N, dtype=np.int32)
    z = np.zeros((S, N), dtype=np.int32, order="F")
    th = np.zeros((K, P, S))
    al = np.zeros(S)
    loss = np.zeros(S)
    best, n_used = C.c_int(-7), C.c_int(-7)

    def run():
        rc = L.bmm_collapsed_run(_capi.vp(X), C.c_int64(N), C.c_int(P), _capi.vp(z0), C.c_int(S + 2), C.c_int(K),
                                 C.c_double(1.0), C.c_double(0.5), C.c_double(0.5), C.c_double(1), C.c_double(1),
                                 C.c_int(2), C.c_int64(0), C.c_uint64(1), C.c_int(0), _capi.vp(z), _capi.vp(th), _capi.vp(al))
        return rc, L.bmm_last_error()

    o = _Out(0, 0, loss.ctypes.data, None, C.addressof(best), None, C.addressof(n_used), None, None, 0, None)
    # refused for its stride before any device is touched; the next run no longer sees it
    assert L.bmm_set_partition_summary(C.byref(o)) == 0
    rc, msg = run()
    assert rc == 1 and b"stride" in msg
    rc, msg = run()
    assert rc != 1 and (rc == 0 or b"partition" not in msg)
    assert n_used.value == -7
    # null outputs are refused the same way
    o.stride = 1
    o.loss = None
    assert L.bmm_set_partition_summary(C.byref(o)) == 0
    rc, msg = run()
    assert rc == 1 and b"null buffer" in msg
    # a good arming: the run that follows owns it (and fills n_used where there is a device), the one after does not
    o.loss = loss.ctypes.data
    assert L.bmm_set_partition_summary(C.byref(o)) == 0
    rc, _ = run()
    assert rc in (0, 3, 4)
    assert n_used.value == (S if rc == 0 else -7)
    n_used.value = -7
    rc2, _ = run()
    assert rc2 == rc and n_used.value == -7
    # entry points that return before they reach the run itself disarm too: a NULL pred, a NULL rel, and
    # bmm_multi_run, which takes no summary
    base = (_capi.vp(X), C.c_int64(N), C.c_int(P), _capi.vp(z0), C.c_int(S + 2), C.c_int(K), C.c_double(1.0),
            C.c_double(0.5), C.c_double(0.5), C.c_double(1), C.c_double(1), C.c_int(2), C.c_int64(0), C.c_uint64(1),
            C.c_int(0), _capi.vp(z), _capi.vp(th), _capi.vp(al))
    early = [lambda: L.bmm_collapsed_run_predict(*base, _capi.vp(X), C.c_int64(0), None),
             lambda: L.bmm_collapsed_run_relabel(*base, None),
             lambda: L.bmm_multi_run(C.c_int(0), C.c_int(0), None, _capi.vp(X), C.c_int64(N), C.c_int(P), None, None, None,
                                     C.c_int(S + 2), C.c_int(K), C.c_double(1.0), C.c_double(0.5), C.c_double(0.5),
                                     C.c_double(1), C.c_double(1), C.c_int(2), C.c_int64(0), C.c_uint64(1), None, None,
                                     None, None)]
    for call in early:
        n_used.value = -7
        assert L.bmm_set_partition_summary(C.byref(o)) == 0
        assert call() == 1
        rc4, _ = run()
        assert rc4 == rc and n_used.value == -7
    # NULL disarms
    o.stride = 0
    assert L.bmm_set_partition_summary(C.byref(o)) == 0 and L.bmm_set_partition_summary(None) == 0
    rc3, msg = run()
    assert rc3 == rc
