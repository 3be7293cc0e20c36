"""relabel=True with stephens="device" (Stephens' relabelling on the device): what can be checked without a GPU --
the new C entry points are exported, and the Python front end refuses bad calls before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi

NEW = ["bmm_collapsed_run_relabel", "bmm_dp_run_relabel", "bmm_sb_run_relabel", "bmm_full_run_relabel",
       "bmm_device_stephens_batch", "bmm_device_stephens_online", "bmm_device_stephens_plan"]


def test_stephens_entry_points_are_exported():
    L = _capi.lib()
    for s in NEW:
        assert s in _capi.SYMBOLS
        getattr(L, s)
    assert bm.STEPHENS_MAX_K == 128
    for name in ("stephens_batch", "stephens_online", "stephens_plan", "DeviceStephens"):
        assert name in bm.__all__


def test_device_relabel_validation_needs_no_gpu():
    X = np.zeros((10, 3), dtype=np.int32)
    with pytest.raises(NotImplementedError, match="relabel"):            # several chains: still per chain only
        bm.gibbs_collapsed(X, 10, 2, burnin=4, relabel=True, chains=2, stephens="device")
    with pytest.raises(NotImplementedError, match="relabel"):
        bm.gibbs_stickbreaking(X, 10, 2, burnin=4, relabel=True, chains=2, stephens="device")
    for burnin in (0, 1):                                                # no batch step: the reference has no Q
        with pytest.raises(ValueError, match="burnin >= 2"):
            bm.gibbs_collapsed(X, 10, 2, burnin=burnin, relabel=True, stephens="device")
        with pytest.raises(ValueError, match="burnin >= 2"):
            bm.gibbs_dp(X, 10, burnin=burnin, relabel=True, stephens="device")
        with pytest.raises(ValueError, match="burnin >= 2"):
            bm.gibbs_full(X, 10, 2, burnin=burnin, relabel=True, stephens="device")
    with pytest.raises(ValueError, match="burnrelabel"):
        bm.gibbs_stickbreaking(X, 10, 2, burnin=4, relabel=True, burnrelabel=0, stephens="device")
    with pytest.raises(ValueError, match="stephens"):
        bm.gibbs_collapsed(X, 10, 2, burnin=4, relabel=True, stephens="gpu")
    with pytest.raises(ValueError, match="stephens"):
        bm.gibbs_full(X, 10, 2, burnin=4, relabel=True, stephens="host")
    # stephens=None keeps asking for an implementation, and now names the device one
    with pytest.raises(NotImplementedError, match='stephens="device"'):
        bm.gibbs_collapsed(X, 10, 2, relabel=True)


def test_relabel_entry_points_refuse_before_touching_a_device():
    L = _capi.lib()
    X = np.zeros((10, 3), dtype=np.int32)
    z0 = np.ones(10, dtype=np.int32)
    S = 5
    z = np.zeros((S, 10), dtype=np.int32)
    th = np.zeros((2, 3, S))
    al = np.zeros(S)

    class Out(C.Structure):
        _fields_ = [("burnrelabel", C.c_int), ("permutations", C.c_void_p), ("z_original", C.c_void_p),
                    ("theta_original", C.c_void_p)]

    perms = np.zeros((S, 2), dtype=np.int32)
    rel = Out(2, perms.ctypes.data, z.ctypes.data, th.ctypes.data)

    def run(K, burnin, W, relp=True):
        rel.burnrelabel = W
        return L.bmm_collapsed_run_relabel(_capi.vp(X), C.c_int64(10), C.c_int(3), _capi.vp(z0), C.c_int(burnin + S),
                                           C.c_int(K), C.c_double(1.0), C.c_double(0.5), C.c_double(0.5), C.c_double(1),
                                           C.c_double(1), C.c_int(burnin), C.c_int64(0), C.c_uint64(1), C.c_int(0),
                                           _capi.vp(z), _capi.vp(th), _capi.vp(al), C.byref(rel) if relp else None)

    assert run(2, 1, 1) == 1 and b"burnin >= 2" in L.bmm_last_error()
    assert run(2, 4, 0) == 1 and b"burnrelabel >= 1" in L.bmm_last_error()
    assert run(129, 4, 2) == 1 and b"128" in L.bmm_last_error()
    assert run(2, 4, 2, relp=False) == 1
    Q = np.ones((4, 200))
    perm = np.zeros(200, dtype=np.int32)
    assert L.bmm_device_stephens_online(C.c_int(0), _capi.vp(Q), _capi.vp(Q), C.c_int64(4), C.c_int(200), C.c_int(3),
                                        _capi.vp(perm), _capi.vp(Q), None) == 1
    assert b"128" in L.bmm_last_error()
    p = np.full((4, 2, 1), np.nan)
    assert L.bmm_device_stephens_batch(C.c_int(0), _capi.vp(p), C.c_int64(4), C.c_int(2), C.c_int(1), _capi.vp(Q),
                                       _capi.vp(perm)) == 1
    assert b"finite" in L.bmm_last_error()


def _plan(N, K, M=0):
    p = bm.stephens_plan(N, K, M)
    return [p[k] for k in ("groups_online", "groups_batch", "rows_online", "rows_batch", "blocks_per_thread",
                           "tile_rows", "blocks", "thread_groups", "cost_in_lds", "cols_per_lane")]


def test_stephens_plan_at_shapes_computed_by_hand():
    # G = ceil(N / 512), at most 1024 (ceil(1024 / M) per slice of a batch) and at most 64 MiB / (M K^2 8) partials;
    # rows = ceil(N / G); nb = ceil(K / 4)^2 blocks, ng = 256 // nb groups below 256 blocks, B = ceil(nb / 256)
    # blocks per thread above; 64-row tiles up to K4 = 32, 16 above; cost in LDS while 8 K^2 + 36 (K + 1) <= 65536
    # (K <= 88); columns 0..K over 64 lanes.
    #                                  G1    GM   rows1 rowsM  B   T   nb   ng  lds cols
    assert _plan(1, 1) == [1, 0, 1, 0, 1, 64, 1, 256, 1, 1]
    assert _plan(5003, 20, 4) == [10, 10, 501, 501, 1, 64, 25, 10, 1, 1]
    assert _plan(1000, 10) == [2, 0, 500, 0, 1, 64, 9, 28, 1, 1]              # 28 * 9 = 252: four threads idle
    assert _plan(512, 32) == [1, 0, 512, 0, 1, 64, 64, 4, 1, 1]
    assert _plan(513, 33) == [2, 0, 257, 0, 1, 16, 81, 3, 1, 1]
    assert _plan(700, 50, 2) == [2, 2, 350, 350, 1, 16, 169, 1, 1, 1]
    assert _plan(100, 63) == [1, 0, 100, 0, 1, 16, 256, 1, 1, 1]
    assert _plan(100, 64) == [1, 0, 100, 0, 1, 16, 256, 1, 1, 2]              # column 64 is lane 0's second
    assert _plan(100, 65) == [1, 0, 100, 0, 2, 16, 289, 1, 1, 2]
    assert _plan(100, 88) == [1, 0, 100, 0, 2, 16, 484, 1, 1, 2]              # 8 * 88^2 + 36 * 89 = 65156
    assert _plan(100, 89) == [1, 0, 100, 0, 3, 16, 529, 1, 0, 2]              # 8 * 89^2 + 36 * 90 = 66608
    assert _plan(100, 108) == [1, 0, 100, 0, 3, 16, 729, 1, 0, 2]
    assert _plan(100, 109) == [1, 0, 100, 0, 4, 16, 784, 1, 0, 2]
    assert _plan(100, 127) == [1, 0, 100, 0, 4, 16, 1024, 1, 0, 2]
    assert _plan(100, 128) == [1, 0, 100, 0, 4, 16, 1024, 1, 0, 3]
    # the caps: 1024 workgroups; ceil(1024 / 3) = 342 per slice; 64 MiB / (128^2 * 8) = 512 partials
    assert _plan(524_288, 3) == [1024, 0, 512, 0, 1, 64, 1, 256, 1, 1]
    assert _plan(600_001, 3) == [1024, 0, 586, 0, 1, 64, 1, 256, 1, 1]
    assert _plan(200_003, 3, 3) == [391, 342, 512, 585, 1, 64, 1, 256, 1, 1]
    assert _plan(262_144, 128) == [512, 0, 512, 0, 4, 16, 1024, 1, 0, 3]
    assert _plan(263_001, 128) == [512, 0, 514, 0, 4, 16, 1024, 1, 0, 3]
    assert _plan(1_000_000, 128, 4) == [512, 128, 1954, 7813, 4, 16, 1024, 1, 0, 3]


def test_stephens_plan_refuses_bad_shapes_and_clears_unused_slots():
    L = _capi.lib()
    out = (C.c_int64 * 12)(*([-1] * 12))
    assert L.bmm_device_stephens_plan(C.c_int64(1000), C.c_int(10), C.c_int(0), out) == 0
    assert list(out)[10:] == [0, 0] and out[1] == 0 and out[3] == 0
    for K in (0, 129):
        with pytest.raises(bm.BmmError, match="128"):
            bm.stephens_plan(100, K)
    for N, M in ((0, 0), (100, -1)):
        with pytest.raises(bm.BmmError, match="N must be"):
            bm.stephens_plan(N, 3, M)
    assert L.bmm_device_stephens_plan(C.c_int64(10), C.c_int(3), C.c_int(0), None) == 1
