"""relabel=True with stephens="device" (Stephens' relabelling on the device): what can be checked without a GPU --
the new C entry points are exported, and the Python front end refuses bad calls before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi

NEW = ["bmm_collapsed_run_relabel", "bmm_dp_run_relabel", "bmm_sb_run_relabel", "bmm_full_run_relabel",
       "bmm_device_stephens_batch", "bmm_device_stephens_online"]


def test_stephens_entry_points_are_exported():
    L = _capi.lib()
    for s in NEW:
        assert s in _capi.SYMBOLS
        getattr(L, s)
    assert bm.STEPHENS_MAX_K == 128
    for name in ("stephens_batch", "stephens_online", "DeviceStephens"):
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
