"""An ensemble of exact chains (include/bmm_mcmc.h "ensemble of exact chains"): what needs no
device -- bmm_ensemble_plan against hand-derived values, every refusal of the library with its code and word, the
wrapper's refusals ahead of the library, the public names, and that the four Gibbs wrappers are as recorded."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi

E_ARG, E_UNSUPPORTED = 1, 2
LDS = 160 * 1024


def _slice(P, K, Kc):
    """(4 P Kc terms + 256 exponentials) doubles and K P counts, rounded up to 16 bytes"""
    b = (4 * P * Kc + 256) * 8 + K * P * 4
    return (b + 15) // 16 * 16


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize("sampler,N,P,K,chains,want", [
    # K = 2, P = 5: 40 terms + 256 doubles = 2368 bytes, 10 counts = 40 -> 2408, rounded 2416; four chains a workgroup
    ("collapsed", 130, 5, 2, 5, dict(group_width=5, lds_bytes_per_chain=2416, chains_per_workgroup=4, workgroups=2, launches_per_sweep=1,
                                     state_bytes=5 * (130 * 4 + 2 * 4 + 10 * 4 + 8), bytes_per_kept_sweep=5 * (2 * 4 + 10 * 8 + 8),
                                     label_bytes_per_kept_sweep=5 * 130 * 4)),
    # DP, maxK = 63: 64 categories; 4 * 12 * 64 = 3072 terms + 256 = 26624 bytes, 63 * 12 counts = 3024 -> 29648
    # P = 12: two passes, 1024 rows a launch
    ("dp", 2000, 12, 63, 300, dict(lds_bytes_per_chain=29648, chains_per_workgroup=4, workgroups=75, launches_per_sweep=2,
                                  state_bytes=300 * (2000 * 4 + 63 * 4 + 63 * 12 * 4 + 8), bytes_per_kept_sweep=300 * (63 * 4 + 63 * 12 * 8 + 8),
                                  label_bytes_per_kept_sweep=300 * 2000 * 4)),
    # K = 20, P = 112: 8960 terms + 256 = 73728 bytes, 2240 counts = 8960 -> 82688: one chain a workgroup; width 4;
    # 14 passes of logs a move: 2048 / 14 = 146 -> 128 rows a launch, 33 launches over 4100 rows
    ("collapsed", 4100, 112, 20, 7, dict(group_width=4, lds_bytes_per_chain=82688, chains_per_workgroup=1, workgroups=7, launches_per_sweep=33,
                                         state_bytes=7 * (4100 * 4 + 20 * 4 + 2240 * 4 + 8), bytes_per_kept_sweep=7 * (20 * 4 + 2240 * 8 + 8),
                                         label_bytes_per_kept_sweep=7 * 4100 * 4)),
])
def test_plan_against_hand_derived_values(oracle, sampler, N, P, K, chains, want):
    p = bm.ensemble_plan(sampler, N, P, K, chains)
    Kc = K + (sampler == "dp")
    assert p["lds_bytes_per_chain"] == _slice(P, K, Kc)
    assert p["chains_per_workgroup"] == min(4, LDS // _slice(P, K, Kc))
    assert p["group_width"] == oracle.lib().oracle_group_width_for(C.c_int({"collapsed": 0, "dp": 1}[sampler]), C.c_int(K), C.c_int(P))
    for key, v in want.items():
        assert p[key] == v, (key, p[key], v)


# ---------------------------------------------------------------- refusals of the library, before a device is touched
def _refused(rc, code, word):
    msg = _capi.lib().bmm_last_error().decode()
    assert rc == code, (rc, msg)
    assert word in msg, msg


def _plan(sampler, N, P, K, chains):
    out = np.zeros(8, dtype=np.int64)
    return _capi.lib().bmm_ensemble_plan(C.c_int(sampler), C.c_int64(N), C.c_int(P), C.c_int(K), C.c_int(chains), _capi.vp(out))


def _run(sampler, N, P, K, chains, beta=0.5, gamma=0.5, z0=None, nsamples=5):
    """bmm_ensemble_run on a zero matrix with every buffer in place"""
    X = np.zeros((N, P), dtype=np.int32, order="F")
    S = nsamples - 1
    n = max(chains, 1)
    if z0 is None and sampler == 0:
        z0 = [np.ones(N, dtype=np.int32) for _ in range(n)]
    z = [np.zeros((S, N), dtype=np.int32, order="F") for _ in range(n)]
    nk = [np.zeros((S, K), dtype=np.int32) for _ in range(n)]
    th = [np.zeros((K, P, S), order="F") for _ in range(n)]
    al = [np.zeros(S) for _ in range(n)]
    zl = [np.zeros(N, dtype=np.int32) for _ in range(n)]
    keep = (X, z0, z, nk, th, al, zl)
    rc = _capi.lib().bmm_ensemble_run(
        C.c_int(sampler), _capi.vp(X), C.c_int64(N), C.c_int(P), C.c_int(chains), bm._ptr_table(z0) if z0 is not None else None,
        C.c_int(nsamples), C.c_int(K), C.c_double(1.0), C.c_double(beta), C.c_double(gamma), C.c_double(1), C.c_double(1), C.c_int(1),
        C.c_uint64(1), C.c_int(0), bm._ptr_table(z), bm._ptr_table(nk), bm._ptr_table(th), bm._ptr_table(al), bm._ptr_table(zl))
    del keep
    return rc


CASES = [
    # (sampler, N, P, K, chains, code, word)
    (0, 100, 5, 65, 4, E_UNSUPPORTED, "65 categories exceed 64"),
    (1, 100, 5, 64, 4, E_UNSUPPORTED, "65 categories exceed 64"),   # the DP's new cluster is a category
    (0, 100, 129, 3, 4, E_UNSUPPORTED, "at most 128 features"),
    (0, 65536, 5, 3, 4, E_UNSUPPORTED, "fewer than 65536 observations"),
    (0, 100, 128, 64, 4, E_UNSUPPORTED, "do not fit in the 163840 bytes of LDS"),
    (0, 100, 5, 3, 0, E_ARG, "chains must be >= 1"),
    (0, 100, 5, 3, -2, E_ARG, "chains must be >= 1"),
    (2, 100, 5, 3, 4, E_UNSUPPORTED, "collapsed and DP samplers only"),
    (3, 100, 5, 3, 4, E_UNSUPPORTED, "collapsed and DP samplers only"),
    (1, 100, 5, 1, 4, E_ARG, "maxK must be >= 2"),
]


@pytest.mark.parametrize("sampler,N,P,K,chains,code,word", CASES)
def test_the_plan_and_the_run_refuse_alike(sampler, N, P, K, chains, code, word):
    _refused(_plan(sampler, N, P, K, chains), code, word)
    _refused(_run(sampler, N, P, K, chains), code, word)


def test_the_limits_themselves_are_accepted():
    for sampler, N, P, K in ((0, 65535, 5, 64), (1, 65535, 128, 3), (1, 100, 5, 63)):
        assert _plan(sampler, N, P, K, 1) == 0, _capi.lib().bmm_last_error().decode()


def test_the_run_refuses_a_dp_with_unequal_priors_and_bad_arguments():
    _refused(_run(1, 50, 5, 6, 2, beta=0.5, gamma=0.7), E_ARG, "non-symmetric priors")
    _refused(_run(0, 50, 5, 3, 2, z0=[np.ones(50, dtype=np.int32), np.full(50, 4, dtype=np.int32)]), E_ARG, "initialK out of range: chain 1")
    _refused(_run(0, 50, 5, 3, 2, nsamples=1), E_ARG, "burnin must be in [0, nsamples)")
    _refused(_run(0, 50, 5, 3, 2, beta=0.0), E_ARG, "beta and gamma must be > 0")


def test_an_armed_run_option_is_refused_and_disarmed():
    L = _capi.lib()
    lv = np.array([1] * 5, dtype=np.int32)
    assert L.bmm_set_categorical(_capi.vp(lv), C.c_int(lv.size)) == 0
    _refused(_run(0, 50, 5, 3, 2), E_UNSUPPORTED, "no run option is offered")
    assert L.bmm_set_split_merge(C.c_int(1), C.c_int(2)) == 0
    _refused(_run(1, 50, 5, 6, 2), E_UNSUPPORTED, "no run option is offered")
    # nothing stays armed: the next refusal is the next call's own
    _refused(_run(0, 50, 5, 65, 2), E_UNSUPPORTED, "65 categories exceed 64")


# ---------------------------------------------------------------- the wrapper refuses before the library is asked
def test_the_wrapper_refuses_before_the_run_is_asked(monkeypatch):
    def never(*args):
        raise AssertionError("the library's run was asked")

    monkeypatch.setattr(bm, "_ensemble_run", never)
    X = np.zeros((40, 5), dtype=np.int32)
    with pytest.raises(ValueError, match="chains must be >= 1"):
        bm.gibbs_ensemble(X, 5, 3, chains=0)
    for sampler in ("stickbreaking", "full", "allocation"):
        with pytest.raises(ValueError, match='"collapsed" or "dp"'):
            bm.gibbs_ensemble(X, 5, 3, sampler=sampler)
    with pytest.raises(ValueError, match="beta == gamma"):
        bm.gibbs_ensemble(X, 5, 6, sampler="dp", beta=0.5, gamma=0.6)
    with pytest.raises(ValueError, match="one start per chain"):
        bm.gibbs_ensemble(X, 5, 3, chains=3, initial_K=[np.ones(40), np.ones(40)])
    with pytest.raises(ValueError, match="one label per observation"):
        bm.gibbs_ensemble(X, 5, 3, chains=2, initial_K=[np.ones(40), np.ones(39)])
    with pytest.raises(ValueError, match="no initial_K"):
        bm.gibbs_ensemble(X, 5, 6, sampler="dp", chains=1, initial_K=[np.ones(40)])
    with pytest.raises(ValueError, match="burnin"):
        bm.gibbs_ensemble(X, 5, 3, burnin=5)
    for kw, word in ((dict(K=65), "65 categories exceed 64"), (dict(K=64, sampler="dp"), "65 categories exceed 64")):
        with pytest.raises(bm.BmmError, match=word) as e:
            bm.gibbs_ensemble(X, 5, kw.pop("K"), **kw)
        assert e.value.code == E_UNSUPPORTED
    with pytest.raises(bm.BmmError, match="at most 128 features") as e:
        bm.gibbs_ensemble(np.zeros((40, 129), dtype=np.int32), 5, 3)
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(bm.BmmError, match="fewer than 65536 observations") as e:
        bm.gibbs_ensemble(np.zeros((65536, 2), dtype=np.int32), 5, 3)
    assert e.value.code == E_UNSUPPORTED


def test_the_new_names_are_public():
    for name in ("gibbs_ensemble", "ensemble_plan"):
        assert name in bm.__all__ and callable(getattr(bm, name))
    for sym in ("bmm_ensemble_plan", "bmm_ensemble_run"):
        assert sym in _capi.SYMBOLS and hasattr(_capi.lib(), sym)


def test_the_four_wrappers_are_as_recorded():
    """the signatures and docstrings tests/golden/run_api.json records: tests/test_run_driver_cpu.py, run as it stands"""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.join(here, "test_run_driver_cpu.py"),
                        "-k", "signature_and_docstring"], capture_output=True, text=True, cwd=os.path.dirname(here))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
