"""Categorical features (include/bmm_mcmc.h "categorical features"): what needs no device -- the
plan and the column map against hand-derived values, every refusal of a run, bm.categorical, and the code-object
metadata of the two new kernels."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi, build

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref as cr  # noqa: E402

E_ARG, E_UNSUPPORTED = 1, 2


# ---------------------------------------------------------------- plan and column map
def test_plan_and_column_map_against_hand_derived_values():
    p = bm.categorical_plan("collapsed", 300, 3, [3, 1])
    assert p["P"] == 4 and p["n_blocks"] == 1 and not p["generic"] and not p["builds_own_tables"]
    np.testing.assert_array_equal(p["first_column"], [0, 3])
    np.testing.assert_array_equal(p["lev"], [3, 3, 3, 0])
    # a block over columns 28 .. 32: across a plane word
    p = bm.categorical_plan("dp", 300, 5, [1] * 28 + [5] + [1] * 4)
    assert p["P"] == 37 and p["n_blocks"] == 1
    np.testing.assert_array_equal(p["first_column"], list(range(29)) + [33, 34, 35, 36])
    np.testing.assert_array_equal(p["lev"], [0] * 28 + [5] * 5 + [0] * 4)
    # P = 130: the generic kernels; a block of 6 over columns 116 .. 121, across the chunk boundary at 120
    lv = [4] * 29 + [6] + [1] * 8
    p = bm.categorical_plan("collapsed", 300, 4, lv)
    assert p["P"] == 130 and p["n_blocks"] == 30 and p["generic"] and not p["packed"]
    assert p["first_column"][29] == 116 and p["first_column"][30] == 122
    np.testing.assert_array_equal(p["lev"], cr.column_map(lv)[1])
    # neighbouring blocks of one length stay apart in the map; blocks of 2 are blocks
    p = bm.categorical_plan("dp", 1000, 10, [2, 2, 3, 3])
    np.testing.assert_array_equal(p["first_column"], [0, 2, 4, 7])
    np.testing.assert_array_equal(p["lev"], [2, 2, 2, 2, 3, 3, 3, 3, 3, 3])
    # the packed form goes by the rule every chain has: a launch that gives a wave four chunks (batch >= 4 x 256 compute
    # units x the workgroup's threads).  Ten 5-level features at K = 20: not at a million rows (batch 250 000), at eight
    # million (batch 2 000 000 >= 4 x 256 x 1024 whatever the workgroup) it is, and never self-built tables
    p = bm.categorical_plan("collapsed", 1_000_000, 20, [5] * 10)
    assert p["P"] == 50 and not p["packed"] and not p["builds_own_tables"] and p["batch"] == bm.default_batch("collapsed", 1_000_000) == 250_000
    p = bm.categorical_plan("collapsed", 8_000_000, 20, [5] * 10)
    assert p["batch"] == 2_000_000 and p["packed"] and not p["builds_own_tables"] and p["threads"] <= 1024
    # ... and a shape whose plain chain builds its own tables does not as a categorical chain
    for N, K, P in ((300, 3, 4), (2000, 3, 10), (5000, 4, 20)):
        assert not bm.categorical_plan("collapsed", N, K, [1] * P)["builds_own_tables"]


def test_plan_refuses_what_the_chain_refuses():
    for levels, word in (([3, 0, 2], "feature 1 has 0 levels"), ([2, -1], "feature 1 has -1 levels"), ([256], "at most 255")):
        with pytest.raises(bm.BmmError, match=word) as e:
            bm.categorical_plan("dp", 100, 5, levels)
        assert e.value.code == E_ARG
    for sampler in ("stickbreaking", "full"):
        with pytest.raises(bm.BmmError) as e:
            bm.categorical_plan(sampler, 100, 5, [3, 1])
        assert e.value.code == E_UNSUPPORTED


# ---------------------------------------------------------------- refusals of a run, before a device is touched
N, P, K, NS = 40, 6, 3, 5
LEVELS = np.array([3, 1, 2], dtype=np.int32)


def _x():
    return cr.expand(cr.draw(N, [3, 1, 2], 0)[0], [3, 1, 2])[0]


def _args(spec, X, K):
    S = NS - 1
    z = np.zeros((S, N), dtype=np.int32, order="F")
    theta = np.zeros((K, X.shape[1], S), order="F")
    al = np.zeros((S, 1), order="F")
    pi = np.zeros((S, K), order="F")
    start = np.ones(N, dtype=np.int32) if spec.start == "labels" else None
    if spec.start == "params":
        start = bm._start_params(1, None, None, K, X.shape[1])
    keep = (z, theta, al, pi, start, X)
    return bm._run_args(spec, X, start, NS, K, 1.0, 0.5, 0.5, 1, 1, 1, None, 1, 0, pi, z, theta, al), keep


def _arm_levels(levels=LEVELS):
    lv = np.ascontiguousarray(levels, dtype=np.int32)
    assert _capi.lib().bmm_set_categorical(_capi.vp(lv), C.c_int(lv.size)) == 0


def _refused(rc, code, word):
    msg = _capi.lib().bmm_last_error().decode()
    assert rc == code, (rc, msg)
    assert word in msg, msg


class _NeverAsked:
    """host relabelling code behind the hooks of a run that is refused"""

    def batch(self, p):
        raise AssertionError("the run was not refused")

    online = batch


def test_bad_levels_are_an_argument_error_before_a_device_is_touched():
    """(a machine without a device answers a call that reaches one with another code)"""
    X = _x()
    L = _capi.lib()
    for levels, word in (([3, 1, 0, 2], "feature 2 has 0 levels"), ([3, 1, 1], "take 5 columns"), ([3, 1, 2, 1], "take 7 columns"),
                         ([-2, 8], "feature 0 has -2 levels")):
        for spec in (bm._COLLAPSED, bm._DP):
            _arm_levels(levels)
            args, keep = _args(spec, X, K)
            _refused(getattr(L, "bmm_%s_run_probs" % spec.base)(*args, None), E_ARG, word)
    assert L.bmm_set_categorical(None, C.c_int(3)) == E_ARG
    assert L.bmm_set_categorical(_capi.vp(LEVELS), C.c_int(-1)) == E_ARG


def test_every_refused_pairing_comes_back_unsupported_in_either_order_of_arming():
    X = _x()
    L = _capi.lib()
    S = NS - 1
    feat = np.arange(3, dtype=np.int32)
    options = {
        "parallel tempering": lambda: bm._Temper([1.0, 0.5], 1, S),
        "feature selection": lambda: bm._Features(0.5, P, S),
        "split-merge": lambda: bm._SplitMerge(1, 2),
        "missing": lambda: bm._Missing(np.array([1], dtype=np.int64), np.array([2], dtype=np.int32), N, P),
        "leave-one-out": lambda: bm._Loo(N, S),
        "log joint": lambda: bm._LogPost(N, S),
        "pair check": lambda: bm._PairFold(feat, 1, S),
        "init_labels": lambda: bm._Init(1, 3),
    }
    for word, make in options.items():
        for spec in (bm._COLLAPSED, bm._DP):
            for levels_first in (True, False):
                o = make()
                if levels_first:
                    _arm_levels()
                o.arm()
                if not levels_first:
                    _arm_levels()
                args, keep = _args(spec, X, K)
                _refused(getattr(L, "bmm_%s_run_probs" % spec.base)(*args, None), E_UNSUPPORTED, word)
    # the other samplers
    for spec in (bm._STICKBREAKING, bm._FULL):
        _arm_levels()
        args, keep = _args(spec, X, K)
        _refused(getattr(L, "bmm_%s_run_probs" % spec.base)(*args, None), E_UNSUPPORTED, "collapsed and DP samplers only")
    # newdata, relabel = TRUE on the device and through the hooks
    for spec in (bm._COLLAPSED, bm._DP):
        _arm_levels()
        args, keep = _args(spec, X, K)
        pr = bm._Predict(X[:4], P, S, K + spec.new_column, False, False, 1)
        pr.arm()
        _refused(getattr(L, "bmm_%s_run_predict" % spec.base)(*args, _capi.vp(pr.X), C.c_int64(pr.M), C.byref(pr.s)), E_UNSUPPORTED, "newdata")
        _arm_levels()
        rel = bm._DeviceRelabelRun(N, K, P, S, 2)
        _refused(getattr(L, "bmm_%s_run_relabel" % spec.base)(*args, rel.ref()), E_UNSUPPORTED, "relabel = TRUE")
        _arm_levels()
        hooks = bm._Relabel(_NeverAsked(), N, K, NS, 1, 1)
        _refused(getattr(L, "bmm_%s_run_probs" % spec.base)(*args, hooks.ref()), E_UNSUPPORTED, "relabel = TRUE")
    # the allocation sampler and the run of several chains
    _arm_levels()
    with pytest.raises(bm.BmmError, match="allocation sampler") as e:
        bm.gibbs_allocation(np.asarray(X), NS, 4, burnin=1, seed=1)
    assert e.value.code == E_UNSUPPORTED
    _arm_levels()
    with pytest.raises(bm.BmmError, match="several chains") as e:
        bm.gibbs_collapsed(np.asarray(X), NS, K, burnin=1, seed=1, chains=2)
    assert e.value.code == E_UNSUPPORTED
    # ... after which nothing is armed: a refused call disarms
    assert not bm.categorical_plan("dp", N, K, LEVELS)["generic"]


def test_the_int32_layout_is_refused(dbg_lib):
    dbg_lib.setenv("BMM_X_LAYOUT_INT32", "1")
    X = _x()
    for spec in (bm._COLLAPSED, bm._DP):
        _arm_levels()
        args, keep = _args(spec, X, K)
        _refused(getattr(_capi.lib(), "bmm_%s_run_probs" % spec.base)(*args, None), E_UNSUPPORTED, "int32 layout")


# ---------------------------------------------------------------- bm.categorical
def test_categorical_round_trips():
    Xc = np.array([[0, 1, 2, 0], [2, 0, 3, 1], [1, 1, 0, 1], [2, 1, 1, 0]])
    D = bm.categorical(Xc)
    np.testing.assert_array_equal(D.levels, [3, 2, 4, 2])
    np.testing.assert_array_equal(D.chain_levels, [3, 1, 4, 1])
    assert D.columns == [slice(0, 3), slice(3, 4), slice(4, 8), slice(8, 9)]
    assert D.shape == (4, 9) and D.dtype == np.int32 and D.flags.f_contiguous
    np.testing.assert_array_equal(np.asarray(D), [[1, 0, 0, 1, 0, 0, 1, 0, 0], [0, 0, 1, 0, 0, 0, 0, 1, 1], [0, 1, 0, 1, 1, 0, 0, 0, 1],
                                                  [0, 0, 1, 1, 0, 1, 0, 0, 0]])
    # the same columns as the raw vector's expansion
    np.testing.assert_array_equal(np.asarray(D), cr.expand(Xc, D.chain_levels)[0])
    # back to the level indices
    back = np.stack([np.asarray(D)[:, sl].argmax(axis=1) if L > 2 else np.asarray(D)[:, sl.start] for L, sl in zip(D.levels, D.columns)], axis=1)
    np.testing.assert_array_equal(back, Xc)
    # explicit levels: room for levels nobody has
    E = bm.categorical(Xc, levels=[4, 2, 5, 3])
    assert E.shape == (4, 1 + 4 + 5 + 3) and E.columns[3] == slice(10, 13)
    # decode: theta of a chain, per feature; a two-level feature's (1 - theta, theta)
    theta = np.arange(2 * 9, dtype=np.float64).reshape(2, 9) / 100.0
    dec = D.decode(theta)
    assert [d.shape for d in dec] == [(2, 3), (2, 2), (2, 4), (2, 2)]
    np.testing.assert_array_equal(dec[0], theta[:, 0:3])
    np.testing.assert_array_equal(dec[1], np.stack([1.0 - theta[:, 3], theta[:, 3]], axis=1))
    assert D.decode(np.zeros((2, 9, 5)))[2].shape == (2, 4, 5)
    with pytest.raises(ValueError):
        D.decode(np.zeros((2, 8)))
    # only the object itself says what it is
    assert bm._categorical_of(D) is D and bm._categorical_of(np.asarray(D)) is None and bm._categorical_of(D[:2]) is None


def test_categorical_refuses_values_outside_a_features_levels():
    Xc = np.array([[0, 1], [2, 0]])
    with pytest.raises(ValueError, match="row 1, feature 0: the value 2"):
        bm.categorical(Xc, levels=[2, 2])
    with pytest.raises(ValueError, match="row 0, feature 1: the value -1"):
        bm.categorical(np.array([[0, -1]]))
    with pytest.raises(ValueError, match="at least 2"):
        bm.categorical(Xc, levels=[3, 1])
    with pytest.raises(ValueError, match="at most 255"):
        bm.categorical(Xc, levels=[3, 256])
    with pytest.raises(ValueError):
        bm.categorical(Xc.astype(np.float64))
    with pytest.raises(ValueError):
        bm.categorical(Xc, levels=[3])


def test_the_wrappers_refuse_before_the_library_is_asked(monkeypatch):
    """every other wrapper, and every option whose scorer knows the Bernoulli cell only"""
    monkeypatch.setattr(_capi, "lib", lambda: pytest.fail("the library was asked"))
    D = bm.categorical(cr.draw(60, [3, 2, 4], 1)[0])
    z = np.ones((3, 60), dtype=np.int32)
    for fn, args in ((bm.gibbs_stickbreaking, (D, 5, 3)), (bm.gibbs_full, (D, 5, 3)), (bm.gibbs_allocation, (D, 5, 3)),
                     (bm.log_joint, (D, z, "dp", 3)), (bm.pair_check, (D, z, 3))):
        with pytest.raises(ValueError, match="Bernoulli cell"):
            fn(*args)
    refused = dict(chains=2, temper=2, select_features=True, missing="na", newdata=np.asarray(D)[:3], loo=True, logpost=True,
                   ecr_pivot="map", pair_check=True, relabel=True)
    for fn, args, extra in ((bm.gibbs_collapsed, (D, 5, 3), dict(init="kmodes")), (bm.gibbs_dp, (D, 5), dict(split_merge=1))):
        for k, v in {**refused, **extra}.items():
            with pytest.raises(ValueError, match="categorical data"):
                fn(*args, seed=1, **{k: v})


# ---------------------------------------------------------------- the code objects
def _tool(name):
    root = os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc())))
    for path in (os.path.join(root, "llvm", "bin", name), os.path.join(root, "lib", "llvm", "bin", name)):
        if os.path.exists(path):
            return path
    raise AssertionError("%s not found beside hipcc" % name)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """kernel name -> its metadata block, from the notes of the library's gfx950 code object"""
    if build.stale(build.LIB):
        build.build()
    d = tmp_path_factory.mktemp("codeobj")
    fat, co = str(d / "fat.bin"), str(d / "lib.co")
    subprocess.run([_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", build.LIB, fat], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                    "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in notes.split("- .agpr_count")[1:]:
        out[re.search(r"\.name:\s+(\S+)", blk).group(1)] = blk
    return out


# the categorical flavour of the sweep's table build (TAB_CAT) and the one-hot check
@pytest.mark.parametrize("pattern", ["k_count_tablesILi4E", "k_cat_check"])
def test_no_private_segment_and_no_spills(kernels, pattern):
    names = [n for n in kernels if pattern in n]
    assert len(names) == 1, names
    blk = kernels[names[0]]
    field = lambda key: re.search(r"\.%s:\s+(\S+)" % key, blk).group(1)  # noqa: E731
    print(names[0], {k: field(k) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size")})
    assert field("private_segment_fixed_size") == "0"
    assert field("uses_dynamic_stack") == "false"
    assert field("vgpr_spill_count") == "0" and field("sgpr_spill_count") == "0"
