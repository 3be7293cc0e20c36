"""k_resample_pk's pipelined body: a trip of the tile loop scores chunk i and, in the same straight-line code, runs the
packed draw of chunk i - 1; the settling path, the DP's books and the movers run a trip late, on the words, the label
and the uniform the wave has carried from the chunk before.  None of this may change a label.

The test variant runs with BMM_DEBUG_NOSPLIT, BMM_DEBUG_NOSELF, BMM_DEBUG_PK and BMM_DEBUG_CUS=1 as in
tests/test_gpu_pk_lean.py, so that one workgroup takes every chunk, and every chain is asked whether its kernel is the
packed one and whether it runs the pipelined body (bmm_dbg_kernel_pk_pipelined): no case passes by running the other
body.  Eight sweeps of z, theta and alpha equal the oracle chain bit for bit.

Fill and drain of the pipeline (collapsed, K = 20, P = 100: sixteen waves, twenty groups, ten pairs):
  N = 700               eleven chunks: waves without a tile, and no wave with a second chunk (prologue and epilogue only)
  N = 1025              seventeen chunks: one wave has two, the last chunk holds one observation
  N = 3072              three chunks per wave
  N = 5000, batch 2500  the benchmark's form, a ragged last chunk, the second launch of a sweep with lo > 0
Slices against steps (G groups, KT/2 pairs):
  K = 20, P = 4         G = 1: no round is whole, every slice follows the rolled loop
  K = 20, P = 50        G = 10 = KT/2: the first round whole, the second empty
  K = 20, P = 73        G = 15: between one round and two
  K = 4, largest P      G beyond two rounds: the rolled loop behind the two unrolled rounds, four words
  K = 32, P = 61        groups of four, 16 pairs: that form keeps the present body (pk_pipelined); the chain must
                        say so, and still equals the oracle
A field across a word boundary: K = 12, P = 33.
DP: maxK = 12, N = 4000, P = 24, batch 333 -- the first sweep with zo = -1, the new-cluster books a trip late, many lo.
Settling a trip late: BMM_DEBUG_PK_DEFER_EVERY = 3 and 64 and everything deferred (BMM_DEBUG_DRAW_FALLBACK) on the
N = 5000 and N = 1025 shapes: the definition must read the words, the label and the uniform of the chunk before.
Movers a trip late: the chains start from a uniformly random allocation, so the first sweeps move nearly every lane;
after sweep 1 the cluster sizes and feature counts equal a recount from the labels.
Both Philox forms: BMM_DEBUG_PK_GENKEY on the N = 5000 shape.
Both bodies: the N = 5000 shape under BMM_DEBUG_PK_NOPIPE runs the present body and equals the oracle too."""
import ctypes

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi
from util import synth

pytestmark = pytest.mark.gpu

SWITCHES = ("DRAW_FALLBACK", "DRAW_NOEPS", "NOSPLIT", "NOSELF", "CUS", "PK_QUEUE", "PK_DEFER_EVERY", "PK_GENKEY", "NOPK",
            "PK", "PK_NOPIPE", "THREADS", "SPLIT", "SMALL", "GENERIC")
SWEEPS = 8
KEYS = ("z", "theta", "alpha")


def _largest_packed_p(K):
    f = _capi.lib().bmm_spec_pk_image_bytes
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_int] * 4
    g = _capi.lib().bmm_spec_group_width_for
    return max(P for P in range(1, 129) if f(0, K, P, g(0, K, P)) > 0)


# name -> (sampler, N, P, K or maxK, batch)
def _cases():
    return {
        "N700": ("collapsed", 700, 100, 20, 700),
        "N1025": ("collapsed", 1025, 100, 20, 1025),
        "N3072": ("collapsed", 3072, 100, 20, 3072),
        "N5000": ("collapsed", 5000, 100, 20, 2500),
        "G1": ("collapsed", 2500, 4, 20, 2500),
        "G10": ("collapsed", 2500, 50, 20, 2500),
        "G15": ("collapsed", 2500, 73, 20, 2500),
        "K4": ("collapsed", 1500, _largest_packed_p(4), 4, 1500),
        "K32": ("collapsed", 3000, 61, 32, 700),
        "word": ("collapsed", 2500, 33, 12, 2500),
        "dp": ("dp", 4000, 24, 12, 333),
    }


NAMES = ("N700", "N1025", "N3072", "N5000", "G1", "G10", "G15", "K4", "K32", "word", "dp")


def _set(mp, **on):
    for k in SWITCHES:
        mp.delenv("BMM_DEBUG_" + k, raising=False)
    for k, v in dict(NOSPLIT=1, NOSELF=1, PK=1, CUS=1, **on).items():
        if v:
            mp.setenv("BMM_DEBUG_" + k, str(int(v)))


def _data(case):
    sampler, N, P, K = case[:4]
    X = synth(N, P, 4, 11 * K + P)[0]
    z0 = np.random.default_rng(5).integers(1, K + 1, N).astype(np.int32)
    return X, z0


def _run(case):
    sampler, N, P, K, batch = case
    X, z0 = _data(case)
    if sampler == "dp":
        return bm.gibbs_dp(X, SWEEPS, burnin=0, maxK=K, seed=47, batch=batch)
    return bm.gibbs_collapsed(X, SWEEPS, K, burnin=0, seed=53, batch=batch, initial_K=z0)


def _want(oracle, case):
    sampler, N, P, K, batch = case
    X, z0 = _data(case)
    if sampler == "dp":
        return oracle.dp(X, SWEEPS, 0.0, 0.5, 0.5, 1, 1, 0, K, seed=47, batch=batch)
    return oracle.collapsed(X, z0, SWEEPS, K, 0.0, 0.5, 0.5, 1, 1, 0, seed=53, batch=batch)


def _body(case):
    """(the chain's kernel is the packed one, it runs the pipelined body)"""
    sampler, N, P, K, batch = case
    with bm.Chain(sampler, N, P, K, batch=batch, seed=53) as c:
        L = _capi.lib()
        return bool(L.bmm_dbg_kernel_packed(c._h)), bool(L.bmm_dbg_kernel_pk_pipelined(c._h))


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), (k, what)


@pytest.fixture(scope="module")
def cases():
    return _cases()


_WANTED = {}


@pytest.fixture(scope="module")
def wanted(oracle, cases):
    def get(name):  # an oracle chain is computed once, by the first test that asks for it
        if name not in _WANTED:
            _WANTED[name] = _want(oracle, cases[name])
        return _WANTED[name]
    return get


def test_the_shapes_are_what_they_are_for(cases):
    g = _capi.lib().bmm_spec_group_width_for
    groups = {n: -(-cases[n][2] // g(0, cases[n][3], cases[n][2])) for n in ("N5000", "G1", "G10", "G15", "K4")}
    assert [groups[n] for n in ("N5000", "G1", "G10", "G15")] == [20, 1, 10, 15], groups
    assert groups["K4"] > 4 and cases["K4"][2] > 96, (groups, cases["K4"])  # beyond two rounds of two pairs; four words


@pytest.mark.parametrize("name", NAMES)
def test_pipelined_chain_matches_the_oracle(wanted, cases, dbg_lib, name):
    _set(dbg_lib)
    packed, piped = _body(cases[name])
    assert packed, cases[name]
    # the decision per form (pk_pipelined, kernels.hip.h): the 1024-thread forms of up to 20 accumulators; the 32
    # accumulators of K = 32 run at 768 threads and keep the present body
    assert piped == (name != "K32"), (cases[name], piped)
    print(name, cases[name], "pipelined" if piped else "present body")
    _same(_run(cases[name]), wanted(name), cases[name])


@pytest.mark.parametrize("name", ["N5000", "N1025"])
@pytest.mark.parametrize("how", ["every third lane deferred", "every 64th lane deferred", "everything deferred"])
def test_lanes_settled_a_trip_late(wanted, cases, dbg_lib, name, how):
    _set(dbg_lib, PK_DEFER_EVERY=3 if "third" in how else 64 if "64th" in how else 0, DRAW_FALLBACK="everything" in how)
    assert _body(cases[name]) == (True, True), (name, how)
    _same(_run(cases[name]), wanted(name), (name, how))


def test_general_key_form(wanted, cases, dbg_lib):
    _set(dbg_lib, PK_GENKEY=1)
    assert _body(cases["N5000"]) == (True, True)
    _same(_run(cases["N5000"]), wanted("N5000"), "general key form")


def test_present_body_on_request(wanted, cases, dbg_lib):
    _set(dbg_lib, PK_NOPIPE=1)
    assert _body(cases["N5000"]) == (True, False)
    present = _run(cases["N5000"])
    _set(dbg_lib)
    assert _body(cases["N5000"]) == (True, True)
    _same(present, _run(cases["N5000"]), "present body against the pipelined one")
    _same(present, wanted("N5000"), "present body against the oracle")


@pytest.mark.parametrize("name", ["N5000", "N1025"])
def test_counts_after_the_first_sweep_are_a_recount(cases, dbg_lib, name):
    _set(dbg_lib)
    sampler, N, P, K, batch = cases[name]
    X, z0 = _data(cases[name])
    with bm.Chain(sampler, N, P, K, batch=batch, seed=53) as c:
        assert _capi.lib().bmm_dbg_kernel_pk_pipelined(c._h) == 1
        c.set_data(X)
        c.set_initial_labels(z0)
        c.sweeps(1)
        z = c.labels()
        Nk, S = c.counts()
    moved = float((z != z0).mean())
    print(name, "moved in the first sweep: %.3f" % moved)
    assert moved > 0.5, moved  # a uniformly random start over twenty clusters: nearly every lane moves
    lab = z.astype(np.int64) - 1
    S_ref = np.zeros((K, P), dtype=np.int32)
    np.add.at(S_ref, lab, np.asarray(X, dtype=np.int32))
    np.testing.assert_array_equal(Nk, np.bincount(lab, minlength=K).astype(np.int32))
    np.testing.assert_array_equal(S, S_ref)
