"""k_resample_pk's second body as a plain trip: the present body's order (counter, scoring, substitution and maximum,
draw, settling, labels stored at the head of the next trip) with the lookups in unrolled steps at compile-time groups,
group 0 a step of its own whatever G; pk_draw2 written plainly, no longer over slices.  None of this may change a
label.

The test variant runs with BMM_DEBUG_NOSPLIT, BMM_DEBUG_NOSELF, BMM_DEBUG_PK and BMM_DEBUG_CUS=1 as in
tests/test_gpu_pk_pipe.py, so that one workgroup of sixteen waves takes every chunk, and every chain is asked whether
its kernel is the packed one and which body it runs (bmm_dbg_kernel_packed, bmm_dbg_kernel_pk_pipelined): no case
passes on the other body.  Eight sweeps of z, theta and alpha equal the oracle chain bit for bit.

Chunks per wave (collapsed, K = 20, P = 100: twenty groups, ten pairs, both rounds whole):
  N = 700               eleven chunks: waves without a tile, the others with one
  N = 1025              seventeen chunks: one wave takes a second, and the last chunk holds one observation
  N = 2500              forty chunks: waves with two and with three, a ragged last chunk
  N = 5000, batch 2500  the second launch of a sweep has lo > 0
The steps (G groups, KT/2 pairs):
  K = 20, P = 4         G = 1: group 0's step is the only step
  K = 20, P = 50        G = 10: exactly one whole round
  K = 20, P = 73        G = 15: one round, then the rolled groups
  K = 4, largest P      G beyond two rounds of two pairs: the rolled groups behind both, four words
  K = 12, P = 61        a field across a word boundary (groups of five)
DP: maxK = 12, N = 4000, P = 24, batch 333 -- K + 1 categories, the first sweep with zo = -1, the new-cluster books.
A first sweep from a uniformly random allocation moves nearly every lane: the cluster sizes and feature counts equal
a recount from the labels.
The draw (bmm_dbg_pk_draw against the SPEC kernel, KT = 4 and 20): rows whose leading running sums are exactly 0
with u = 0 (t - c[k] is +0 there and counts), and rows where t equals a running sum exactly: the counts are known
by hand, and no such row is certain.
Both bodies: the N = 2500 shape under BMM_DEBUG_PK_NOPIPE runs the present body and equals the second and the oracle."""
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


def _group_width(K, P):
    return _capi.lib().bmm_spec_group_width_for(0, K, P)


def _largest_packed_p(K):
    f = _capi.lib().bmm_spec_pk_image_bytes
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_int] * 4
    return max(P for P in range(1, 129) if f(0, K, P, _group_width(K, P)) > 0)


# name -> (sampler, N, P, K or maxK, batch)
def _cases():
    return {
        "N700": ("collapsed", 700, 100, 20, 700),
        "N1025": ("collapsed", 1025, 100, 20, 1025),
        "N2500": ("collapsed", 2500, 100, 20, 2500),
        "lo": ("collapsed", 5000, 100, 20, 2500),
        "G1": ("collapsed", 2500, 4, 20, 2500),
        "G10": ("collapsed", 2500, 50, 20, 2500),
        "G15": ("collapsed", 2500, 73, 20, 2500),
        "K4": ("collapsed", 1500, _largest_packed_p(4), 4, 1500),
        "word": ("collapsed", 2500, 61, 12, 2500),
        "dp": ("dp", 4000, 24, 12, 333),
    }


NAMES = ("N700", "N1025", "N2500", "lo", "G1", "G10", "G15", "K4", "word", "dp")


def _set(mp, **on):
    for k in SWITCHES:
        mp.delenv("BMM_DEBUG_" + k, raising=False)
    for k, v in dict(NOSPLIT=1, NOSELF=1, PK=1, CUS=1, **on).items():
        if v:
            mp.setenv("BMM_DEBUG_" + k, str(int(v)))


def _data(case):
    sampler, N, P, K = case[:4]
    X = synth(N, P, 4, 13 * K + P)[0]
    z0 = np.random.default_rng(7).integers(1, K + 1, N).astype(np.int32)
    return X, z0


def _run(case):
    sampler, N, P, K, batch = case
    X, z0 = _data(case)
    if sampler == "dp":
        return bm.gibbs_dp(X, SWEEPS, burnin=0, maxK=K, seed=59, batch=batch)
    return bm.gibbs_collapsed(X, SWEEPS, K, burnin=0, seed=61, batch=batch, initial_K=z0)


def _want(oracle, case):
    sampler, N, P, K, batch = case
    X, z0 = _data(case)
    if sampler == "dp":
        return oracle.dp(X, SWEEPS, 0.0, 0.5, 0.5, 1, 1, 0, K, seed=59, batch=batch)
    return oracle.collapsed(X, z0, SWEEPS, K, 0.0, 0.5, 0.5, 1, 1, 0, seed=61, batch=batch)


def _body(case):
    """(the chain's kernel is the packed one, it runs the second body)"""
    sampler, N, P, K, batch = case
    with bm.Chain(sampler, N, P, K, batch=batch, seed=61) as c:
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
    groups = {n: -(-cases[n][2] // _group_width(cases[n][3], cases[n][2])) for n in NAMES if n != "dp"}
    assert [groups[n] for n in ("N2500", "G1", "G10", "G15")] == [20, 1, 10, 15], groups
    assert groups["K4"] > 4 and cases["K4"][2] > 96, (groups, cases["K4"])  # beyond two rounds of two pairs; four words
    gw = _group_width(cases["word"][3], cases["word"][2])
    assert any(g * gw < 32 < (g + 1) * gw for g in range(groups["word"])), gw  # a field lies across bit 32
    chunks = {n: -(-cases[n][1] // 64) for n in ("N700", "N1025", "N2500")}
    assert chunks == {"N700": 11, "N1025": 17, "N2500": 40}, chunks  # sixteen waves: 0 or 1, 1 or 2, 2 or 3 chunks each


@pytest.mark.parametrize("name", NAMES)
def test_plain_trip_chain_matches_the_oracle(wanted, cases, dbg_lib, name):
    _set(dbg_lib)
    assert _body(cases[name]) == (True, True), cases[name]
    _same(_run(cases[name]), wanted(name), cases[name])


def test_present_body_on_request_equals_both(wanted, cases, dbg_lib):
    _set(dbg_lib, PK_NOPIPE=1)
    assert _body(cases["N2500"]) == (True, False)
    present = _run(cases["N2500"])
    _set(dbg_lib)
    assert _body(cases["N2500"]) == (True, True)
    _same(present, _run(cases["N2500"]), "present body against the second one")
    _same(present, wanted("N2500"), "present body against the oracle")


@pytest.mark.parametrize("name", ["N2500", "G1"])
def test_counts_after_a_first_sweep_from_a_random_allocation(cases, dbg_lib, name):
    _set(dbg_lib)
    sampler, N, P, K, batch = cases[name]
    X, z0 = _data(cases[name])
    with bm.Chain(sampler, N, P, K, batch=batch, seed=61) as c:
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


def _edge_rows(KT):
    """(scores, uniforms, rows whose count is known by hand -> that count)"""
    ninf = -np.inf
    sc, u, known = [], [], {}

    def row(s, uu, count=None):
        if count is not None:
            known[len(sc)] = count
        sc.append(s)
        u.append(uu)

    # every leading running sum exactly 0 (weight exp2(-inf) = 0, or underflowed), u = 0: t = +0 = c[k], diff = +0 counts
    for lead in range(1, KT):
        s = np.full(KT, ninf)
        s[lead:] = -0.5 * np.arange(KT - lead)
        row(s, 0.0, lead)
        s = np.full(KT, -2900.0)  # 2^(-2900 log2 e) is 0 in binary32, denormals or not
        s[lead:] = 0.0
        row(s, 0.0, lead)
    one = np.full(KT, ninf)
    one[KT - 1] = -3.0
    row(one, 0.0, KT - 1)
    row(one, 1.0 - 2.0 ** -52, KT)  # (float)u is 1: t = run = c[KT - 1], and every sum ahead of it is 0
    # t equal to a running sum: equal scores, weights 1, c[k] = k + 1 exactly, u a multiple of 1/4 (KT is one of 4)
    for q in (1, 2, 3):
        row(np.zeros(KT), q / 4.0, q * KT // 4)
        row(np.full(KT, -17.25), q / 4.0, q * KT // 4)
    # ... with impossible categories between them: the sums repeat, t equals several of them
    s = np.zeros(KT)
    s[1::2] = ninf  # c = 1, 1, 2, 2, ..., KT/2, KT/2
    row(s, 0.5, KT // 2)
    row(s, 1.0 - 2.0 ** -52, KT)  # (float)u is 1: t = run
    return (np.ascontiguousarray(np.array(sc, dtype=np.float32)), np.ascontiguousarray(np.array(u, dtype=np.float64)),
            known)


@pytest.mark.parametrize("KT", [4, 20])
def test_the_draws_count_at_zero_sums_and_at_ties(dbg_lib, KT):
    sc, u, known = _edge_rows(KT)
    n = sc.shape[0]
    f = _capi.lib().bmm_dbg_pk_draw
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                  ctypes.c_int64, ctypes.c_void_p]
    for G in (1, 20):
        kernel, spec = np.full((n, 2), -7, dtype=np.int32), np.full((n, 2), -7, dtype=np.int32)
        _capi.check(f(0, KT, 0, sc.ctypes.data, u.ctypes.data, G, n, kernel.ctypes.data))
        _capi.check(f(0, KT, 1, sc.ctypes.data, u.ctypes.data, G, n, spec.ctypes.data))
        assert np.array_equal(kernel, spec), (KT, G, np.flatnonzero((kernel != spec).any(axis=1))[:8])
        for i, cnt in known.items():
            assert spec[i, 0] == cnt, (KT, G, i, sc[i], u[i], spec[i], cnt)
        assert not spec[:, 1].any(), (KT, G)  # a tie is never certain
