"""Every form of the resample kernel that loops -- a wave taking a second chunk and more from its workgroup's LDS
counter, with the next chunk's X words, previous labels and position prefetched while this one is scored --
against the oracle, bit for bit.

Test-sized batches fill one round of the real chip, so the tests below make the kernel choice see fewer compute
units (BMM_DEBUG_CUS, test variant): a batch of a few thousand observations then runs the default-sized kernels
of plan_kernel's own rules with several chunks per wave.  Every case states which kernel it gets and how many
chunks per wave that gives (kernel_shape), so that a later change to plan_kernel cannot quietly turn a looping case
back into a one-round one, and test_the_cases_reach_every_selectable_kernel holds the set of k_resample
instantiations the cases reach against the kernel set of chain.hip (instantiated).  The last tests run the benchmark
shapes on the product library at the real CU count."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi
from util import assert_matrix_equal, synth

pytestmark = pytest.mark.gpu

KKT = (4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 52, 56, 64)   # chain.hip kKT


def threads_for(kt, bits):
    """chain.hip threads_for: the default workgroup size of the one-lane kernels"""
    if bits:
        return 1024 if kt <= 20 else (768 if kt <= 32 else 512)
    return 1024 if kt <= 12 else (768 if kt <= 20 else 512)


def kt_of(sampler, K):
    cats = K + 1 if sampler == "dp" else K
    return next(kt for kt in KKT if kt >= cats)


# One shape (sampler, K, P) per accumulator count for each (own-cluster tier, group width) the rules can give at
# P <= 128: tier 1 = own-cluster tables in LDS (collapsed / DP), 2 = in global memory, 0 = none (stick-breaking /
# full).  The group width is 4 only where the 32-entry tables would not fit (bmm_spec_group_width_for); tier 2 only
# occurs at width 4 (the width rule asks for the whole image to fit at 5), and at neither width for fewer than 24
# accumulators.  The two samplers of a tier alternate.
SHAPES = {
    (1, 5): [("collapsed", 3, 100), ("dp", 7, 65), ("collapsed", 11, 128), ("dp", 15, 96), ("collapsed", 20, 100),
             ("dp", 22, 85), ("collapsed", 27, 70), ("dp", 30, 50), ("collapsed", 37, 50), ("dp", 44, 33),
             ("collapsed", 50, 36), ("dp", 53, 31), ("collapsed", 64, 30)],
    (1, 4): [("collapsed", 14, 127), ("dp", 18, 110), ("collapsed", 23, 100), ("dp", 26, 90), ("collapsed", 30, 70),
             ("dp", 36, 60), ("collapsed", 45, 45), ("dp", 50, 45), ("collapsed", 55, 40), ("dp", 60, 33)],
    (2, 4): [("dp", 21, 120), ("collapsed", 28, 100), ("dp", 30, 100), ("collapsed", 40, 80), ("dp", 46, 70),
             ("collapsed", 52, 60), ("dp", 54, 60), ("collapsed", 60, 50)],
    (0, 5): [("full", 4, 33), ("stickbreaking", 6, 128), ("full", 10, 64), ("stickbreaking", 16, 100), ("full", 18, 97),
             ("stickbreaking", 24, 100), ("full", 25, 90), ("stickbreaking", 32, 63), ("full", 35, 64),
             ("stickbreaking", 48, 40), ("stickbreaking", 50, 50), ("full", 56, 40), ("stickbreaking", 64, 20)],
    (0, 4): [("full", 22, 125), ("stickbreaking", 28, 110), ("full", 30, 100), ("stickbreaking", 40, 90),
             ("full", 47, 70), ("stickbreaking", 51, 60), ("full", 54, 60), ("stickbreaking", 63, 50)],
}

# env: the test variant's switches (CUS = BMM_DEBUG_CUS); loops: the case claims at least two chunks per wave on
# its full-size launches; probs: the case's second sweep hands its probabilities over (the EMIT twin)
Case = namedtuple("Case", "id sampler N P K batch layout env loops probs tier W")

SWEEPS = 4


def _cases():
    out = []
    for (tier, W), shapes in SHAPES.items():
        for sampler, K, P in shapes:
            kt = kt_of(sampler, K)
            explicit = tier == 0
            N, batch = 10_000, (10_000 if explicit else 4_500)   # collapsed / DP: two full batches and a short one
            for layout in ("bits", "int32"):
                # the default-sized one-lane kernel on one CU: 4500 observations are 71 chunks for at most
                # 2 workgroups of 16 waves (8 of 8 above 32 accumulators)
                env = {"CUS": 1, "NOSPLIT": kt > 32 and layout == "bits"}
                out.append(Case(f"one-lane-{layout}-t{tier}w{W}-{sampler}-K{K}-P{P}", sampler, N, P, K, batch, layout,
                                env, True, layout == "bits", tier, W))
            if tier != 2 and (kt > 32 or (W == 5 and kt >= 16)):
                # the two-lane form (always above 32 accumulators; 16-32 on short launches, BMM_DEBUG_SPLIT here)
                out.append(Case(f"two-lane-t{tier}w{W}-{sampler}-K{K}-P{P}", sampler, N, P, K, batch, "bits",
                                {"CUS": 1, "SPLIT": kt <= 32}, True, False, tier, W))
            if tier != 2 and W == 5 and kt <= 32:
                # the stepped-down workgroups: a batch that cannot give every CU a default-sized one, but fits one
                # round of the smaller ones (3000 observations: 4 CUs -> 768 threads, 6 CUs -> 512)
                for cus in ((4, 6) if kt <= 20 else (6,)):
                    out.append(Case(f"step-down-{cus}cus-t{tier}-{sampler}-K{K}-P{P}", sampler, 3000, P, K, 3000, "bits",
                                    {"CUS": cus, "NOSPLIT": kt >= 16}, False, False, tier, W))
            if tier != 2 and W == 5 and not (tier == 1 and kt == 64):
                # the 256-thread workgroups: fewer tiles than CUs, tables small enough for four per CU (P = 2)
                for layout in ("bits", "int32"):
                    out.append(Case(f"small-{layout}-t{tier}-{sampler}-K{K}", sampler, 3000, 2, K, 3000, layout,
                                    {"CUS": 64, "NOSPLIT": True, "NOSELF": True}, False, False, tier, W))
    for K, P in ((3, 20), (7, 14), (11, 9)):   # the table-building 256-thread kernels (finite sampler, K(4P+5) <= 512)
        out.append(Case(f"self-K{K}-P{P}", "collapsed", 3000, P, K, 1000, "bits", {"CUS": 64}, False, False, 1, 5))
    # ragged edges: batches that are not a multiple of 64 and a short last batch (5000 = 2 x 2300 + 400), on 1 and 2 CUs
    out.append(Case("ragged-1cu-collapsed-K20-P50", "collapsed", 5000, 50, 20, 2300, "bits", {"CUS": 1}, True, True, 1, 5))
    out.append(Case("ragged-2cus-dp-K30-P60", "dp", 9000, 60, 30, 4001, "bits", {"CUS": 2}, False, True, 1, 5))
    out.append(Case("ragged-int32-collapsed-K12-P97", "collapsed", 7777, 97, 12, 3333, "int32", {"CUS": 1}, True, False, 1, 5))
    return out


CASES = _cases()
ENV = {"CUS": "BMM_DEBUG_CUS", "NOSPLIT": "BMM_DEBUG_NOSPLIT", "SPLIT": "BMM_DEBUG_SPLIT", "NOSELF": "BMM_DEBUG_NOSELF"}


def _set_env(mp, env, layout=None):
    for k, name in ENV.items():
        v = env.get(k)
        if v is None or v is False:
            mp.delenv(name, raising=False)
        else:
            mp.setenv(name, str(int(v)))
    if layout == "int32":
        mp.setenv("BMM_X_LAYOUT_INT32", "1")
    else:
        mp.delenv("BMM_X_LAYOUT_INT32", raising=False)


def kernel_key(ch):
    """(accumulators, threads, lanes, own-cluster tier, bit planes, group width, builds own tables, emitting twin's
    threads, generic, emitting twin's grid limit) of the chain's kernel: bmm_dbg_kernel_key, test variant"""
    k = (ctypes.c_int * 10)()
    _capi.check(_capi.lib().bmm_dbg_kernel_key(ch._h, k))
    return tuple(k)


def kernel_plan(case, num_cus, shares_device=False):
    """the same key, slot 9 zero, as the shape arithmetic and the kernel choice give it for the case's arguments
    without a chain or a device: bmm_dbg_kernel_plan, test variant"""
    k = (ctypes.c_int * 10)()
    _capi.check(_capi.lib().bmm_dbg_kernel_plan(_capi.SAMPLER_CODE[case.sampler], ctypes.c_int64(case.N), case.P, case.K,
                                                ctypes.c_int64(case.batch), num_cus, int(shares_device),
                                                int(case.layout == "int32"), k))
    return tuple(k)


def launch(n, threads, grid_max, lanes):
    """How k_resample hands out one launch of n observations (kernels.hip.h): chunks of 64 / lanes observations,
    workgroup b owning chunks [b * cpw, (b + 1) * cpw) of them."""
    ow, nw = 64 // lanes, threads // 64
    nchunks = -(-n // ow)
    grid = min(-(-n // (threads // lanes)), grid_max)
    cpw = -(-nchunks // grid)
    per_wg = [max(0, min(cpw, nchunks - b * cpw)) for b in range(grid)]
    return {"ow": ow, "nw": nw, "nchunks": nchunks, "grid": grid, "cpw": cpw, "per_wg": per_wg,
            "chunks_per_wave": cpw / nw}


def batches(N, batch):
    return [(lo, min(N, lo + batch)) for lo in range(0, N, batch)]


def _init(case, seed):
    rng = np.random.default_rng(seed)
    if case.sampler in ("collapsed",):
        return rng.integers(1, case.K + 1, case.N).astype(np.int32)
    if case.sampler == "dp":
        return None
    pi0 = rng.dirichlet(np.ones(case.K))
    th0 = 0.05 + 0.9 * rng.random((case.K, case.P))
    return pi0, th0


def _oracle(oracle, case, X, init, S, seed, probs_sweep=None):
    """the oracle chain of a case; probs_sweep=j: with the whole probability matrix of sweep j (its "probs")"""
    if case.sampler == "collapsed":
        return oracle.collapsed(X, init, S, case.K, 0.0, 0.5, 0.5, 1, 1, 0, seed=seed, batch=case.batch,
                                probs_sweep=probs_sweep)
    if case.sampler == "dp":
        return oracle.dp(X, S, 0.0, 0.5, 0.5, 1, 1, 0, case.K, seed=seed, batch=case.batch, probs_sweep=probs_sweep)
    fn = oracle.stickbreaking if case.sampler == "stickbreaking" else oracle.full
    return fn(X, init[0], init[1], S, case.K, 0.0, 0.5, 0.5, 1, 1, 0, seed=seed, probs_sweep=probs_sweep)


def _run(case, X, init, S, seed):
    if case.sampler == "collapsed":
        return bm.gibbs_collapsed(X, S, case.K, burnin=0, seed=seed, batch=case.batch, initial_K=init)
    if case.sampler == "dp":
        return bm.gibbs_dp(X, S, burnin=0, maxK=case.K, seed=seed, batch=case.batch)
    fn = bm.gibbs_stickbreaking if case.sampler == "stickbreaking" else bm.gibbs_full
    return fn(X, S, case.K, burnin=0, seed=seed, initial_pi=init[0], initial_theta=init[1])


def _start(ch, case, init):
    if case.sampler == "collapsed":
        ch.set_initial_labels(init)
    elif case.sampler != "dp":
        ch.set_initial_params(*init)


def probe_rows(lo, hi, threads, grid_max, lanes=1):
    """Observations of one launch at its chunk and workgroup edges: first and last of every workgroup's range, the
    first of the first chunk handed out by the counter, the last of the launch"""
    g = launch(hi - lo, threads, grid_max, lanes)
    rows = {lo, hi - 1}
    for b, cn in enumerate(g["per_wg"]):
        if cn <= 0:
            continue
        c0 = b * g["cpw"]
        rows.add(lo + c0 * g["ow"])
        rows.add(min(hi, lo + (c0 + cn) * g["ow"]) - 1)
        if cn > g["nw"]:
            rows.add(lo + (c0 + g["nw"]) * g["ow"])
            rows.add(lo + (c0 + g["nw"]) * g["ow"] + g["ow"] - 1)
    return sorted(r for r in rows if lo <= r < hi)


def check_probs(oracle, case, X, probs, want_matrix, z_before, z_after, alpha_before, params_before, threads, grid_max,
                limit=24):
    """a hand-off sweep's probabilities against the oracle chain's matrix of the same sweep, every row and column bit
    for bit (the DP's too: the oracle files the new-cluster mass by the reference's rule, tests/test_oracle_probs.py);
    then rows at the chunk and workgroup edges against the oracle's per-row conditionals, each under the state its
    batch saw: the labels already redrawn by the earlier batches of the sweep, the previous sweep's for the rest"""
    np.testing.assert_allclose(probs.sum(axis=1), 1.0, rtol=0, atol=1e-13)
    assert_matrix_equal(probs, want_matrix, case.id)
    if case.sampler == "dp":
        return   # (no per-row probes: the whole matrix above covers them)
    rows = []
    for lo, hi in batches(case.N, case.batch if case.sampler == "collapsed" else case.N):
        rows += [(lo, r) for r in probe_rows(lo, hi, threads, grid_max)]
    if len(rows) > limit:
        keep = np.linspace(0, len(rows) - 1, limit).round().astype(int)
        rows = [rows[i] for i in sorted(set(keep))]
    for lo, i in rows:
        if case.sampler == "collapsed":
            state = np.concatenate([z_after[:lo], z_before[lo:]])
            _, norm = oracle.collapsed_cond(X, state, i, case.K, alpha_before, 0.5, 0.5, spec=True)
        else:
            _, norm = oracle.sb_cond(X, i, params_before[0], params_before[1], spec=True)
        assert np.array_equal(probs[i], norm), (case.id, i)


def test_hand_off_probabilities_at_52_accumulators(oracle):
    """49-52 categories on the default path (two-lane kernel, one-lane emitting twin): 52 accumulators at group width
    5, where rounding up to 56 would ask for the narrower groups -- the oracle must size the image the same way, or
    its conditionals are grouped differently and come out a few ulps off while the drawn labels still agree"""
    N, P, K = 6000, 36, 50
    X, _, _, _ = synth(N, P, 5, N + P)
    z0 = np.random.default_rng(5).integers(1, K + 1, N).astype(np.int32)
    want = oracle.collapsed(X, z0, 3, K, 0.0, 0.5, 0.5, 1, 1, 0, seed=9, batch=N, probs_sweep=2)
    with bm.Chain("collapsed", N, P, K, batch=N, seed=9) as ch:
        ch.set_data(X)
        ch.set_initial_labels(z0)
        ch.sweeps(1)
        zb, alpha = ch.labels(), ch.alpha()
        probs = ch.sweep_probs()
        assert np.array_equal(ch.labels(), want["z"][2])
    assert_matrix_equal(probs, want["probs"], "52 accumulators")
    for i in (0, 1, 63, 64, N - 1):
        _, norm = oracle.collapsed_cond(X, zb, i, K, alpha, 0.5, 0.5, spec=True)
        assert np.array_equal(probs[i], norm), i


def _geometry_checks(case, ch, key):
    shape = ch.kernel_shape()
    nt, gmax, lanes = shape["threads"], shape["grid_max"], shape["lanes_per_observation"]
    full = launch(min(ch.batch, case.N), nt, gmax, lanes)
    if case.loops:
        assert full["chunks_per_wave"] >= 2, (case.id, full["chunks_per_wave"], shape)
    if nt == 256 and not key[6]:
        # the 256-thread forms are chosen for fewer tiles than CUs at the default size: one round whenever the
        # occupancy query allows default-size / 256 of them per CU (four at 1024 threads), which is not a given for
        # the big kernels (VGPRs) -- so the round count is checked, not assumed
        assert full["chunks_per_wave"] <= 1, (case.id, shape)
    if nt in (768, 512) and lanes == 1 and nt < threads_for(key[0], key[4] == 1):
        assert full["chunks_per_wave"] <= 1, case.id   # the step-down forms: one round by their rule
    return nt, gmax, lanes


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_kernel_form_draws_the_oracle_chain(oracle, dbg_lib, case):
    _set_env(dbg_lib, case.env)
    S, seed = SWEEPS, 11 + case.K + case.P
    X, _, _, _ = synth(case.N, case.P, min(case.K, 5), case.N + case.P)
    init = _init(case, seed)
    # (sample 0 of the oracle's trace: the initial state; with the whole matrix of the hand-off sweep)
    want = _oracle(oracle, case, X, init, S + 1, seed, probs_sweep=2 if case.probs else None)
    explicit = case.sampler in ("stickbreaking", "full")
    with bm.Chain(case.sampler, case.N, case.P, case.K, batch=case.batch, seed=seed, x_layout=case.layout) as ch:
        key = kernel_key(ch)
        assert key[8] == 0 and key[3] == case.tier and key[5] == case.W and key[4] == (case.layout == "bits"), (case.id, key)
        nt, gmax, lanes = _geometry_checks(case, ch, key)
        ch.set_data(X)
        _start(ch, case, init)
        z_prev = init if case.sampler == "collapsed" else None
        for j in range(1, S + 1):
            # sweep by sweep, stopping at the first one that differs (what a wrong chunk hand-out leaves behind is
            # not read again)
            alpha_before = ch.alpha()
            params_before = (init if j == 1 else ch.params()) if explicit else None
            if case.probs and j == 2:
                probs = ch.sweep_probs()
                kp = kernel_key(ch)
                assert kp[7] == threads_for(key[0], True) and kp[9] > 0, (case.id, kp)
                if case.loops:
                    assert launch(min(ch.batch, case.N), kp[7], kp[9], 1)["chunks_per_wave"] >= 2, (case.id, kp)
            else:
                ch.sweeps(1)
            z = ch.labels()
            assert np.array_equal(z, want["z"][j]), (case.id, j, int((z != want["z"][j]).sum()))
            if case.probs and j == 2:
                check_probs(oracle, case, X, probs, want["probs"], z_prev, z, alpha_before, params_before, kp[7], kp[9])
            z_prev = z
        nk, s = ch.counts()
        assert np.array_equal(nk, np.bincount(z - 1, minlength=case.K)[:case.K]), case.id
        assert np.array_equal(s, np.stack([X[z == k + 1].sum(axis=0) for k in range(case.K)])), case.id
        assert ch.alpha() == want["alpha"][S, 0], case.id
        if explicit:
            pi, th = ch.params()
            assert np.array_equal(pi, want["pi"][S]) and np.array_equal(th, want["theta"][:, :, S]), case.id
    # the *_run entry point of the same shape: the whole trace, theta and alpha (and pi)
    _set_env(dbg_lib, case.env, case.layout)
    got = _run(case, X, init, S + 1, seed)
    for k in ("z", "theta", "alpha") + (("pi",) if explicit else ()):
        assert np.array_equal(got[k], want[k], equal_nan=True), (case.id, k)


# --------------------------------------------------------------------------- which kernels the cases reach
# Every k_resample instantiation of chain.hip (the forms `instantiated` admits) that plan_kernel (and the hand-off's
# probs_alloc) can select, written out per family: {(own-cluster tier, group width): accumulator counts}.  Tier 1 = own-cluster
# tables in LDS, 2 = in global memory, 0 = none.  Left out, because no rule selects them:
#   - tier 2 at group width 5 (default-sized kernels and emitting twins): the width rule picks 5 only when the whole table image
#     fits in LDS, own-cluster tables included, so a width-5 shape never needs the second tier;
#   - width 4 at 4-12 accumulators (any tier) and at 16-20 without own-cluster tables, and tier 2 below 24: those
#     tables fit at P <= 128 (beyond that the generic kernel runs);
#   - the two-lane forms of 16-32 accumulators at width 4 (not instantiated) and in tier 2
#     (the split form reads its own-cluster tables from LDS only);
#   - the 256-thread kernels with own-cluster tables at 64 accumulators: the tables never fit four times into LDS;
#   - the kernels of a chosen size for the int32 layout (1024 / 768 / 512 threads): only BMM_DEBUG_THREADS reaches them, no
#     rule; for bit planes at 1024 threads it is the default instantiation itself;
#   - the stepped-down forms of 16-32 accumulators are reached only where the short-launch rule, which would run
#     them two lanes per observation, is off (a chain that shares its device; BMM_DEBUG_NOSPLIT here).
KT_ALL = (4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 52, 56, 64)
KT_W4_OWN = (16, 20, 24, 28, 32, 40, 48, 52, 56, 64)
KT_W4 = (24, 28, 32, 40, 48, 52, 56, 64)
SELECTABLE = {
    # one lane, default size, for both layouts (2 x 52)
    "default": {(1, 5): KT_ALL, (0, 5): KT_ALL, (1, 4): KT_W4_OWN, (0, 4): KT_W4, (2, 4): KT_W4},
    # the emitting twins, bit planes only (52)
    "emit": {(1, 5): KT_ALL, (0, 5): KT_ALL, (1, 4): KT_W4_OWN, (0, 4): KT_W4, (2, 4): KT_W4},
    # 1024 threads, two lanes per observation (30)
    "two-lane": {(1, 5): KT_ALL[3:], (0, 5): KT_ALL[3:], (1, 4): KT_ALL[8:], (0, 4): KT_ALL[8:]},
    # 768 / 512 threads: the stepped-down workgroups, width 5 (26)
    "step-down-768": {(1, 5): KT_ALL[:5], (0, 5): KT_ALL[:5]},
    "step-down-512": {(1, 5): KT_ALL[:8], (0, 5): KT_ALL[:8]},
    # 256 threads, width 5, for both layouts (2 x 25)
    "256": {(1, 5): KT_ALL[:12], (0, 5): KT_ALL},
    # SELF: 256 threads that build their own tables (3)
    "self": {(1, 5): (4, 8, 12)},
}
SELECTABLE_COUNTS = {"default": 104, "emit": 52, "two-lane": 30, "step-down-768": 10, "step-down-512": 16, "256": 50, "self": 3}


def _table_of(key):
    """which family of SELECTABLE a (kind, accumulators, threads, lanes, tier, bits, width, own tables) key comes from"""
    kind, kt, nt, lanes, _, bits, _, own = key
    if kind == "emit":
        return "emit"
    if own:
        return "self"
    if lanes == 2:
        return "two-lane"
    if nt == 256:
        return "256"
    return "default" if nt == threads_for(kt, bits) else f"step-down-{nt}"


def _selectable():
    out = {}
    for table, tiers in SELECTABLE.items():
        keys = out.setdefault(table, set())
        for (tier, W), kts in tiers.items():
            for kt in kts:
                if table in ("default", "256"):
                    for bits in (1, 0):
                        keys.add(("resample", kt, 256 if table == "256" else threads_for(kt, bits), 1, tier, bits, W, 0))
                elif table == "emit":
                    keys.add(("emit", kt, threads_for(kt, True), 1, tier, 1, W, 0))
                elif table == "two-lane":
                    keys.add(("resample", kt, 1024, 2, tier, 1, W, 0))
                elif table == "self":
                    keys.add(("resample", kt, 256, 1, tier, 1, W, 1))
                else:
                    keys.add(("resample", kt, int(table[-3:]), 1, tier, 1, W, 0))
    return out


def test_the_cases_reach_every_selectable_kernel(dbg_lib):
    got = {}
    for case in CASES:
        _set_env(dbg_lib, case.env)
        with bm.Chain(case.sampler, case.N, case.P, case.K, batch=case.batch, seed=1, x_layout=case.layout) as ch:
            k = kernel_key(ch)
            assert k[8] == 0, case.id
            # the plan and what the chain set up cannot drift apart (every case names its CU count, so the real
            # device's does not enter)
            assert kernel_plan(case, 256)[:9] == k[:9], (case.id, kernel_plan(case, 256), k)
            key = ("resample", k[0], k[1], k[2], k[3], k[4], k[5], k[6])
            got.setdefault(_table_of(key), set()).add(key)
            if case.probs:
                # the emitting twin as the hand-off sets it up (the data are irrelevant to the choice)
                ch.set_data(np.zeros((case.N, case.P), dtype=np.int32))
                _start(ch, case, _init(case, 1))
                ch.sweep_probs()
                e = kernel_key(ch)
                assert e[9] > 0, case.id
                got.setdefault("emit", set()).add(("emit", e[0], e[7], 1, e[3], e[4], e[5], 0))
    want = _selectable()
    assert {t: len(v) for t, v in want.items()} == SELECTABLE_COUNTS
    for table in SELECTABLE:
        assert got.get(table, set()) == want[table], (table, sorted(want[table] - got.get(table, set())),
                                                      sorted(got.get(table, set()) - want[table]))
    assert set(got) == set(SELECTABLE), sorted(got)


def test_every_family_the_dp_can_select_hands_a_matrix_over():
    """The DP has own-cluster tables, so it selects tier 1 at both group widths and tier 2 (at width 4): each of those
    families must keep a DP case whose hand-off matrix is compared (check_probs), or a wrong weight of a DP
    category that was not drawn goes unseen in that family's emitting twins."""
    families = {(c.tier, c.W) for c in CASES if c.sampler == "dp" and c.probs}
    assert families == {(1, 5), (1, 4), (2, 4)}, sorted(families)
    for fam in families:      # and at more than one accumulator count each
        assert len({kt_of("dp", c.K) for c in CASES if c.sampler == "dp" and c.probs and (c.tier, c.W) == fam}) >= 4, fam


def test_a_launch_with_workgroups_that_get_no_chunk(oracle, dbg_lib):
    """cpw = ceil(chunks / grid) can leave the last workgroups of a launch nothing (wg_cn <= 0): they stage the
    tables and flush an empty histogram.  The batch is chosen from the grid limit the kernel choice reports, so
    that the last workgroup is empty while the others loop."""
    N0, P, K = 100_000, 20, 8
    _set_env(dbg_lib, {"CUS": 40})
    with bm.Chain("collapsed", N0, P, K, batch=N0, seed=1) as ch:
        shape = ch.kernel_shape()
    nt, g = shape["threads"], shape["grid_max"]
    nw = nt // 64
    q = next(q for q in range(2 * nw, g) if q * (g - 1) > g * nw)
    batch = q * (g - 1) * 64 - 23                  # q (g - 1) chunks, the last one ragged
    N = batch + 5000
    geo = launch(batch, nt, g, 1)
    assert geo["grid"] == g and geo["per_wg"][-1] == 0 and geo["chunks_per_wave"] >= 2, geo
    X, _, _, _ = synth(N, P, 4, 77)
    z0 = np.random.default_rng(3).integers(1, K + 1, N).astype(np.int32)
    want = oracle.collapsed(X, z0, 4, K, 0.0, 0.5, 0.5, 1, 1, 0, seed=8, batch=batch)
    with bm.Chain("collapsed", N, P, K, batch=batch, seed=8) as ch:
        assert ch.kernel_shape() == shape
        ch.set_data(X)
        ch.set_initial_labels(z0)
        for j in range(3):
            ch.sweeps(1)
            assert np.array_equal(ch.labels(), want["z"][j + 1]), j
        assert ch.alpha() == want["alpha"][3, 0]


def test_chains_sharing_their_data_on_one_device(oracle, dbg_lib):
    """Chains that share a device run the one-lane forms (no short-launch split); several chunks per wave each."""
    N, P, K, batch = 10_000, 50, 20, 4_500
    _set_env(dbg_lib, {"CUS": 1})
    X, _, _, _ = synth(N, P, 4, 5)
    z0s = [np.random.default_rng(40 + c).integers(1, K + 1, N).astype(np.int32) for c in range(2)]
    wants = [oracle.collapsed(X, z0s[c], 5, K, 0.0, 0.5, 0.5, 1, 1, 0, seed=60 + c, batch=batch) for c in range(2)]
    chains = [bm.Chain("collapsed", N, P, K, batch=batch, seed=60 + c) for c in range(2)]
    try:
        chains[0].set_data(X)
        chains[1].share_data(chains[0])
        for ch, z0 in zip(chains, z0s):
            ch.set_initial_labels(z0)
            shape = ch.kernel_shape()
            assert shape["lanes_per_observation"] == 1 and shape["threads"] == 1024
            assert launch(batch, 1024, shape["grid_max"], 1)["chunks_per_wave"] >= 2
        bm.sweep_chains(chains, 1)
        for ch, want in zip(chains, wants):
            ch.sync()
            assert np.array_equal(ch.labels(), want["z"][1])
        bm.sweep_chains(chains, 3)
        for ch, want in zip(chains, wants):
            ch.sync()
            assert np.array_equal(ch.labels(), want["z"][4])
            assert ch.alpha() == want["alpha"][4, 0]
    finally:
        for ch in chains:
            ch.close()


# --------------------------------------------------------------------------- benchmark shapes, product library
def block_matrix(N, P, K_true, seed, block=1 << 16):
    """N x P 0/1 matrix (int32, column-major) drawn a block of rows at a time, so that host memory stays near the
    matrix itself"""
    rng = np.random.default_rng(seed)
    w = np.arange(K_true, 0, -1, dtype=np.float64)
    theta = 0.1 + 0.8 * rng.random((K_true, P))
    X = np.empty((N, P), dtype=np.int32, order="F")
    for lo in range(0, N, block):
        hi = min(N, lo + block)
        lab = rng.choice(K_true, hi - lo, p=w / w.sum())
        X[lo:hi] = (rng.random((hi - lo, P)) < theta[lab]).astype(np.uint8)
    return X


def _full_size(oracle, sampler, X, K, sweeps, seed, batch=None, layout=None, loops=None, generic=False):
    """A few sweeps of a chain on the product library against the oracle: labels after every sweep, the
    statistics, alpha (and pi, theta).  Returns the chain's kernel shape and batch."""
    N, P = X.shape
    case = Case("full-size", sampler, N, P, K, batch or 0, layout, {}, False, False, None, None)
    init = _init(case, seed)
    with bm.Chain(sampler, N, P, K, batch=batch, seed=seed, x_layout=layout) as ch:
        case = case._replace(batch=ch.batch)
        shape = ch.kernel_shape()
        if generic:
            assert shape["lds_bytes"] == 0 and shape["threads"] == 256
            assert N > shape["grid_max"] * 256          # the grid-stride loop of the generic kernel
        if loops is not None:
            geo = launch(ch.batch, shape["threads"], shape["grid_max"], shape["lanes_per_observation"])
            assert (geo["chunks_per_wave"] >= 2) == loops, (geo["chunks_per_wave"], shape)
        want = _oracle(oracle, case, X, init, sweeps + 1, seed)
        ch.set_data(X)
        _start(ch, case, init)
        for j in range(sweeps):
            ch.sweeps(1)
            z = ch.labels()
            assert np.array_equal(z, want["z"][j + 1]), (j, int((z != want["z"][j + 1]).sum()))
        nk, _ = ch.counts()
        assert np.array_equal(nk, np.bincount(z - 1, minlength=K)[:K])
        assert ch.alpha() == want["alpha"][sweeps, 0]
        if sampler in ("stickbreaking", "full"):
            pi, th = ch.params()
            assert np.array_equal(pi, want["pi"][sweeps]) and np.array_equal(th, want["theta"][:, :, sweeps])
        return shape, ch.batch


@pytest.mark.timeout(900)
def test_benchmark_shape_c5_kernel_loops_in_both_layouts(oracle):
    """K=20, P=100, N=2^20 in one launch: 1024-thread workgroups on every CU, four chunks per wave"""
    X = block_matrix(1 << 20, 100, 5, 1)
    shape, _ = _full_size(oracle, "collapsed", X, 20, 2, 5, batch=1 << 20, layout="bits", loops=True)
    assert (shape["threads"], shape["lanes_per_observation"]) == (1024, 1)
    _full_size(oracle, "collapsed", X, 20, 2, 5, batch=1 << 20, layout="int32")


@pytest.mark.timeout(900)
def test_benchmark_shape_north_star_default_batch_and_one_launch(oracle):
    X = block_matrix(1_000_000, 50, 5, 2)
    shape, batch = _full_size(oracle, "collapsed", X, 20, 2, 7, loops=False)
    assert batch == 250_000 and shape["threads"] == 1024      # the 245 x 1024 launch bench.py times
    _full_size(oracle, "collapsed", X, 20, 2, 7, batch=1_000_000, loops=True)


@pytest.mark.timeout(900)
def test_benchmark_shape_c3_dp(oracle):
    X = block_matrix(1_000_000, 50, 6, 3)
    shape, _ = _full_size(oracle, "dp", X, 30, 2, 9)
    assert shape["threads"] == 768


@pytest.mark.timeout(900)
def test_benchmark_shape_c4_stickbreaking_two_lanes(oracle):
    X = block_matrix(1_000_000, 50, 6, 4)
    shape, _ = _full_size(oracle, "stickbreaking", X, 50, 2, 3, loops=True)
    assert shape["lanes_per_observation"] == 2


@pytest.mark.timeout(900)
def test_benchmark_shape_c2_self_built_tables(oracle):
    X = block_matrix(100_000, 20, 3, 5)
    shape, _ = _full_size(oracle, "collapsed", X, 3, 3, 4)
    assert shape["builds_own_tables"]


@pytest.mark.timeout(900)
def test_benchmark_shape_generic_kernel_past_its_grid(oracle):
    X = block_matrix(300_000, 200, 4, 6)
    _full_size(oracle, "collapsed", X, 5, 2, 6, batch=300_000, generic=True)


@pytest.mark.timeout(900)
def test_benchmark_shape_north_star_hand_off_in_one_launch(oracle):
    """sweep_probs() at the north-star shape, batch N: the whole matrix against the oracle chain's, then rows at chunk
    and workgroup edges against the per-row conditionals"""
    N, P, K = 1_000_000, 50, 20
    X = block_matrix(N, P, 5, 2)
    z0 = np.random.default_rng(12).integers(1, K + 1, N).astype(np.int32)
    want = oracle.collapsed(X, z0, 3, K, 0.0, 0.5, 0.5, 1, 1, 0, seed=13, batch=N, probs_sweep=2)
    with bm.Chain("collapsed", N, P, K, batch=N, seed=13) as ch:
        shape = ch.kernel_shape()
        ch.set_data(X)
        ch.set_initial_labels(z0)
        ch.sweeps(1)
        zb, alpha = ch.labels(), ch.alpha()
        assert np.array_equal(zb, want["z"][1])
        probs = ch.sweep_probs()
        assert np.array_equal(ch.labels(), want["z"][2])
    np.testing.assert_allclose(probs.sum(axis=1), 1.0, rtol=0, atol=1e-13)
    assert_matrix_equal(probs, want["probs"], "north-star hand-off")
    # the emitting twin has the plain kernel's workgroup size and tables, hence its grid limit
    rows = probe_rows(0, N, 1024, shape["grid_max"])
    rows = [rows[i] for i in sorted(set(np.linspace(0, len(rows) - 1, 16).round().astype(int)))]
    for i in rows:
        _, norm = oracle.collapsed_cond(X, zb, i, K, alpha, 0.5, 0.5, spec=True)
        assert np.array_equal(probs[i], norm), i
