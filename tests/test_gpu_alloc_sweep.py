"""The allocation sampler's sweep on the device (k_count_tables<TAB_ALLOC> and the resample kernels that draw from its image;
include/bmm_mcmc.h "allocation sampler": sweep) against the oracle chain oracle.alloc, bit for
bit: equal labels after every sweep, at the shapes of tests/alloc_sweep_cases.py, on every kernel form an armed chain
can take, with K changed between the sweeps by set_k and by the moves.  Everything compared is an integer or a ratio
of equal integers, so every comparison is exact.  tests/test_oracle_alloc.py ties the oracle chain to NumPy and to the
enumerated posterior, and shows on the CPU that every case reaches what it is for."""
import functools
import os
import sys

import numpy as np
import pytest

import bmm_mcmc_amd as bm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_cases  # noqa: E402
import alloc_sweep_cases as cases  # noqa: E402
from test_gpu_chunks import _selectable, _set_env, kernel_key, launch, threads_for  # noqa: E402

pytestmark = pytest.mark.gpu
BETA, GAMMA = alloc_cases.BETA, alloc_cases.GAMMA


def _recount(X, z1, K):
    z = np.asarray(z1) - 1
    Nk = np.bincount(z, minlength=K).astype(np.int32)
    S = np.zeros((K, X.shape[1]), dtype=np.int32)
    np.add.at(S, z, X)
    return Nk, S


def _same_theta(got, want, what):
    """theta-hat as bit patterns, the NaNs (empty labels) in the same places"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]), what


# ---------------------------------------------------------------- 1. content: the run route
@functools.lru_cache(maxsize=None)
def _content_want(burnin):
    """the oracle's traces, computed once and shared"""
    from oracle import oracle
    oracle.build()
    out = {}
    for c in cases.CONTENT:
        X, z0 = cases.content_start(c.name)
        out[c.name] = oracle.alloc(X, z0, c.sweeps + 1, c.maxK, c.K_open, c.a, c.beta, c.gamma, burnin, c.seed, batch=c.batch)
    return out


def _content_run(c, burnin):
    X, z0 = cases.content_start(c.name)
    return bm.gibbs_allocation(X, c.sweeps + 1, c.maxK, a=c.a, prior_k="uniform", K0=c.K_open, moves=0, beta=c.beta,
                               gamma=c.gamma, burnin=burnin, batch=c.batch, seed=c.seed, initial_K=z0)


@pytest.mark.parametrize("burnin", [0, 3])
@pytest.mark.parametrize("name", [c.name for c in cases.CONTENT])
def test_content_cases_draw_the_oracle_chain(name, burnin):
    c = cases.CONTENT_BY_NAME[name]
    want = _content_want(burnin)[name]
    got = _content_run(c, burnin)
    for s in range(want["z"].shape[0]):   # the first sweep that differs, and by how much
        assert np.array_equal(got["z"][s], want["z"][s]), (name, "kept sweep", s, int((got["z"][s] != want["z"][s]).sum()))
    _same_theta(got["theta"], want["theta"], name)
    assert (got["K"] == c.K_open).all(), name
    assert np.array_equal(got["k_used"], [len(np.unique(r)) for r in want["z"]]), name
    assert got["moves"] == {k: 0 for k in got["moves"]}, name


# ---------------------------------------------------------------- 2. forms: a resident chain on every kernel family
@functools.lru_cache(maxsize=None)
def _form_want(name):
    from oracle import oracle
    oracle.build()
    c = cases.FORM_BY_NAME[name]
    X, z0 = cases.form_start(name)
    return oracle.alloc(X, z0, cases.FORM_SWEEPS + 1, c.maxK, c.K_open, c.a, BETA, GAMMA, 0, c.seed, batch=c.batch)


def _family_of(key):
    kt, nt, lanes, _, bits, _, own, _, generic, _ = key
    if generic:
        return "generic"
    if own:
        return "self"
    if lanes == 2:
        return "two-lane"
    if nt == 256:
        return "256"
    return "default" if nt == threads_for(kt, bits == 1) else f"step-down-{nt}"


def _armed(c, X, z0):
    ch = bm.Chain("collapsed", c.N, c.P, c.maxK, alpha=c.a, beta=BETA, gamma=GAMMA, batch=c.batch, seed=c.seed)
    try:
        ch.set_data(X)
        ch.set_initial_labels(z0)
        ch.set_alloc("uniform", 0)
        ch.set_k(c.K_open)
    except BaseException:
        ch.close()
        raise
    return ch


def _check_key(c, ch):
    """the kernel the armed chain runs, and the geometry of its launches"""
    key, shape = kernel_key(ch), ch.kernel_shape()
    assert ch.k() == c.K_open and not shape["builds_own_tables"] and key[6] == 0, (c.name, key)
    assert _family_of(key) == c.family and key[0] == cases.kt_of(c.maxK) and key[4] == 1, (c.name, key)
    if c.family == "generic":
        assert shape["lds_bytes"] == 0 and shape["threads"] == 256, (c.name, shape)
        return key, (256, shape["grid_max"], 0)
    assert (key[3], key[5]) == (c.tier, c.W), (c.name, key)
    nt, gmax, lanes = shape["threads"], shape["grid_max"], shape["lanes_per_observation"]
    full = launch(min(ch.batch, c.N), nt, gmax, lanes)
    if c.loops:
        assert full["chunks_per_wave"] >= 2, (c.name, full["chunks_per_wave"], shape)
    else:
        assert full["chunks_per_wave"] <= 1, (c.name, full["chunks_per_wave"], shape)   # one round by their rules
    assert full["grid"] >= 2, (c.name, full)
    return key, (nt, gmax, lanes)


def _open(dbg_lib, c, X, z0):
    """The armed chain of a form case under the case's switches.  A looping case sees one CU, which takes one or two of
    its workgroups depending on the kernel's registers and tables; where it takes one, a launch has a single workgroup
    and no second range for a birth to fall into, so the chain is set up again on two CUs: the same kernel (4500 rows
    are five tiles, more than either CU count, and past the short-launch limit of both), two workgroups, still more than
    two chunks per wave."""
    _set_env(dbg_lib, c.env)
    ch = _armed(c, X, z0)
    shape = ch.kernel_shape()
    if c.loops and launch(min(ch.batch, c.N), shape["threads"], shape["grid_max"], shape["lanes_per_observation"])["grid"] < 2:
        key = kernel_key(ch)
        ch.close()
        _set_env(dbg_lib, dict(c.env, CUS=2))
        ch = _armed(c, X, z0)
        assert kernel_key(ch)[:9] == key[:9], (c.name, key, kernel_key(ch))
    return ch


def _form_sweeps(c, ch, want):
    for j in range(1, cases.FORM_SWEEPS + 1):
        # sweep by sweep, stopping at the first that differs (what a wrong draw leaves behind is not read again)
        ch.sweeps(1)
        z = ch.labels()
        assert np.array_equal(z, want["z"][j]), (c.name, j, int((z != want["z"][j]).sum()))
    return z


@pytest.mark.parametrize("name", [c.name for c in cases.FORMS])
def test_every_kernel_form_of_an_armed_chain_draws_the_oracle_chain(dbg_lib, name):
    c = cases.FORM_BY_NAME[name]
    X, z0 = cases.form_start(name)
    want = _form_want(name)
    with _open(dbg_lib, c, X, z0) as ch:
        _, geometry = _check_key(c, ch)
        # what the case is for, now with the launches' real geometry: births in two workgroups' ranges of a launch
        print(name, cases.check_reached(c, want["z"], geometry))
        z = _form_sweeps(c, ch, want)
        Nk, S = ch.counts()
        Nk_ref, S_ref = _recount(X, z, c.maxK)
        np.testing.assert_array_equal(Nk, Nk_ref)
        np.testing.assert_array_equal(S, S_ref)
        assert ch.k() == c.K_open and z.max() <= c.K_open


# {family: {(own-cluster tier, group width): accumulator counts}} of the k_resample instantiations the form cases reach:
# a subset of what tests/test_gpu_chunks.py writes out as selectable (an armed chain is a finite collapsed chain on bit
# planes: tier 1 or 2, never the table-building workgroups, the emitting twins or the int32 layout)
REACHED = {
    "default": {(1, 5): (4, 28, 64), (1, 4): (16, 32, 56), (2, 4): (28, 40, 64)},
    "two-lane": {(1, 5): (16, 20, 40, 64), (1, 4): (48, 56)},
    "step-down-768": {(1, 5): (4, 12, 20)},
    "step-down-512": {(1, 5): (4, 20, 32)},
    "256": {(1, 5): (4, 12, 28, 56)},
}
GENERIC_REACHED = (4, 20, 64)


def test_the_form_cases_reach_the_kernels_written_out(dbg_lib):
    got, generic = {}, set()
    for c in cases.FORMS:
        _set_env(dbg_lib, c.env)
        with _armed(c, *cases.form_start(c.name)) as ch:
            k = kernel_key(ch)
        if k[8]:
            generic.add(k[0])
            continue
        got.setdefault(_family_of(k), set()).add(("resample", k[0], k[1], k[2], k[3], k[4], k[5], k[6]))
    want = {}
    for fam, tiers in REACHED.items():
        for (tier, W), kts in tiers.items():
            for kt in kts:
                nt = {"default": threads_for(kt, True), "two-lane": 1024, "256": 256}.get(fam) or int(fam[-3:])
                want.setdefault(fam, set()).add(("resample", kt, nt, 2 if fam == "two-lane" else 1, tier, 1, W, 0))
    assert got == want, {f: (sorted(want.get(f, set()) - got.get(f, set())), sorted(got.get(f, set()) - want.get(f, set())))
                         for f in set(got) | set(want)}
    assert generic == set(GENERIC_REACHED)
    selectable = _selectable()
    for fam, keys in want.items():
        assert keys <= selectable[fam], (fam, sorted(keys - selectable[fam]))


# ---------------------------------------------------------------- 3. K changing under the sweeps
def test_set_k_between_the_sweeps_and_the_first_batch_after_it(oracle):
    """alloc_prepare builds the tables of sweep 0 under K = maxK before set_k writes the new K: the first batch of the
    next sweep must rebuild them, here and after every later set_k, down and up"""
    X, z0 = cases.k_start()
    Ks, zs = [], [z0]
    with bm.Chain("collapsed", cases.K_N, cases.K_P, cases.K_MAXK, alpha=cases.K_A, beta=BETA, gamma=GAMMA, batch=cases.K_BATCH,
                  seed=cases.K_SEED) as ch:
        ch.set_data(X)
        ch.set_initial_labels(z0)
        ch.set_alloc("uniform", 0)
        assert ch.k() == cases.K_MAXK
        for step in range(cases.K_SWEEPS):
            z = ch.labels()
            ch.set_k(cases.k_schedule(step, z, ch.k()))
            K = ch.k()
            want = oracle.alloc(X, z, 2, cases.K_MAXK, K, cases.K_A, BETA, GAMMA, 0, cases.K_SEED, batch=cases.K_BATCH,
                                first_sweep=ch.sweep_index + 1)["z"][1]
            ch.sweeps(1)
            got = ch.labels()
            assert np.array_equal(got, want), (step, K, int((got != want).sum()))
            Ks.append(K)
            zs.append(got)
        Nk, S = ch.counts()
        Nk_ref, S_ref = _recount(X, got, cases.K_MAXK)
        np.testing.assert_array_equal(Nk, Nk_ref)
        np.testing.assert_array_equal(S, S_ref)
    print(Ks, cases.k_reached(Ks, zs))


# ---------------------------------------------------------------- 4. moves between the sweeps
@pytest.mark.parametrize("name", sorted(cases.MOVE_CASES))
def test_a_move_ahead_of_every_sweep(oracle, name):
    """40 rounds of one eject / absorb move, stepped by hand, then one sweep: the sweep from the labels and the K the move
    left, against the oracle -- an absorb's relabelled Nk and S, and the K it wrote, feed the next table build.  (The
    move's own numbers are held by tests/test_gpu_alloc.py's replay.)"""
    case, batch = alloc_cases.BY_NAME[name], cases.MOVE_CASES[name]
    X, z1, lp = alloc_cases.start(case)
    seen = []
    with bm.Chain("collapsed", case.N, case.P, case.maxK, alpha=case.a, beta=BETA, gamma=GAMMA, batch=batch, seed=case.seed) as ch:
        ch.set_data(X)
        ch.set_initial_labels(z1)
        ch.set_alloc(np.exp(lp), 0, case.e)
        ch.set_k(case.K0)
        for r in range(cases.MOVE_ROUNDS):
            d = ch.alloc_step()
            assert (d["sweep"], d["move"]) == (ch.sweep_index + 1, 0) and ch.sweep_index == r
            z, K = ch.labels(), ch.k()
            assert K == d["k_after"] and z.max() <= K
            want = oracle.alloc(X, z, 2, case.maxK, K, case.a, BETA, GAMMA, 0, case.seed, batch=batch, first_sweep=r + 1)["z"][1]
            ch.sweeps(1)
            got = ch.labels()
            assert np.array_equal(got, want), (name, r, d["kind"], d["accepted"], K, int((got != want).sum()))
            assert ch.k() == K
            Nk, S = ch.counts()
            Nk_ref, S_ref = _recount(X, got, case.maxK)
            np.testing.assert_array_equal(Nk, Nk_ref)
            np.testing.assert_array_equal(S, S_ref)
            seen.append((d["kind"], d["accepted"], d["labels"][1] - 1, d["k_before"]))
    if name in cases.MOVE_REACH:
        cases.moves_reached(seen)


# ---------------------------------------------------------------- 5. same seed, same bytes
def test_same_seed_same_bytes_on_the_run_route():
    c = cases.CONTENT_BY_NAME["P128-width-4-tier-2"]
    a, b = _content_run(c, 0), _content_run(c, 0)
    assert a["z"].tobytes() == b["z"].tobytes() and a["theta"].tobytes() == b["theta"].tobytes()
    assert a["K"].tobytes() == b["K"].tobytes()


def test_same_seed_same_bytes_on_a_resident_chain(dbg_lib):
    c = cases.FORM_BY_NAME["two-lane-t1w5-K37of35-P50"]
    X, z0 = cases.form_start(c.name)
    runs = []
    for _ in range(2):
        with _open(dbg_lib, c, X, z0) as ch:
            _check_key(c, ch)
            ch.sweeps(cases.FORM_SWEEPS)
            runs.append((ch.labels(), ch.counts()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes()
    assert runs[0][1][0].tobytes() == runs[1][1][0].tobytes() and runs[0][1][1].tobytes() == runs[1][1][1].tobytes()
