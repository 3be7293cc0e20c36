"""The oracle's third mode of the counts chain -- the allocation sampler's sweep with open empty labels (oracle.alloc,
oracle.alloc_cond; include/bmm_mcmc.h "allocation sampler": sweep) -- tied to what is independent of it: the float64
NumPy restatement of the conditional (tests/alloc_ref.py), the collapsed chain where the two must agree, and the exact
posterior by enumeration.  tests/test_gpu_alloc_sweep.py holds the device to this chain bit for bit; here the oracle
alone also shows that every case of tests/alloc_sweep_cases.py reaches what it is for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_cases  # noqa: E402
import alloc_ref as ref  # noqa: E402
import alloc_sweep_cases as cases  # noqa: E402
import split_merge_checks as smchk  # noqa: E402
from test_split_merge_ref import seven_observations  # noqa: E402

# ---------------------------------------------------------------- 1. the conditional against the restatement
# 12 rows on maxK = 5 labels (0-based here).  Each state is scored at every row.
STATES = {
    # label 2 holds row 10 alone (its own row is scored with the label at prior weight), label 3 is open and empty,
    # label 4 is closed
    "singleton-empty-closed": (4, [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 0]),
    # everything open: a singleton on the last label, label 1 empty
    "all-open": (5, [0, 0, 0, 0, 2, 2, 2, 3, 3, 3, 3, 4]),
    # one open label: four closed
    "one-open": (1, [0] * 12),
    # two rows, each alone, and two empty labels between occupied ones
    "two-singletons": (5, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 4]),
}
MAXK = 5


def _small_data(P, seed=8):
    rng = np.random.default_rng(seed)
    theta = np.where(rng.random((2, P)) < 0.5, 0.2, 0.8)
    X = (rng.random((12, P)) < theta[rng.integers(2, size=12)]).astype(np.int32)
    X[10] = rng.random(P) < 0.5
    return np.asfortranarray(X)


@pytest.mark.parametrize("P", [1, 5, 6, 33, 121, 130])
@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("a,beta,gamma", [(0.25, 0.5, 0.5), (1.0, 0.5, 1.5), (3.0, 2.0, 0.5)])
def test_conditional_against_the_numpy_restatement(oracle, P, state, a, beta, gamma):
    """rtol 1e-11 on the normalised row: the figure tests/test_oracle_kats.py uses for a normalised conditional against
    an independent computation.  Closed labels are exactly 0."""
    K_open, z = STATES[state]
    z = np.asarray(z)
    X = _small_data(P)
    for i in range(len(z)):
        score, norm = oracle.alloc_cond(X, z + 1, i, MAXK, K_open, a, beta, gamma)
        want = ref.conditional(X, z, i, K_open, a, beta, gamma)
        np.testing.assert_allclose(norm[:K_open], want, rtol=1e-11, atol=0, err_msg=f"{state} row {i}")
        assert (norm[K_open:] == 0.0).all() and np.isneginf(score[K_open:]).all(), (state, i)
        assert np.isfinite(score[:K_open]).all(), (state, i)   # an open label is never shut, empty or not
        assert norm.sum() == pytest.approx(1.0, abs=1e-14)


def test_the_states_hold_what_they_are_for():
    K_open, z = STATES["singleton-empty-closed"]
    nk = np.bincount(z, minlength=MAXK)
    assert nk[2] == 1 and z[10] == 2 and nk[3] == 0 and K_open == 4 < MAXK
    assert STATES["one-open"][0] == 1 and STATES["all-open"][0] == MAXK
    nk = np.bincount(STATES["all-open"][1], minlength=MAXK)
    assert nk[4] == 1 and nk[1] == 0


# ---------------------------------------------------------------- 2. the tie to the collapsed chain
@pytest.mark.parametrize("P", alloc_cases.TIE_P)
@pytest.mark.parametrize("batch", [1, 64])
def test_no_label_empty_or_single_is_the_collapsed_chain_byte_for_byte(oracle, batch, P):
    """K_open = maxK = 4 and a = 0.25: K a = 1 and a are exact in binary, and the tie data keep every label above one
    row (tests/test_alloc_ref.py), so the third mode must write the bytes of the first at alpha = 1"""
    X, z0 = alloc_cases.tie_start(P)
    S = alloc_cases.TIE_SWEEPS + 1
    a = oracle.alloc(X, z0, S, 4, 4, 0.25, alloc_cases.BETA, alloc_cases.GAMMA, 0, alloc_cases.TIE_SEED, batch=batch)
    b = oracle.collapsed(X, z0, S, 4, 1.0, alloc_cases.BETA, alloc_cases.GAMMA, 1.0, 1.0, 0, alloc_cases.TIE_SEED, batch=batch)
    assert a["z"].tobytes() == b["z"].tobytes()
    assert a["theta"][:, :, 1:].tobytes() == b["theta"][:, :, 1:].tobytes()
    assert np.isnan(a["theta"][:, :, 0]).all() and np.isnan(b["theta"][:, :, 0]).all()


def test_sweeps_continue_from_any_sweep_number(oracle):
    """first_sweep: a chain stopped after sweep 3 and continued from its labels with first_sweep = 4 is the chain"""
    c = cases.CONTENT_BY_NAME["P33-padding-labels"]
    X, z0 = cases.content_start(c.name)
    whole = oracle.alloc(X, z0, 8, c.maxK, c.K_open, c.a, c.beta, c.gamma, 0, c.seed, batch=c.batch)
    rest = oracle.alloc(X, whole["z"][3], 5, c.maxK, c.K_open, c.a, c.beta, c.gamma, 0, c.seed, batch=c.batch, first_sweep=4)
    np.testing.assert_array_equal(rest["z"], whole["z"][3:])
    assert rest["theta"][:, :, 1:].tobytes() == whole["theta"][:, :, 4:].tobytes()
    burnt = oracle.alloc(X, z0, 8, c.maxK, c.K_open, c.a, c.beta, c.gamma, 3, c.seed, batch=c.batch)
    np.testing.assert_array_equal(burnt["z"], whole["z"][3:])
    assert burnt["theta"].tobytes() == whole["theta"][:, :, 3:].tobytes()


def test_a_row_on_a_closed_label_is_refused(oracle):
    X = _small_data(5)
    with pytest.raises(RuntimeError):
        oracle.alloc(X, np.array([1] * 11 + [3], dtype=np.int32), 3, 4, 2, 1.0, 0.5, 0.5, 0, 1)


# ---------------------------------------------------------------- 3. the scan samples the enumerated posterior
def test_the_scan_samples_the_dirichlet_multinomial_posterior(oracle):
    """rule and data of tests/test_gpu_alloc.py::test_open_empties_sample_the_dirichlet_multinomial_posterior, run on
    the CPU: batch 1, K_open = maxK = 3, the seven observations, 30 000 kept sweeps under the 4-standard-error rule"""
    X = np.asfortranarray(seven_observations().astype(np.int32))
    a7 = 0.7
    parts, w, _ = ref.exact_posterior(X, 3, a7, alloc_cases.BETA, alloc_cases.GAMMA, ref.uniform_prior(3), fixed_K=3)
    z0 = np.random.default_rng(5).integers(1, 4, 7).astype(np.int32)
    out = oracle.alloc(X, z0, 30_001, 3, 3, a7, alloc_cases.BETA, alloc_cases.GAMMA, 1, 5, batch=1)
    smchk.check_against_enumeration([ref.sm.canon(r) for r in out["z"]], parts, w)
    occ = np.stack([(out["z"] == k + 1).any(axis=1) for k in range(3)], axis=1)
    assert any((~occ[:-1, k] & occ[1:, k]).any() for k in range(3))   # an emptied label is taken again


# ---------------------------------------------------------------- 4. every case reaches what it is for
@pytest.mark.parametrize("name", [c.name for c in cases.CONTENT])
def test_every_content_case_reaches_what_it_is_for(oracle, name):
    c = cases.CONTENT_BY_NAME[name]
    X, z0 = cases.content_start(name)
    assert z0.max() <= c.K_open and len(np.unique(z0)) < c.K_open or c.K_open == 1   # an open label starts empty
    out = oracle.alloc(X, z0, c.sweeps + 1, c.maxK, c.K_open, c.a, c.beta, c.gamma, 0, c.seed, batch=c.batch)
    print(name, cases.check_reached(c, out["z"]))
    # theta-hat belongs to the labels: S / Nk, NaN where a label is empty
    z = out["z"][-1] - 1
    nk = np.bincount(z, minlength=c.maxK)
    S = np.zeros((c.maxK, c.P))
    np.add.at(S, z, X)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = S / nk[:, None]
    np.testing.assert_array_equal(out["theta"][:, :, -1], want)


def test_the_content_cases_cover_what_the_sweep_can_take():
    cs = cases.CONTENT
    assert {c.P for c in cs} >= {1, 5, 6, 32, 33, 120, 121, 128, 130, 241, 1024}
    assert {c.maxK for c in cs} >= {4, 6, 13, 64}
    assert {c.a for c in cs} >= {0.25, 1.0, 3.0}
    assert {1, 64} <= {c.batch for c in cs} and any(c.batch == c.N for c in cs)
    assert {1, 2} <= {c.K_open for c in cs}
    assert any(c.K_open == c.maxK - 1 for c in cs) and any(c.K_open == c.maxK for c in cs)
    assert sum(c.beta != c.gamma for c in cs) >= 2
    assert all(80 <= c.N <= 600 and 40 <= c.sweeps <= 100 for c in cs)


@pytest.mark.parametrize("name", [c.name for c in cases.FORMS])
def test_every_form_case_reaches_what_it_is_for(oracle, name):
    c = cases.FORM_BY_NAME[name]
    X, z0 = cases.form_start(name)
    assert z0.max() < c.K_open or c.K_open < c.maxK
    out = oracle.alloc(X, z0, cases.FORM_SWEEPS + 1, c.maxK, c.K_open, c.a, alloc_cases.BETA, alloc_cases.GAMMA, 0, c.seed,
                       batch=c.batch)
    print(name, cases.check_reached(c, out["z"]))


def test_the_form_cases_cover_every_family_an_armed_chain_selects():
    by = {}
    for c in cases.FORMS:
        by.setdefault(c.family, []).append(cases.kt_of(c.maxK))
        assert 3000 <= c.N <= 10_000
    assert set(by) == {"default", "two-lane", "step-down-768", "step-down-512", "256", "generic"}
    # per family at least three accumulator counts, its smallest and largest among them (chain.hip's kernel set as
    # tests/test_gpu_chunks.py SELECTABLE writes it out, tier 1 / 2 of the counting samplers)
    ends = {"default": (4, 64), "two-lane": (16, 64), "step-down-768": (4, 20), "step-down-512": (4, 32), "256": (4, 56),
            "generic": (4, 64)}
    for fam, kts in by.items():
        assert len(set(kts)) >= 3 and (min(kts), max(kts)) == ends[fam], (fam, sorted(kts))
    assert 2 * sum(c.K_open < c.maxK for c in cases.FORMS) >= len(cases.FORMS)


# ---------------------------------------------------------------- 5. the chain draws from the conditional
def _draw(oracle, score, u):
    """the oracle's draw_index over scores_to_weights, restated: the number of k with u * total >= c_k"""
    w = oracle.expw_array(score - score.max())
    c = np.cumsum(w)     # (sequential, in label order)
    return int((u * c[-1] >= c).sum())


@pytest.mark.parametrize("name", ["P33-padding-labels", "P128-width-4-tier-2", "P130-generic"])
def test_a_batch_draws_every_row_from_its_conditional(oracle, name):
    """one batch-N sweep: every row's new label is the inverse-CDF draw from oracle.alloc_cond under the starting labels,
    which section 1 ties to NumPy -- so the chain's tables (built once per batch, kept while a label is untouched) and
    the per-row conditional are one arithmetic"""
    c = cases.CONTENT_BY_NAME[name]
    assert c.batch == c.N
    X, z0 = cases.content_start(name)
    for first in (1, 7):
        got = oracle.alloc(X, z0, 2, c.maxK, c.K_open, c.a, c.beta, c.gamma, 0, c.seed, batch=c.batch, first_sweep=first)["z"][1]
        for i in range(c.N):
            score, _ = oracle.alloc_cond(X, z0, i, c.maxK, c.K_open, c.a, c.beta, c.gamma)
            assert got[i] == 1 + _draw(oracle, score, oracle.z_uniform(c.seed, i, first)), (name, i)


# ---------------------------------------------------------------- 6. the two protocols of the GPU tests, on the CPU
def test_the_K_schedule_reaches_what_it_is_for(oracle):
    X, z = cases.k_start()
    K, Ks, zs = cases.K_MAXK, [], [z]
    for step in range(cases.K_SWEEPS):
        K = cases.k_schedule(step, z, K)
        Ks.append(K)
        z = oracle.alloc(X, z, 2, cases.K_MAXK, K, cases.K_A, alloc_cases.BETA, alloc_cases.GAMMA, 0, cases.K_SEED,
                         batch=cases.K_BATCH, first_sweep=step + 1)["z"][1]
        zs.append(z)
    print(Ks, cases.k_reached(Ks, zs))


def test_the_moves_between_the_sweeps_reach_what_they_are_for(oracle, tmp_path):
    """the restatement's move (p_E from the host build), then the oracle's sweep, 40 rounds: an accepted eject and an
    accepted absorb with its swap sit directly ahead of a compared sweep"""
    import alloc_checks as chk
    exe = chk.build_host(tmp_path)
    for name, batch in cases.MOVE_CASES.items():
        seen = []
        case = alloc_cases.BY_NAME[name]
        X, z1, lp = alloc_cases.start(case)
        z, K = z1.astype(np.int64) - 1, case.K0
        for r in range(cases.MOVE_ROUNDS):
            j = r + 1
            h = chk.host_draws(exe, tmp_path, case.seed, j, 0, K, case.maxK, case.e)
            m = ref.move(X, z, K, case.maxK, case.a, alloc_cases.BETA, alloc_cases.GAMMA, case.e, lp,
                         ref.PhiloxDraws(case.seed, j, 0, pe=h["pe"]))
            seen.append(("eject" if m["kind"] == ref.EJECT else "absorb", m["K"] != K, m["labels"][1], K))
            z, K = m["z"], m["K"]
            z = oracle.alloc(X, (z + 1).astype(np.int32), 2, case.maxK, K, case.a, alloc_cases.BETA, alloc_cases.GAMMA, 0,
                             case.seed, batch=batch, first_sweep=j)["z"][1].astype(np.int64) - 1
            assert z.max() < K
        if name in cases.MOVE_REACH:
            cases.moves_reached(seen)
