"""The NumPy restatement of the ECR relabelling (tests/ecr_ref.py) held to the definitions on the CPU, and the reach
of its cases over the forms of the device kernels (bm.ecr_plan touches no device)."""
import numpy as np
import pytest

import bmm_mcmc_amd as bm
import ecr_ref as E


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6])
def test_agreement_equals_brute_force(K):
    assert hasattr(bm, "ecr_relabel") and hasattr(bm, "ecr_plan")
    rng = np.random.default_rng(100 + K)
    for trial in range(6):
        N = int(rng.integers(1, 60))
        z = rng.integers(0, K, size=(4, N)).astype(np.int32)
        if trial % 2:  # skewed: empty labels, many equal costs
            z = np.minimum(z, rng.integers(0, K, size=(4, 1))).astype(np.int32)
        c = rng.integers(0, K, size=N).astype(np.int32)
        r = E.ecr(z, K, c)
        for t in range(4):
            assert sorted(r["permutations"][t]) == list(range(K))
            assert int(r["agree"][t]) == E.brute_agree(r["tables"][t])
            assert int(r["agree"][t]) == int((r["z"][t] == c).sum())


@pytest.mark.parametrize("K,N,noise", [(2, 200, 0.15), (3, 300, 0.3), (5, 1000, 0.4), (8, 2000, 0.3), (20, 4000, 0.25)])
def test_planted_permutations_are_undone(K, N, noise):
    assert hasattr(bm, "ecr_relabel")
    z, truth, s = E.noisy(7 * K, 12, N, K, noise)
    r = E.ecr(z, K, truth)
    for t in range(12):
        assert np.array_equal(r["permutations"][t][s[t]], np.arange(K))
    it = E.ecr(z, K, None)
    g = it["permutations"][0][s[0]]  # the one global permutation left
    assert sorted(g) == list(range(K))
    for t in range(12):
        assert np.array_equal(it["permutations"][t][s[t]], g)
    assert it["converged"]


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_cases_are_monotone_and_converge(case):
    assert hasattr(bm, "ecr_relabel")
    z, pivot, r = E.solved(case)
    assert all(b >= a for a, b in zip(r["totals"], r["totals"][1:]))
    assert r["converged"] and r["iterations"] <= 50
    if pivot is None:
        assert r["iterations"] >= 2  # the stopping rule compares two totals


def test_the_cases_reach_every_form():
    plans = [bm.ecr_plan(c["S"], c["N"], c["K"]) for c in E.CASES]
    given = [p for p, c in zip(plans, E.CASES) if c["pivot"]]
    itera = [p for p, c in zip(plans, E.CASES) if not c["pivot"]]
    for group in (given, itera):  # the tables pass runs in both
        assert {p["tables_lds"] for p in group} == {0, 1}
        assert {p["slices"] > 1 for p in group} == {False, True}
        assert {p["row_blocks"] > 1 for p in group} == {False, True}
    assert {p["copies"] for p in plans if p["tables_lds"]} >= {1, 2, 16}
    assert {p["votes_lds"] for p in itera} == {0, 1}
    assert {p["votes_workgroups"] > 1 for p in itera if p["votes_lds"]} == {False, True}
    assert {p["votes_workgroups"] > 1 for p in itera if not p["votes_lds"]} == {False, True}
    # one byte per label in the stand-alone call's block; a run reads the resident int32 trace (tests/test_gpu_ecr.py
    # runs all four samplers through it)
    assert {p["label_bytes"] for p in plans} == {1}
    # the boundaries themselves
    assert bm.ecr_plan(17, 4099, 110)["tables_lds"] == 1 and bm.ecr_plan(17, 4099, 111)["tables_lds"] == 0
    assert bm.ecr_plan(17, 4099, 96)["votes_lds"] == 1 and bm.ecr_plan(17, 4099, 97)["votes_lds"] == 0
    for p in plans:
        if p["tables_lds"]:
            assert 0 < p["tables_lds_bytes"] <= 48 << 10
        assert p["span"] % 256 == 0 and p["slices"] * p["span"] >= p["pitch"] - 15
    for S, N, K in [(0, 5, 3), (5, 0, 3), (5, 5, 0), (5, 5, 129), (65536, 5, 3)]:
        with pytest.raises(bm.BmmError):
            bm.ecr_plan(S, N, K)
