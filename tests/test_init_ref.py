"""The k-modes++ initial allocation as defined (include/bmm_mcmc.h "initial allocation"), on the CPU: properties of the
NumPy restatement (tests/init_ref.py), a hand-worked case, its uniforms against the spec header compiled for the host,
and that every case of tests/init_cases.py reaches what it is for."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import init_cases as cases  # noqa: E402
import init_ref as ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(os.path.dirname(HERE), "bmm-mcmc_amd", "csrc")


def _random_sets(n=50):
    rng = np.random.default_rng(2024)
    for t in range(n):
        N, P, K = int(rng.integers(2, 201)), int(rng.integers(1, 41)), int(rng.integers(1, 9))
        comps = int(rng.integers(1, 5))
        theta = rng.random((comps, P))
        X = (rng.random((N, P)) < theta[rng.integers(comps, size=N)]).astype(np.int32)
        if t % 5 == 0:  # few distinct rows: the seeding stops early
            X = X[rng.integers(min(N, 3), size=N)]
        yield X, K, 100 + t


def test_cost_never_increases_and_labels_are_valid():
    """a theorem of the tie rule: (a) moves every bit to the majority of its cluster and keeps it on a tie, (b) moves
    every row to a nearest centre; neither can raise the cost, from the seeding on"""
    stopped = 0
    for X, K, seed in _random_sets():
        r = ref.kmodes(X, K, seed, 20)
        assert all(a >= b for a, b in zip(r["costs"], r["costs"][1:])), r["costs"]
        assert r["labels"].min() >= 0 and r["labels"].max() < r["k_eff"] <= K
        assert len(set(r["rows"].tolist())) == len(r["rows"]) == r["k_eff"]
        distinct = len(np.unique(X, axis=0))
        assert r["k_eff"] == min(K, distinct)
        stopped += r["k_eff"] < K
        assert r["Nk"].sum() == len(X) and r["cost"] == ref.distances(X, r["centres"])[np.arange(len(X)), r["labels"]].sum()
        assert r["rounds_run"] == len(r["changed"]) <= 20
        if r["rounds_run"] < 20:
            assert r["changed_last"] == 0
    assert stopped >= 5  # the early stop was met


def test_hand_worked_case():
    """N = 6, P = 3, Kc = 2, by hand.  Rows: 0:000 1:001 2:000 3:111 4:110 5:111.
    r_0 = floor(u_0 * 6); say centre 0 = row r_0.  The test fixes the draws by choosing the seed whose u_0 lands on row 0
    and follows the definition from there:
      dist to 000: [0, 1, 0, 3, 2, 3], T = 9, inclusive prefix sums [0, 1, 1, 4, 6, 9];
      t = floor(u_1 * 9): t = 0 -> row 1; t in 1..3 -> row 3; t in 4..5 -> row 4; t in 6..8 -> row 5.
    With the second centre 111 (row 3 or 5): dist = [0, 1, 0, 0, 1, 0], near = [0, 0, 0, 1, 1, 1], cost 2.
      round 1 (a): cluster 0 = rows 0, 1, 2: S = [0, 0, 1], Nk = 3 -> 000; cluster 1 = rows 3, 4, 5: S = [3, 3, 2] -> 111.
              (b): nothing moves: changed = 0, cost 2; the refinement ends with rounds_run = 1."""
    X = np.array([[0, 0, 0], [0, 0, 1], [0, 0, 0], [1, 1, 1], [1, 1, 0], [1, 1, 1]], dtype=np.int32)
    seed = next(s for s in range(1000) if int(ref.init_uniform(s, 0) * 6.0) == 0 and 1 <= int(ref.init_uniform(s, 1) * 9.0) <= 3)
    r = ref.kmodes(X, 2, seed, 10)
    assert r["rows"].tolist() == [0, 3]
    assert r["labels"].tolist() == [0, 0, 0, 1, 1, 1]
    assert r["centres"].tolist() == [[0, 0, 0], [1, 1, 1]]
    assert r["Nk"].tolist() == [3, 3]
    assert (r["k_eff"], r["rounds_run"], r["changed_last"], r["cost"]) == (2, 1, 0, 2)
    assert r["costs"] == [2, 2]
    # a tie in (a): rows 000 and 110 alone under one label keep the centre's bits where 2 S == Nk
    r1 = ref.kmodes(np.array([[0, 0, 0], [1, 1, 0]], dtype=np.int32), 1, seed, 3)
    assert r1["centres"].tolist() == [X[0].tolist()] and r1["cost"] == 2 and r1["rounds_run"] == 1


def test_init_uniform_matches_the_spec_header(tmp_path):
    exe = os.path.join(str(tmp_path), "init_uniform_host")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", INC, os.path.join(HERE, "init", "init_uniform_host.cpp"),
                    "-o", exe], check=True)
    for seed in (0, 17, 2 ** 32 + 5, 2 ** 64 - 1):
        out = subprocess.run([exe, str(seed), "40"], check=True, capture_output=True, text=True).stdout.split()
        got = np.array([int(w, 16) for w in out], dtype=np.uint64).view(np.float64)
        want = np.array([ref.init_uniform(seed, j) for j in range(40)])
        assert np.array_equal(got, want)
        assert got.min() >= 0.0 and got.max() < 1.0


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_case_reaches_what_it_is_for(name):
    case = cases.BY_NAME[name]
    cases.check_reached(case, None if case.refused else cases.restated(name))
