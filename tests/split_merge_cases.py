"""The shapes at which tests/test_gpu_split_merge.py replays device moves against the restatement, and what each of
them is there to reach.  Pair, kind and members of a move are pure functions of the seed, the counters and the labels,
so the restatement alone (tests/test_split_merge_cases.py, on the CPU) shows that a case's seed reaches what the case
is for before the device is asked to: the labels the moves start from come from the oracle's DP chain, which the device
chain equals bit for bit (tests/test_gpu_parity.py), or are planted."""
import collections

import numpy as np

import split_merge_ref as ref

BETA = GAMMA = 0.5
ALPHA = 1.3
SWEEPS, BATCH = 3, 16  # every case: three sweeps at batch 16, then the moves ahead of sweep 4

# phases: ((scans, steps), ...) on one chain; plant: None (the labels the sweeps left) or a function N -> 1-based labels
Case = collections.namedtuple("Case", "name N P K phases data_seed seed sorted plant")


def wide_k_labels(N):
    """rows 0 .. 258 alone under labels 1 .. 259, every other row under label 260: the first free label is the 261st"""
    z = np.full(N, 260, dtype=np.int32)
    z[:259] = np.arange(1, 260)
    return z


# The chain seed: 17, the seed of the two original cases, was tried first at every shape, and at every shape the
# restatement meets `check_reached` with it (tests/test_split_merge_cases.py holds every case to that on the CPU), so
# no other seed was looked at.
CASES = [
    Case("original-P37", 300, 37, 8, ((2, 40),), 4, 17, False, None),
    Case("original-P130", 300, 130, 8, ((2, 40),), 4, 17, False, None),
    # N = 2500 = 9 * 256 + 196 = 2 * 1024 + 452: ten workgroups, the third trip of k_sm_decide's row loop; the rows
    # sorted by generating component, so a cluster's rows leave whole workgroups without a member; nd = 1 in word 1
    Case("many-rows", 2500, 33, 8, ((2, 40),), 4, 17, True, None),
    Case("one-feature", 300, 1, 8, ((2, 40),), 4, 17, False, None),
    Case("full-word", 300, 32, 8, ((2, 40),), 4, 17, False, None),
    Case("two-full-words", 300, 64, 8, ((2, 40),), 4, 17, False, None),
    Case("widest-P", 600, 1024, 8, ((1, 40),), 4, 17, False, None),
    Case("wide-K", 600, 20, 300, ((2, 40),), 4, 17, False, wide_k_labels),
    Case("no-scans", 300, 37, 8, ((0, 40),), 4, 17, False, None),
    Case("scans-changing", 300, 37, 8, ((2, 12), (6, 12), (1, 12)), 4, 17, False, None),
]
BY_NAME = {c.name: c for c in CASES}


def mixture(N, P, thetas, seed, in_order=False):
    """N rows of P features that share their component's rate; `in_order`: the rows in the order of their generating
    component.  Returns X and the components."""
    rng = np.random.default_rng(seed)
    comp = rng.integers(len(thetas), size=N)
    if in_order:
        comp = np.sort(comp)
    X = (rng.random((N, P)) < np.asarray(thetas)[comp][:, None]).astype(np.int32)
    return np.asfortranarray(X), comp


def data(case):
    """the mixture of the original cases"""
    return mixture(case.N, case.P, [0.2, 0.5, 0.8], case.data_seed, case.sorted)[0]


def scans_of(case):
    """what _replay of tests/test_gpu_split_merge.py takes as `scans`: a number, or the phases of a chain that changes it"""
    return case.phases[0][0] if len(case.phases) == 1 else case.phases


def steps_of(case):
    return sum(n for _, n in case.phases)


def start_labels(case, X, oracle):
    """1-based labels the moves start from, without a device"""
    if case.plant is not None:
        return case.plant(case.N)
    return oracle.dp(X, SWEEPS + 1, ALPHA, BETA, GAMMA, 1, 1, 0, case.K, seed=case.seed, batch=BATCH)["z"][SWEEPS].copy()


def restated(case, X, z1):
    """every move of the case by the restatement alone, from labels z1 (1-based): [(kind, labels 1-based, members,
    launch_side)]"""
    z = np.asarray(z1, dtype=np.int64) - 1
    seen, step = [], 0
    for scans, n in case.phases:
        for _ in range(n):
            r = ref.move(X, z, case.K, ALPHA, BETA, GAMMA, scans, ref.PhiloxDraws(case.seed, SWEEPS + 1, step))
            seen.append((r["kind"], tuple(v + 1 for v in r["labels"]), r["members"], r.get("launch_side")))
            z = r["z"]
            step += 1
    return seen


def check_reached(case, seen):
    """Conditions, not measurements: what the case is there to reach, from the (kind, labels 1-based, members,
    launch_side) of the moves it saw."""
    kinds = {s[0] for s in seen}
    assert {"split", "merge"} <= kinds, (case.name, kinds)
    if case.name == "many-rows":
        grid = -(-case.N // 256)
        assert grid == 10 and case.N > 2 * 1024
        # a step whose members span fewer workgroups than the grid: a block of 256 rows entirely outside the move
        assert any(s[3] is not None and any(np.all(s[3][b * 256:(b + 1) * 256] == ref.OUTSIDE) for b in range(grid))
                   for s in seen if s[0] != "skipped"), case.name
    if case.name == "wide-K":
        assert any(s[0] == "split" and s[1][1] >= 257 for s in seen), case.name
        assert any(s[0] == "merge" and s[2] == 0 for s in seen), case.name
