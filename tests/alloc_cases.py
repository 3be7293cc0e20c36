"""The shapes at which tests/test_gpu_alloc.py replays device moves against the restatement, and what each of them is
there to reach.  Kind, labels and members of a move are pure functions of the seed, the counters, K and the labels, and
every case starts its moves from planted labels, so the restatement alone (tests/test_alloc_ref.py, on the CPU, with
p_E from the host build of the spec) shows that a case's seed reaches what the case is for before the device is asked."""
import collections

import numpy as np

import alloc_ref as ref
from split_merge_cases import mixture

BETA = GAMMA = 0.5
STEPS = 40

# plant: (N, comp, rng) -> 1-based labels in 1..K0; prior: "poisson" or "uniform"; reach: what check_reached looks for
Case = collections.namedtuple("Case", "name N P maxK K0 a e prior plant data_seed seed sorted reach")


def random_labels(K0):
    return lambda N, comp, rng: rng.integers(1, K0 + 1, N).astype(np.int32)


def by_component(N, comp, rng):
    return (comp + 1).astype(np.int32)


def one_label(N, comp, rng):
    return np.ones(N, dtype=np.int32)


def round_robin(K0):
    return lambda N, comp, rng: (np.arange(N) % K0 + 1).astype(np.int32)


# The chain seed: 17 was tried first at every shape; tests/test_alloc_ref.py holds every case to `check_reached` with
# the restatement alone.
CASES = [
    Case("original-P37", 600, 37, 8, 4, 1.0, 1.0, "poisson", random_labels(4), 4, 17, False, ("both-kinds",)),
    Case("original-P130", 600, 130, 8, 4, 1.0, 1.0, "poisson", random_labels(4), 4, 17, False, ("both-kinds",)),
    # N = 2500 = 9 * 256 + 196: ten workgroups; the rows sorted by generating component and labelled by it, so a
    # label's rows leave whole workgroups without a member; nd = 1 in word 1
    Case("many-rows", 2500, 33, 8, 3, 1.0, 1.0, "poisson", by_component, 4, 17, True, ("both-kinds", "empty-workgroup")),
    Case("one-feature", 300, 1, 8, 4, 1.0, 1.0, "poisson", random_labels(4), 4, 17, False, ("both-kinds",)),
    Case("full-word", 300, 32, 8, 4, 1.0, 1.0, "poisson", random_labels(4), 4, 17, False, ("both-kinds",)),
    Case("two-full-words", 300, 64, 8, 4, 1.0, 1.0, "poisson", random_labels(4), 4, 17, False, ("both-kinds",)),
    Case("widest-P", 600, 1024, 8, 4, 1.0, 1.0, "poisson", random_labels(4), 4, 17, False, ("both-kinds",)),
    Case("all-64-labels", 600, 20, 64, 64, 1.0, 1.0, "uniform", round_robin(64), 4, 17, False, ("all-64",)),
    Case("K-is-1", 300, 20, 8, 1, 1.0, 1.0, "poisson", one_label, 4, 17, False, ("k1-eject",)),
    Case("K-is-maxK", 300, 20, 4, 4, 1.0, 1.0, "poisson", random_labels(4), 4, 17, False, ("kmax-absorb",)),
    # few rows, a small a and the uniform prior: ejecting and absorbing an empty component are accepted often, and the
    # absorbs meet both the last label (no relabel pass) and another one (the relabel pass)
    Case("empties", 40, 12, 6, 3, 0.25, 1.0, "uniform", one_label, 4, 17, False,
         ("both-kinds", "eject-empty-accepted", "absorb-empty-accepted", "absorb-last", "absorb-swap")),
    Case("eject-a", 300, 37, 8, 4, 1.0, 2.5, "poisson", random_labels(4), 4, 17, False, ("both-kinds",)),
]
BY_NAME = {c.name: c for c in CASES}


# the tie to the collapsed chain: four crisp components, the rows labelled by component, eight sweeps
TIE_N, TIE_P, TIE_SEED, TIE_SWEEPS = 700, (24, 130), 21, 8


def tie_start(P, seed=3):
    """four crisp components -- every feature's rate 0.05 or 0.95, the pattern a component's own -- and their labels"""
    rng = np.random.default_rng(seed)
    comp = rng.integers(4, size=TIE_N)
    rates = np.where(rng.random((4, P)) < 0.5, 0.05, 0.95)
    X = (rng.random((TIE_N, P)) < rates[comp]).astype(np.int32)
    return np.asfortranarray(X), (comp + 1).astype(np.int32)


def data(case):
    return mixture(case.N, case.P, [0.2, 0.5, 0.8], case.data_seed, case.sorted)


def start(case):
    """X, the planted 1-based labels, log p(K)"""
    X, comp = data(case)
    z1 = case.plant(case.N, comp, np.random.default_rng(case.seed))
    lp = ref.poisson_prior(case.maxK) if case.prior == "poisson" else ref.uniform_prior(case.maxK)
    return X, z1, lp


def check_reached(case, start_labels, seen):
    """seen: per move a dict with kind, k_before, labels (0-based j1, j2), accepted, n_before, n_after, side"""
    kinds = {s["kind"] for s in seen}
    for what in case.reach:
        if what == "both-kinds":
            assert kinds == {ref.EJECT, ref.ABSORB}, kinds
        elif what == "empty-workgroup":
            ok = False
            for s in seen:
                touched = np.asarray(s["side"]) != ref.OUTSIDE
                blocks = [touched[b:b + 256] for b in range(0, case.N, 256)]
                ok = ok or (any(b.any() for b in blocks) and any(not b.any() for b in blocks))
            assert ok
        elif what == "all-64":
            assert len(np.unique(start_labels)) == 64 and seen[0]["k_before"] == 64 and seen[0]["kind"] == ref.ABSORB
        elif what == "k1-eject":
            assert seen[0]["k_before"] == 1 and seen[0]["kind"] == ref.EJECT
        elif what == "kmax-absorb":
            assert seen[0]["k_before"] == case.maxK and seen[0]["kind"] == ref.ABSORB
        elif what == "eject-empty-accepted":
            assert any(s["kind"] == ref.EJECT and s["accepted"] and s["n_before"][0] == 0 for s in seen)
        elif what == "absorb-empty-accepted":
            assert any(s["kind"] == ref.ABSORB and s["accepted"] and s["n_before"][1] == 0 for s in seen)
        elif what == "absorb-last":
            assert any(s["kind"] == ref.ABSORB and s["accepted"] and s["labels"][1] == s["k_before"] - 1 for s in seen)
        elif what == "absorb-swap":
            assert any(s["kind"] == ref.ABSORB and s["accepted"] and s["labels"][1] != s["k_before"] - 1 for s in seen)
        else:
            raise AssertionError(what)
