"""The shapes at which tests/test_gpu_alloc_split.py steps the allocation sampler's split-merge move by hand against the
restatement (tests/alloc_split_ref.py), and what each of them is there to reach.

The moves of a case are keyed (seed, sweep 1, move m) and nothing else runs between them, so the restatement alone
(tests/test_alloc_split_ref.py, on the CPU) shows that a case's seed reaches what the case is for before the device is
asked.  Data: crisp planted components (every feature's rate 0.1 or 0.9).  The starting labels put the first two
components under label 1 (a split the data ask for) and cut every other component at random into two labels (merges
the data ask for); `empty` more open labels hold nothing.
"""
import collections
import functools

import numpy as np

import alloc_ref as al
import alloc_split_ref as ref

BETA, GAMMA = 0.5, 0.5
A7 = 0.7  # the Dirichlet parameter of the seven-observation chains

# reach: split+ / split- / merge+ / merge-: an accepted / rejected move of that kind; skipped: a split at K == maxK;
# K1: a split proposed at K == 1; nomembers: a move whose block holds the two anchors only; a<b+ / a>b+: an accepted merge
# with la < lb / la > lb; last+: an accepted merge with lb == K - 1 (nothing moved); moved+: one with lb < K - 1 (label
# K - 1 moved into the gap); edge: anchors in the first and in the last row
Case = collections.namedtuple("Case", "name N P maxK K0 a beta gamma prior scans comps merged empty steps seed reach")

# The seed: 17 was tried first at every shape; where the restatement did not reach what the case is for with it, the next
# seeds were tried in order and the first that does is recorded.
CASES = [
    # two rows: the anchors are the first and the last row and the only rows of their block; K = 1 allows a split only
    Case("N2-P1-maxK2", 2, 1, 2, 1, 1.0, 0.5, 0.5, "uniform", 0, 1, 1, 0, 30, 17, ("K1", "nomembers", "edge", "split+", "split-", "merge+", "a<b+", "a>b+", "last+", "moved+")),
    # K == maxK with both rows under one label: every move is a skipped split
    Case("N2-P33-maxK2-full", 2, 33, 2, 2, 1.0, 0.5, 0.5, "poisson", 1, 1, 1, 1, 6, 17, ("skipped", "edge")),
    Case("N255-P32-maxK13", 255, 32, 13, 5, 1.0, 0.5, 0.5, "poisson", 1, 4, 2, 0, 40, 17, ("split+", "merge+", "split-", "merge-")),
    Case("N256-P33-maxK13", 256, 33, 13, 6, 0.7, 0.4, 1.1, "uniform", 3, 4, 2, 1, 40, 17, ("split+", "merge+", "moved+")),
    Case("N257-P130-maxK64", 257, 130, 64, 5, 1.0, 0.5, 0.5, "poisson", 1, 4, 2, 0, 40, 17, ("split+", "merge+", "a<b+", "a>b+")),
    Case("N513-P1024-maxK13", 513, 1024, 13, 3, 1.0, 0.5, 0.5, "poisson", 0, 3, 2, 0, 30, 17, ("split+", "merge+", "merge-", "moved+")),
    # every label open (one of them empty): splits are skipped until a merge has gone through (seed 17: a merge is
    # accepted ahead of the first split)
    Case("N300-P20-maxK4-full", 300, 20, 4, 4, 1.0, 0.5, 0.5, "poisson", 1, 2, 1, 1, 30, 18, ("skipped", "merge+", "merge-")),
    Case("N300-P20-K1", 300, 20, 13, 1, 1.0, 0.5, 0.5, "poisson", 3, 2, 2, 0, 20, 17, ("K1", "split+")),
]
BY_NAME = {c.name: c for c in CASES}
EVERYTHING = {"split+", "split-", "merge+", "merge-", "skipped", "K1", "nomembers", "a<b+", "a>b+", "last+", "moved+", "edge"}


def log_prior_of(case):
    return al.poisson_prior(case.maxK) if case.prior == "poisson" else al.uniform_prior(case.maxK)


@functools.lru_cache(maxsize=None)
def start(name):
    """X (N x P int32, column-major) and the 1-based starting labels in 1..K0"""
    c = BY_NAME[name]
    rng = np.random.default_rng(5)
    rates = np.where(rng.random((c.comps, c.P)) < 0.5, 0.1, 0.9)
    comp = rng.integers(c.comps, size=c.N)
    X = (rng.random((c.N, c.P)) < rates[comp]).astype(np.int32)
    z = np.ones(c.N, dtype=np.int32)
    nxt = 2
    for k in range(c.merged, c.comps):  # the components past the merged ones, each cut into two labels
        rows = np.flatnonzero(comp == k)
        z[rows] = nxt + rng.integers(2, size=len(rows))
        nxt += 2
    if c.N == 2 and c.K0 == 1:
        z[:] = 1
    assert nxt - 1 + c.empty == c.K0 or c.N == 2, (name, nxt, c.K0)
    assert z.max() <= c.K0 <= c.maxK
    return np.asfortranarray(X), z


def restated_steps(case):
    """the case's moves by the restatement alone, from the device's own streams"""
    X, z1 = start(case.name)
    lp = log_prior_of(case)
    z, K = z1.astype(np.int64) - 1, case.K0
    seen = []
    for m in range(case.steps):
        r = ref.move(X, z, K, case.maxK, case.a, case.beta, case.gamma, lp, case.scans, ref.PhiloxDraws(case.seed, 1, m))
        seen.append(r)
        z, K = r["z"], r["K"]
    return seen


def reached(case, seen):
    """seen: the steps as dicts with kind, accepted, rows, labels (0-based), members, k_before"""
    got = set()
    for r in seen:
        kind, acc = r["kind"], r["accepted"]
        la, lb = r["labels"]
        if set(r["rows"]) == {0, case.N - 1}:
            got.add("edge")
        if kind == ref.SKIPPED:
            got.add("skipped")
            continue
        got.add(kind + ("+" if acc else "-"))
        if kind == ref.SPLIT and r["k_before"] == 1:
            got.add("K1")
        if r["members"] == 0:
            got.add("nomembers")
        if kind == ref.MERGE and acc:
            got.add("a<b+" if la < lb else "a>b+")
            got.add("last+" if lb == r["k_before"] - 1 else "moved+")
    return got


assert set().union(*(c.reach for c in CASES)) == EVERYTHING


def check_reached(case, seen):
    got = reached(case, seen)
    assert set(case.reach) <= got, (case.name, sorted(set(case.reach) - got), sorted(got))
    return got


# -------------------------------------------------------------------------------------------------- the point of the feature
# Crisp planted data as alloc_sweep_cases.planted builds them, every row on one label, K0 = 1, Poisson prior, a = 1, one
# eject / absorb and two split-merge moves (SPLIT_MERGE_SCANS scans) ahead of every sweep from the second.  The
# restatement's chain (alloc_split_ref.planted_chain, batch 1) arrives at PLANT_COMPS non-empty labels, and stays, at
# sweeps 14, 5, 9, 10, 7, 4, 4, 9, 6, 5 for the seeds 1..10: the budget is twice the slowest and a little more.
PLANT_N, PLANT_P, PLANT_COMPS, PLANT_MAXK, PLANT_DATA_SEED = 2000, 32, 5, 30, 5
PLANT_SWEEPS, PLANT_SCANS, PLANT_SEEDS = 30, 5, tuple(range(1, 11))
PLANT_ARRIVALS = (14, 5, 9, 10, 7, 4, 4, 9, 6, 5)
