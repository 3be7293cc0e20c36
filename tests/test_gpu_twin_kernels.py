"""Bytes before equal bytes after: every flavour of the one count-table kernel (k_count_tables: plain, mask, alloc,
temper) and both flavours of the split-merge kernels (k_sm_launch / scan / decide / commit: DP chain, allocation chain)
against a golden recorded with the separate kernels they replaced (tests/golden/twin_kernels.json).

The restatement tests hold what these kernels compute; this file holds that merging the hand-kept copies changed no bit.
The golden was written by this module's own recording function, run on a build of the commit before the merge:

    python tests/test_gpu_twin_kernels.py --record tests/golden/twin_kernels.json

(two recordings there were identical).  It holds sha256 digests of the raw bytes of the big arrays and the small records
themselves, doubles as bit patterns.  Seeds and step counts of the move cases were chosen on the CPU with the host
restatements (`--seeds` prints the search): the first seed from 17 on whose first 60 moves hold an accepted and a
rejected split, an accepted and a rejected merge and, where the case is there for it, a skipped move; the steps end with
the move that completes the set.

Table cases: N = 600 at batch 250, so the build runs three times a sweep; P = 5 (one word), 37 (a partial second word)
and 128 (kChunkP is 120: the chunk loop's second trip); three sweeps, the last one handing its probabilities over.  They
run the test variant of the library with BMM_DEBUG_NOSELF, so that every batch of every case is built by k_count_tables
and not by the resample workgroups themselves; the collapsed plain P = 5 case also sets BMM_DEBUG_NOSPLIT and
BMM_DEBUG_PK and is asserted to run the packed kernel, so the Tq / write_own32 branch of the build is in the golden.  An
allocation chain refuses the probability hand-off, so its cases digest the state after three plain sweeps.
"""
import collections
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import alloc_ref as al  # noqa: E402
import alloc_split_ref as as_ref  # noqa: E402
import split_merge_ref as sm_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden", "twin_kernels.json")
BETA = GAMMA = 0.5

# ------------------------------------------------------------------------------------------------------ the table builds
TAB_N, TAB_BATCH, TAB_SWEEPS = 600, 250, 3
TableCase = collections.namedtuple("TableCase", "name flavour sampler P K")
# K: collapsed K = 3; DP maxK = 6, so that the new-cluster row k == K is built; alloc maxK = 5 with K set to 3 and label
# 3 empty, so closed labels and an open empty label both occur
TABLE_CASES = [TableCase("%s-%s-P%d" % (f, s, P), f, s, P, K)
               for f, samplers in (("plain", ("collapsed", "dp")), ("mask", ("collapsed", "dp")), ("alloc", ("collapsed",)),
                                   ("temper", ("collapsed", "dp")))
               for s in samplers for P in (5, 37, 128) for K in ((5 if f == "alloc" else 3) if s == "collapsed" else 6,)]
PACKED = "plain-collapsed-P5"
SWITCHES = ("DRAW_FALLBACK", "DRAW_NOEPS", "NOSPLIT", "NOSELF", "CUS", "PK_QUEUE", "NOPK", "PK", "GENERIC", "THREADS")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _bits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _planted(N, P, comps, merged, seed):
    """crisp components (every rate 0.1 or 0.9); the first `merged` under label 1, every other one cut at random into
    two labels of its own: splits and merges the data ask for beside those they do not.  X and 1-based labels."""
    rng = np.random.default_rng(seed)
    rates = np.where(rng.random((comps, P)) < 0.5, 0.1, 0.9)
    comp = rng.integers(comps, size=N)
    X = np.asfortranarray((rng.random((N, P)) < rates[comp]).astype(np.int32))
    z = np.ones(N, dtype=np.int32)
    for k in range(merged, comps):
        rows = np.flatnonzero(comp == k)
        z[rows] = 2 * (k - merged) + 2 + rng.integers(2, size=len(rows))
    return X, z


def mask_of(P):
    """excluded features in the first and in the last word"""
    g = np.ones(P, dtype=np.uint8)
    g[[1, P - 2]] = 0
    return g


def observe_table(bmm, case, setenv):
    """the digests of one table case on the library loaded now (the test variant); setenv(name, value or None)"""
    _capi = bmm._capi
    for k in SWITCHES:
        setenv("BMM_DEBUG_" + k, None)
    setenv("BMM_DEBUG_NOSELF", "1")
    if case.name == PACKED:
        setenv("BMM_DEBUG_NOSPLIT", "1")
        setenv("BMM_DEBUG_PK", "1")
    X, _ = _planted(TAB_N, case.P, 3, 0, 40 + case.P)
    alloc = case.flavour == "alloc"
    z0 = np.random.default_rng(3).integers(1, (2 if alloc else case.K) + 1, TAB_N).astype(np.int32)
    with bmm.Chain(case.sampler, TAB_N, case.P, case.K, alpha=0.8 if alloc else None, beta=BETA, gamma=GAMMA, batch=TAB_BATCH,
                   seed=23) as c:
        c.set_data(X)
        if case.sampler == "collapsed":
            c.set_initial_labels(z0)
        if case.flavour == "mask":
            c.set_features(mask_of(case.P))
        elif case.flavour == "temper":
            c.set_temper(0.5)
        elif alloc:
            c.set_alloc("poisson", 0)
            c.set_k(3)
        assert bool(_capi.lib().bmm_dbg_kernel_packed(c._h)) == (case.name == PACKED), case.name
        out = {}
        if alloc:
            c.sweeps(TAB_SWEEPS)
            out["K"] = c.k()
        else:
            c.sweeps(TAB_SWEEPS - 1)
            out["probs"] = _sha(c.sweep_probs())
        Nk, S = c.counts()
        out.update(z=_sha(c.labels()), Nk=[int(v) for v in Nk], S=_sha(S), alpha=_bits(c.alpha()))
    return out


# ------------------------------------------------------------------------------------------------------------- the moves
# N = 600: three workgroups, a tail of 88 rows; N = 2500: the third trip of the decide kernel's row loop.  `full`: every
# label in use (DP) / open (allocation chain) at the start, so a split is skipped until a merge has gone through.
MoveCase = collections.namedtuple("MoveCase", "name target N P scans full seed steps")
COMPS, MERGED, LABELS = 4, 2, 5  # two components under label 1, two cut in two: five labels
ALPHA, A = 1.3, 1.0
MOVE_FIELDS = ("rows", "labels", "kind", "accepted", "members", "n_before", "n_after", "log_prior", "log_lik", "log_q", "log_u",
               "log_r", "sweep", "move")
ALLOC_FIELDS = MOVE_FIELDS + ("k_before", "k_after", "moved")
WANTED = {("split", True), ("split", False), ("merge", True), ("merge", False)}
# (seed, steps) per case, by `--seeds`
CHOSEN = {
    "dp-N600-P5-scans0": (17, 39),
    "dp-N600-P5-scans2": (17, 17),
    "dp-N600-P37-scans0": (17, 16),
    "dp-N600-P37-scans2": (17, 48),
    "dp-N600-P37-scans2-full": (19, 54),
    "dp-N2500-P5-scans0": (59, 18),
    "dp-N2500-P5-scans2": (17, 18),
    "dp-N2500-P37-scans0": (17, 17),
    "dp-N2500-P37-scans2": (17, 17),
    "alloc-N600-P5-scans0": (19, 15),
    "alloc-N600-P5-scans2": (17, 9),
    "alloc-N600-P37-scans0": (17, 27),
    "alloc-N600-P37-scans2": (17, 27),
    "alloc-N600-P37-scans2-full": (17, 41),
    "alloc-N2500-P5-scans0": (100, 24),
    "alloc-N2500-P5-scans2": (17, 22),
    "alloc-N2500-P37-scans0": (17, 44),
    "alloc-N2500-P37-scans2": (17, 44),
}
MOVE_CASES = [MoveCase("%s-N%d-P%d-scans%d%s" % (t, N, P, s, "-full" if full else ""), t, N, P, s, full,
                       *CHOSEN.get("%s-N%d-P%d-scans%d%s" % (t, N, P, s, "-full" if full else ""), (None, None)))
              for t in ("dp", "alloc") for N in (600, 2500) for P in (5, 37) for s in (0, 2)
              for full in ((False, True) if (N, P, s) == (600, 37, 2) else (False,))]


def _max_k(case):
    return LABELS if case.full else 8


def _start(case):
    return _planted(case.N, case.P, COMPS, MERGED, 7 + case.P)


def _wanted(case):
    return WANTED | ({("skipped", False)} if case.full else set())


def restated(case, seed, steps):
    """[(kind, accepted)] of the case's moves by the host restatement alone"""
    X, z1 = _start(case)
    z, K, maxK, seen = z1.astype(np.int64) - 1, LABELS, _max_k(case), []
    lp = al.poisson_prior(maxK)
    for m in range(steps):
        if case.target == "dp":  # (the device chain has made one sweep before the labels are planted: moves of sweep 2)
            r = sm_ref.move(X, z, maxK, ALPHA, BETA, GAMMA, case.scans, sm_ref.PhiloxDraws(seed, 2, m), diagnostics=False)
        else:
            r = as_ref.move(X, z, K, maxK, A, BETA, GAMMA, lp, case.scans, as_ref.PhiloxDraws(seed, 1, m), diagnostics=False)
            K = r["K"]
        z = r["z"]
        seen.append((r["kind"], bool(r["accepted"])))
    return seen


def choose(case, budget=60, seeds=range(17, 600)):
    for seed in seeds:
        seen = restated(case, seed, budget)
        for n in range(1, budget + 1):
            if _wanted(case) <= set(seen[:n]):
                return seed, n
    raise AssertionError("no seed reaches the coverage of " + case.name)


def observe_moves(bmm, case):
    X, z1 = _start(case)
    maxK = _max_k(case)
    dp = case.target == "dp"
    if dp:
        c = bmm.Chain("dp", case.N, case.P, maxK, alpha=ALPHA, beta=BETA, gamma=GAMMA, batch=256, seed=case.seed)
    else:
        c = bmm.Chain("collapsed", case.N, case.P, maxK, alpha=A, beta=BETA, gamma=GAMMA, seed=case.seed)
    with c:
        c.set_data(X)
        if dp:
            c.sweeps(1)
            c.set_labels(z1)
            c.set_split_merge(1, case.scans)  # the scans of the manual moves ...
            c.set_split_merge(0, case.scans)  # ... and nothing armed
        else:
            c.set_initial_labels(z1)
            c.set_alloc("poisson", 0)
            c.set_k(LABELS)
            c.set_alloc_split_merge(0, case.scans)
        records = []
        for _ in range(case.steps):
            d = c.split_merge_step(sides=True) if dp else c.alloc_split_merge_step(sides=True)
            rec = [_bits(d[f]) if isinstance(d[f], float) else d[f] for f in (MOVE_FIELDS if dp else ALLOC_FIELDS)]
            records.append(json.loads(json.dumps(rec)) + [_sha(d["launch_side"]), _sha(d["proposal_side"])])
        Nk, S = c.counts()
        st = c.split_merge_stats() if dp else c.alloc_split_merge_stats()
        return {"records": records, "z": _sha(c.labels()), "Nk": [int(v) for v in Nk], "S": _sha(S),
                "K": int((Nk > 0).sum()) if dp else c.k(), "counters": [int(v) for v in st.values()]}


# ------------------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def bmm():
    import importlib
    return importlib.import_module("bmm_mcmc_amd")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", [c.name for c in TABLE_CASES])
def test_table_build_writes_the_bytes_of_the_separate_kernels(bmm, golden, dbg_lib, name):
    case = next(c for c in TABLE_CASES if c.name == name)
    got = observe_table(bmm, case, lambda k, v: dbg_lib.delenv(k, raising=False) if v is None else dbg_lib.setenv(k, v))
    assert got == golden["tables"][name]


@pytest.mark.parametrize("name", [c.name for c in MOVE_CASES])
def test_moves_write_the_bytes_of_the_separate_kernels(bmm, golden, name):
    case = next(c for c in MOVE_CASES if c.name == name)
    want = golden["moves"][name]
    # the golden itself holds what the case is there for
    kind, accepted = MOVE_FIELDS.index("kind"), MOVE_FIELDS.index("accepted")
    assert _wanted(case) <= {(r[kind], r[accepted]) for r in want["records"]}, name
    assert len(want["records"]) == case.steps <= 60
    got = observe_moves(bmm, case)
    for m, (g, w) in enumerate(zip(got["records"], want["records"])):
        assert g == w, (name, m)
    assert got == want


def test_the_golden_holds_every_case(golden):
    assert sorted(golden["tables"]) == sorted(c.name for c in TABLE_CASES)
    assert sorted(golden["moves"]) == sorted(c.name for c in MOVE_CASES)
    assert sum(c.full for c in MOVE_CASES if c.target == "dp") == 1 and sum(c.full for c in MOVE_CASES if c.target == "alloc") == 1


def record(path):
    """write the golden from the libraries of this tree"""
    import importlib
    bmm = importlib.import_module("bmm_mcmc_amd")
    from bmm_mcmc_amd import _capi, build
    out = {"moves": {c.name: observe_moves(bmm, c) for c in MOVE_CASES}, "tables": {}}
    if build.stale(build.LIB_DBG):
        build.build(debug_variant=True)
    _capi._LIB = _capi.load(build.LIB_DBG)

    def setenv(k, v):
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    for c in TABLE_CASES:
        out["tables"][c.name] = observe_table(bmm, c, setenv)
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    if sys.argv[1] == "--seeds":
        for mc in MOVE_CASES:
            print('    "%s": %r,' % (mc.name, choose(mc)), flush=True)
    elif sys.argv[1] == "--record":
        record(sys.argv[2])
