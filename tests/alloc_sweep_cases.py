"""The shapes at which tests/test_gpu_alloc_sweep.py holds the allocation sampler's sweep (k_count_tables<TAB_ALLOC> and the
resample kernels behind it) to the oracle chain oracle.alloc bit for bit, and what each of them is there to reach.

A label's weight shows in the drawn labels only when it is not negligible, so the data make empty labels and rows that
sit alone compete: crisp planted components (every feature's rate 0.1 or 0.9), labelled by component, and a few
coin-flip rows (rate 0.5 on every feature) at the first row, the last row and the batch and chunk edges, seated alone
or in pairs on otherwise unused open labels, with at least one open label left empty and, where K_open < maxK, at
least one label closed.  A coin-flip row fits no crisp component, so it chooses among the empty labels, its own and
those of the other loners: exactly the weights under test.  Weights that all of these share cancel in the draw, so
most cases also seat a crowd of coin-flip rows together on one more label: its rates are near 0.5, a coin-flip row
fits it about as well as the prior, and an occupied label's tables then compete with the empty labels' in one draw.

The chain is a pure function of (data, labels, seed), so the oracle alone (tests/test_oracle_alloc.py, on the CPU)
shows that a case's seed reaches what the case is for before the device is asked."""
import collections
import functools

import numpy as np

# -------------------------------------------------------------------------------------------------- content cases
# comps crisp components on labels 1..comps; `loners` further labels hold the coin-flip rows, `per` (1 or 2) to a
# label; loners = 0 seats the coin-flip rows with component 1 (K_open <= 2 leaves no label for them); `crowd` more
# coin-flip rows sit together on the label after those (about P / 10 of them: a row's fit to a crowd of m falls short of
# the prior by about P / (4 m) nats, which its weight m / a makes up for).
# reach: "hop" = the counts of check_reached; "closed" = no row ever on a closed label (every K_open < maxK case).
Content = collections.namedtuple("Content", "name N P maxK K_open a beta gamma batch sweeps comps loners per coins crowd seed reach")

# The seed: 17 was tried first at every shape; where the oracle's chain did not reach what the case is for with it, the
# next seeds were tried in order and the first that does is recorded here with the reason.
CONTENT = [
    # one feature leaves room for two clusters only, which then hold nearly every row, and a row that sits alone keeps its
    # label about once in (rows in its pattern's cluster) / a turns; so the one-feature case spreads its 80 rows over
    # 64 open labels, where a / (n + a) is not small
    Content("P1-all-64-labels-open", 80, 1, 64, 64, 3.0, 0.5, 0.5, 80, 100, 3, 4, 1, 4, 0, 17, ("hop",)),
    # K_open = 1: every weight but one is a closed label's; nothing can hop, so the case is held to "closed" alone
    Content("P33-one-open", 80, 33, 6, 1, 1.0, 0.5, 0.5, 64, 40, 1, 0, 1, 4, 0, 17, ("closed",)),
    # K_open = 2: one component and one empty label that fills and empties again (no label is left for loners); five
    # features and a small a, so that a coin-flip row weighs a * prior on label 2, alone or not yet there, against
    # 79 * a poor fit on label 1
    Content("P5-two-open", 80, 5, 13, 2, 0.25, 0.5, 0.5, 1, 100, 1, 0, 1, 5, 0, 17, ("hop", "closed")),
    Content("P6-one-past-a-group", 80, 6, 4, 3, 3.0, 0.5, 1.5, 1, 100, 1, 1, 2, 2, 0, 17, ("hop", "closed")),
    # (seed 17: 14 born, 16 loners left; 18 is the next seed: 28 and 22)
    Content("P32-full-word", 200, 32, 6, 5, 1.0, 0.5, 0.5, 64, 60, 1, 2, 1, 2, 6, 18, ("hop", "closed")),
    Content("P33-padding-labels", 300, 33, 13, 12, 0.25, 0.5, 0.5, 300, 60, 3, 3, 2, 6, 6, 17, ("hop", "closed")),
    Content("P120-one-trip", 300, 120, 13, 13, 0.25, 0.5, 0.5, 64, 60, 3, 4, 1, 4, 12, 17, ("hop",)),
    # (seeds 17 and 18: three loners kept their label; 19: seven)
    Content("P121-second-trip", 600, 121, 13, 13, 1.0, 1.5, 0.5, 64, 40, 2, 4, 2, 8, 12, 19, ("hop",)),
    Content("P128-width-4-tier-2", 300, 128, 64, 63, 0.25, 0.5, 0.5, 300, 60, 4, 6, 1, 6, 12, 17, ("hop", "closed")),
    Content("P130-generic", 300, 130, 13, 12, 1.0, 0.5, 0.5, 300, 60, 3, 4, 1, 4, 12, 17, ("hop", "closed")),
    Content("P241-generic-three-trips", 200, 241, 6, 6, 3.0, 0.5, 0.5, 1, 60, 1, 2, 1, 2, 60, 17, ("hop",)),
    # (seed 17: 19 loners left; 18: 27)
    Content("P1024-generic-widest", 200, 1024, 6, 5, 1.0, 0.5, 0.5, 64, 60, 1, 2, 1, 2, 100, 18, ("hop", "closed")),
]
CONTENT_BY_NAME = {c.name: c for c in CONTENT}

MIN_BORN, MIN_KEPT, MIN_LEFT = 20, 5, 20          # content cases
MIN_FORM_BORN, MIN_FORM_LEFT = 10, 5              # form cases


def coin_rows(N, batch, n):
    """where the coin-flip rows go: the first row, the last, then both sides of every batch and 64-row chunk edge"""
    rows = [0, N - 1]
    for edge in sorted({e for e in range(batch, N, batch)} | {e for e in range(64, N, 64)}):
        rows += [edge - 1, edge]
    out = []
    for r in rows:
        if 0 <= r < N and r not in out:
            out.append(r)
    return out[:n]


def planted(N, P, comps, loners, per, coins, batch, data_seed, crowd=0):
    """X (N x P int32, column-major) and the 1-based starting labels"""
    rng = np.random.default_rng(data_seed)
    rates = np.where(rng.random((comps, P)) < 0.5, 0.1, 0.9)
    comp = rng.integers(comps, size=N)
    X = (rng.random((N, P)) < rates[comp]).astype(np.int32)
    z = (comp + 1).astype(np.int32)
    rows = coin_rows(N, batch, coins)
    assert loners == 0 or len(rows) <= loners * per
    for q, r in enumerate(rows):
        X[r] = rng.random(P) < 0.5
        z[r] = comps + 1 + q // per if loners else 1
    others = [r for r in range(N) if r not in rows]
    for r in others[1:: max(1, len(others) // max(crowd, 1))][:crowd]:   # the crowd, spread over the rows
        X[r] = rng.random(P) < 0.5
        z[r] = comps + loners + 1
    return np.asfortranarray(X), z


@functools.lru_cache(maxsize=None)
def content_start(name):
    c = CONTENT_BY_NAME[name]
    # an open label is left empty
    assert c.comps + c.loners + (1 if c.crowd else 0) + (1 if c.K_open > 1 else 0) <= c.K_open <= c.maxK
    return planted(c.N, c.P, c.comps, c.loners, c.per, c.coins, c.batch, 5, c.crowd)


# -------------------------------------------------------------------------------------------------- form cases
# Every family of k_resample an armed chain can select, at the collapsed shapes of tests/test_gpu_chunks.py's SHAPES for
# the tiers (1, 5), (1, 4) and (2, 4) on bit planes -- with (4, 100) for its (3, 100), since three labels leave too
# little room for what check_reached asks, and with (15, 96) and (30, 50), its DP shapes of 16 and 32 accumulators,
# which are the smallest two-lane form and the largest stepped-down one.  An armed chain never selects the table-building workgroups
# (SELF), the emitting twins (the hand-off is refused) or the int32 layout (refused).  env: the test variant's
# switches; loops: at least two chunks per wave on the full-size launches; generic: P above 128.
Form = collections.namedtuple("Form", "name family N P maxK K_open a batch env loops tier W seed")

FORM_SWEEPS = 4
KKT = (4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 52, 56, 64)


def kt_of(K):
    return next(kt for kt in KKT if kt >= K)


def _forms():
    out = []

    def add(family, N, P, maxK, K_open, a, batch, env, loops, tier, W, seed=17):
        out.append(Form(f"{family}-t{tier}w{W}-K{maxK}of{K_open}-P{P}", family, N, P, maxK, K_open, a, batch, env, loops, tier, W, seed))
    # one lane, default size, one CU: 4500 rows are 71 chunks for at most two workgroups.  Per (tier, width) the
    # smallest, a middle and the largest accumulator count of the collapsed shapes (4 accumulators: maxK = 4, see
    # form_start)
    for (tier, W), shapes in {(1, 5): [(4, 100), (27, 70), (64, 30)], (1, 4): [(14, 127), (30, 70), (55, 40)],
                              (2, 4): [(28, 100), (40, 80), (60, 50)]}.items():
        for q, (K, P) in enumerate(shapes):
            add("default", 10_000, P, K, K if q == 1 or K == 4 else K - 1, 4.0 if K == 4 else 1.0, 4_500, {"CUS": 1, "NOSPLIT": kt_of(K) > 32}, True, tier, W)
    # two lanes per observation: always above 32 accumulators, from 16 on short launches (SPLIT here)
    for q, (tier, W, K, P) in enumerate([(1, 5, 15, 96), (1, 5, 20, 100), (1, 5, 37, 50), (1, 5, 64, 30), (1, 4, 45, 45), (1, 4, 55, 40)]):
        add("two-lane", 10_000, P, K, K - 2 if q % 2 == 0 else K, 1.0, 4_500, {"CUS": 1, "SPLIT": kt_of(K) <= 32}, True, tier, W)
    # the stepped-down workgroups: 3000 rows on 4 CUs -> 768 threads (up to 20 accumulators), on 6 CUs -> 512 (up to 32).
    # The seed: 17 was tried first everywhere, then the next in order; where another is recorded, the oracle's counts
    # (born, loners that left) with the seeds before it are given.
    # four labels, 3000 rows, one batch (the same chain for the three families): 17 (20, 3), 18 (11, 4), 19 (17, 4): fewer
    # than five loners left; 20 (15, 5)
    K4_SEED = 20
    for K, K_open, P, seed in ((4, 4, 100, K4_SEED), (11, 10, 128, 17), (20, 19, 100, 17)):
        add("step-down-768", 3_000, P, K, K_open, 3.0 if K == 4 else 1.0, 3_000, {"CUS": 4, "NOSPLIT": kt_of(K) >= 16}, False, 1, 5, seed)
    for K, K_open, P, seed in ((4, 4, 100, K4_SEED), (20, 20, 100, 17), (30, 29, 50, 17)):
        add("step-down-512", 3_000, P, K, K_open, 3.0 if K == 4 else 1.0, 3_000, {"CUS": 6, "NOSPLIT": kt_of(K) >= 16}, False, 1, 5, seed)
    # 256 threads: fewer tiles than CUs, tables small enough for four per CU: P = 2, or four labels (at P = 2 four labels
    # settle on the four row patterns and nothing is born after that)
    for K, K_open, P, seed in ((4, 4, 100, K4_SEED), (12, 10, 2, 17), (27, 25, 2, 17), (55, 52, 2, 17)):
        add("256", 3_000, P, K, K_open, 3.0 if K == 4 else 1.0, 3_000, {"CUS": 64, "NOSPLIT": True, "NOSELF": True}, False, 1, 5, seed)
    # the generic kernel: P above 128, no LDS image, the narrow groups, own-cluster tables in global memory
    for K, K_open, P in ((4, 4, 130), (20, 19, 200), (64, 60, 300)):
        add("generic", 3_000, P, K, K_open, 3.0 if K == 4 else 1.0, 1_000, {}, False, 2, 4)
    return out


FORMS = _forms()
FORM_BY_NAME = {c.name: c for c in FORMS}


def spread(N, n, batch):
    """n rows spread over the whole range, the first and the last row and both sides of the first batch edge among them"""
    rows = [0, N - 1] + ([batch - 1, batch] if batch < N else [])
    rows += [int(r) for r in np.linspace(0, N - 1, max(n, 2)).round()]
    out = []
    for r in rows:
        if r not in out:
            out.append(r)
    return out[:n]


@functools.lru_cache(maxsize=None)
def form_start(name):
    """Four sweeps are few, so the start is arranged for them.  With a dozen open labels or more: crisp components on the
    first labels, coin-flip rows alone on half of the others, a crowd of them on one more, the rest empty, and eight
    more coin-flip rows seated with component 1, which the first sweep sends into empty labels.  With fewer labels, or at P = 2, where two features
    carry no signal: every row a coin flip, all on label 1 but for single rows on some of the other labels; a row is then
    drawn into an empty label with probability about a / N, and one that sits alone joins the crowd at its next turn."""
    c = FORM_BY_NAME[name]
    free = c.K_open - 1
    if c.P == 2 or c.maxK <= 4:
        rng = np.random.default_rng(5)
        X = (rng.random((c.N, c.P)) < 0.5).astype(np.int32)
        z = np.ones(c.N, dtype=np.int32)
        for q, r in enumerate(spread(c.N, min(free - 1, 6), c.batch)):
            z[r] = 2 + q
        return np.asfortranarray(X), z
    comps = max(1, min(4, free // 4))
    loners = min((free - comps) // 2, 24)
    rng = np.random.default_rng(5)
    rates = np.where(rng.random((comps, c.P)) < 0.5, 0.1, 0.9)
    comp = rng.integers(comps, size=c.N)
    X = (rng.random((c.N, c.P)) < rates[comp]).astype(np.int32)
    z = (comp + 1).astype(np.int32)
    rows = spread(c.N, loners + 8, c.batch)
    for q, r in enumerate(rows):
        X[r] = rng.random(c.P) < 0.5
        z[r] = comps + 1 + q if q < loners else 1
    # and a crowd of coin-flip rows together on the next label: an occupied label that a coin-flip row fits about as
    # well as the prior, so that its tables and the empty labels' compete in one draw (see the content cases)
    others = [r for r in range(c.N) if r not in rows]
    crowd = max(8, c.P // 8)
    for r in others[1:: len(others) // crowd][:crowd]:
        X[r] = rng.random(c.P) < 0.5
        z[r] = comps + loners + 1
    return np.asfortranarray(X), z


# -------------------------------------------------------------------------------------------------- what a chain reached
def batches(N, batch):
    return [(lo, min(N, lo + batch)) for lo in range(0, N, batch)]


def events(z, batch, maxK):
    """z: the oracle's trace, row 0 the starting labels (1-based).  Against the statistics frozen at every batch's start:
    born = rows drawn into a label that was empty then, as (sweep, batch start, row); kept / left = rows that sat alone
    then and kept / gave up their label; retaken = a label seen occupied, then empty, then occupied again."""
    z = np.asarray(z) - 1
    S, N = z.shape
    nk = np.bincount(z[0], minlength=maxK)
    born, kept, left = [], 0, 0
    was_emptied = np.zeros(maxK, dtype=bool)
    seen = nk > 0
    retaken = False
    for j in range(1, S):
        for lo, hi in batches(N, batch):
            old, new = z[j - 1, lo:hi], z[j, lo:hi]
            into_empty = nk[new] == 0
            born += [(j, lo, lo + int(r)) for r in np.flatnonzero(into_empty)]
            alone = nk[old] == 1
            kept += int((alone & (new == old)).sum())
            left += int((alone & (new != old)).sum())
            nk = nk - np.bincount(old, minlength=maxK) + np.bincount(new, minlength=maxK)
            was_emptied |= seen & (nk == 0)
            retaken = retaken or bool((was_emptied & (nk > 0)).any())
            seen |= nk > 0
    return {"born": born, "kept": kept, "left": left, "retaken": retaken}


def workgroup_of(row, lo, hi, geometry):
    """the workgroup that draws `row` in the launch [lo, hi).  geometry = (threads, grid_max, lanes) of k_resample: chunks
    of 64 / lanes rows, workgroup b owning chunks [b cpw, (b + 1) cpw); lanes = 0 stands for k_resample_generic, whose
    threads stride over the launch by the whole grid"""
    threads, grid_max, lanes = geometry
    if lanes == 0:
        return ((row - lo) // threads) % min(-(-(hi - lo) // threads), grid_max)
    ow = 64 // lanes
    nchunks = -(-(hi - lo) // ow)
    grid = min(-(-(hi - lo) // (threads // lanes)), grid_max)
    cpw = -(-nchunks // grid)
    return ((row - lo) // ow) // cpw


def births_span_workgroups(born, N, batch, geometry=None):
    """births in at least two workgroups' ranges of one launch.  Without a device the geometry is unknown: then two births
    of one launch further apart than half the launch plus a chunk, which no split into two or more contiguous ranges
    of whole chunks, the first ones equal, keeps in one range."""
    per = collections.defaultdict(list)
    for j, lo, r in born:
        per[(j, lo)].append(r)
    for (j, lo), rows in per.items():
        hi = min(N, lo + batch)
        if geometry is None:
            if max(rows) - min(rows) >= (hi - lo + 1) // 2 + 64:
                return True
        elif len({workgroup_of(r, lo, hi, geometry) for r in rows}) >= 2:
            return True
    return False


def check_reached(case, z, geometry=None):
    """Conditions, not measurements, counted on the oracle's own chain.  Returns the counts for the record."""
    ev = events(z, case.batch, case.maxK)
    counts = {"born": len(ev["born"]), "kept": ev["kept"], "left": ev["left"]}
    if isinstance(case, Content):
        if "hop" in case.reach:
            assert counts["born"] >= MIN_BORN and counts["kept"] >= MIN_KEPT and counts["left"] >= MIN_LEFT, (case.name, counts)
            assert ev["retaken"], case.name
        if case.K_open < case.maxK:
            assert "closed" in case.reach and np.asarray(z).max() <= case.K_open, case.name
    else:
        assert counts["born"] >= MIN_FORM_BORN and counts["left"] >= MIN_FORM_LEFT, (case.name, counts)
        assert births_span_workgroups(ev["born"], case.N, case.batch, geometry), case.name
        assert np.asarray(z).max() <= case.K_open, case.name
    return counts


# -------------------------------------------------------------------------------------------------- K changing under the sweeps
# One resident chain, two batches per sweep: set_k down to the highest occupied label, a sweep, set_k up by two, a
# sweep, and so on.  Three crisp components, two coin-flip rows alone on labels 4 and 5 and eight more seated with
# component 1; armed, the chain has K = maxK = 8, so the very first sweep follows a set_k.
K_N, K_P, K_MAXK, K_BATCH, K_A, K_SEED, K_SWEEPS = 2500, 33, 8, 1250, 1.0, 17, 6


@functools.lru_cache(maxsize=None)
def k_start():
    rng = np.random.default_rng(5)
    rates = np.where(rng.random((3, K_P)) < 0.5, 0.1, 0.9)
    comp = rng.integers(3, size=K_N)
    X = (rng.random((K_N, K_P)) < rates[comp]).astype(np.int32)
    z = (comp + 1).astype(np.int32)
    for q, r in enumerate(spread(K_N, 10, K_BATCH)):
        X[r] = rng.random(K_P) < 0.5
        z[r] = 4 + q if q < 2 else 1
    return np.asfortranarray(X), z


def k_schedule(step, labels, K_now):
    """the K to set ahead of sweep `step` (0-based): down to the highest occupied label, then up by two, in turn"""
    return int(np.max(labels)) if step % 2 == 0 else min(K_MAXK, K_now + 2)


def k_reached(Ks, zs):
    """Ks: the K of every sweep; zs: the labels before the first sweep and after each.  The first sweep ran below maxK (the
    step down from the armed chain's maxK closes labels), K went up at least twice after that, and rows were drawn into
    labels that a step up had just opened"""
    assert Ks[0] < K_MAXK and sum(b > a for a, b in zip(Ks, Ks[1:])) >= 2, Ks
    opened = 0
    for j in range(1, len(Ks)):
        if Ks[j] > Ks[j - 1]:
            opened += int((np.asarray(zs[j + 1]) > Ks[j - 1]).sum())
    assert opened >= 5, (Ks, opened)
    return opened


# -------------------------------------------------------------------------------------------------- moves between the sweeps
# The cases many-rows, empties and K-is-1 of tests/alloc_cases.py: 40 rounds of one move, then one sweep.  A move ahead of
# sweep j is keyed (seed, j, 0).  The batch: three launches, the last one short, for the 2500 rows; one for the others.
# Whether a case's moves are accepted is the seed's doing: "empties" is the one that must reach both kinds.
MOVE_CASES = {"many-rows": 1000, "empties": 40, "K-is-1": 300}
MOVE_REACH = ("empties",)
MOVE_ROUNDS = 40


def moves_reached(seen):
    """seen: per round (kind, accepted, j2 (0-based), k_before): an accepted eject and an accepted absorb whose freed
    label is not the last, so that the last label's rows, Nk and S move into it, each directly ahead of a compared sweep"""
    assert any(kind == "eject" and acc for kind, acc, _, _ in seen)
    assert any(kind == "absorb" and acc and j2 != kb - 1 for kind, acc, j2, kb in seen)
