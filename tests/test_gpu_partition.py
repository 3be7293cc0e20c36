"""Clustering point estimate and posterior similarity on the device (include/bmm_mcmc.h), held
to the NumPy restatement tests/partition_ref.py: Binder bit-exact in every form of the kernels (the cases are
partition_ref.CASES; tests/test_partition_cpu.py proves they reach every form), VI within the bound derived from the
arithmetic, the similarity counts exact and tied to the Binder totals by Dahl's identity, the summary of a run equal
to the stand-alone call on what the run returns, and the minimiser where a theorem puts it."""
import numpy as np
import pytest

import bmm_mcmc_amd as bm
import partition_ref as ref
from util import synth

pytestmark = pytest.mark.gpu


def _ids():
    return ["K%d-N%d-S%d-st%d-%s-%s" % (c[0], c[1], c[2], c[3], c[4], "skew" if c[5] else "unif") for c in ref.CASES]


@pytest.mark.parametrize("Kc,N,S,stride,crit,skewed", ref.CASES, ids=_ids())
def test_every_form_against_the_restatement(Kc, N, S, stride, crit, skewed):
    z = ref.make_rows(Kc, N, S, skewed, 1000 + Kc + S)
    got = bm.partition_distances(z, crit, stride, distances=True, Kc=Kc)
    C = -(-S // stride)
    assert got["loss"].shape == (C,) and got["distances"].shape == (C, S) and got["n_used"] == S
    DB = ref.distances(z, Kc, "binder", stride)
    tot = ref.binder2_totals(z, Kc, stride, DB)
    # Binder: exact, under either criterion
    assert [int(x) for x in got["binder2"]] == tot
    if crit == "binder":
        assert np.array_equal(got["distances"], DB.astype(np.float64))
        assert all(int(got["distances"][c, t]) == DB[c, t] for c in range(C) for t in range(S))
        assert np.array_equal(got["loss"], ref.expected_loss(z, Kc, "binder", stride, DB))
        assert got["best"] == ref.point_estimate(z, Kc, "binder", stride, DB)
    else:
        DV = ref.distances(z, Kc, "vi", stride)
        want = ref.expected_loss(z, Kc, "vi", stride, DV)
        bound = ref.vi_bound(Kc, N)
        err_d = float(np.abs(got["distances"] - DV).max())
        err_l = float(np.abs(got["loss"] - want).max())
        print("VI K=%d N=%d S=%d: max |dist - ref| = %.3g, max |loss - ref| = %.3g, bound %.3g" % (Kc, N, S, err_d, err_l, bound))
        assert err_d <= bound and err_l <= bound
        assert got["best"] % stride == 0 and want[got["best"] // stride] <= want.min() + bound
        for c in range(C):
            assert got["distances"][c, c * stride] == 0.0
        again = bm.partition_distances(z, crit, stride, distances=True, Kc=Kc)
        assert np.array_equal(again["distances"], got["distances"]) and np.array_equal(again["loss"], got["loss"])
        assert again["best"] == got["best"]
    assert np.array_equal(got["z"], z[got["best"]])


@pytest.mark.parametrize("crit", ["binder", "vi"])
def test_identical_rows_and_ties(crit):
    rng = np.random.default_rng(3)
    a, b = rng.integers(1, 4, 777), rng.integers(1, 4, 777)
    perm = np.array([3, 1, 2])
    z = np.asfortranarray(np.stack([a, b, perm[a - 1], b, a]), dtype=np.int32)  # row 2 is row 0 renumbered
    got = bm.partition_distances(z, crit, distances=True, Kc=3)
    D = got["distances"]
    for i, j in ((0, 2), (0, 4), (2, 4), (1, 3)):
        assert D[i, j] == 0.0 and D[j, i] == 0.0
    assert D[0, 1] > 0 and got["loss"][0] == got["loss"][4]
    assert got["best"] == 0                       # rows 0, 2, 4 tie: the lowest wins
    z = np.asfortranarray(np.stack([b, a, b, a]), dtype=np.int32)   # everything ties
    assert bm.partition_distances(z, crit, Kc=3)["best"] == 0
    assert bm.partition_distances(z, crit, stride=3, Kc=3)["best"] == 0
    z = np.asfortranarray(np.stack([b, a, a, b, a]), dtype=np.int32)  # a is the minimiser: rows 1, 2, 4
    assert bm.partition_distances(z, crit, Kc=3)["best"] == 1
    assert bm.partition_distances(z, crit, stride=2, Kc=3)["best"] == 2   # candidates 0, 2, 4


@pytest.mark.parametrize("crit", ["binder", "vi"])
@pytest.mark.parametrize("S,copies", [(9, [4, 5, 6, 7, 8]), (200, None)])
def test_the_majority_partition_is_the_point_estimate(crit, S, copies):
    """Both distances are metrics: when more than half of the rows are one partition r, the lowest-indexed copy of
    r has the smallest expected loss whatever the other rows are."""
    rng = np.random.default_rng(40 + S)
    N, Kc = 2000, 5
    z = ref.make_rows(Kc, N, S, True, 77 + S)
    z[::2] = ref.make_rows(Kc, N, S, False, 78 + S)[::2]  # the others: skewed and uniform rows
    if copies is None:
        copies = sorted(rng.choice(np.arange(3, S), size=101, replace=False).tolist())
    r = rng.integers(1, Kc + 1, N).astype(np.int32)
    z[copies] = r
    got = bm.partition_distances(np.asfortranarray(z), crit, Kc=Kc)
    assert got["best"] == copies[0]


@pytest.mark.parametrize("M", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("Kc", [7, 300])
def test_similarity_counts(M, Kc):
    S, N = 17, 1200
    z = ref.make_rows(Kc, N, S, Kc == 7, 5 + M)
    idx = np.random.default_rng(M).integers(0, N, M)   # unsorted, with repeats once M is large
    if M >= 63:
        idx[5] = idx[60]
    got = bm.posterior_similarity(z, idx)
    assert got.dtype == np.uint32 and np.array_equal(got, ref.similarity(z, idx))


def test_similarity_and_binder_totals_check_each_other():
    """M = N = 300, idx = arange: Dahl's identity, exactly, between bmm_device_psm and binder2_out"""
    S, N, Kc = 17, 300, 6
    z = ref.make_rows(Kc, N, S, False, 9)
    cnt = bm.posterior_similarity(z, np.arange(N))
    b2 = bm.partition_distances(z, "binder", Kc=Kc)["binder2"]
    up = [int(x) for x in cnt[np.triu_indices(N, 1)]]
    sq, sm = sum(x * x for x in up), sum(up)
    for c in range(S):
        assert ref.dahl_least_squares(z[c], cnt, S) == S * (int(b2[c]) // 2) + sq - S * sm


def _data(N=600, P=8, K=3, seed=21):
    return synth(N, P, K, seed)[0]


def _same_summary(p, q):
    assert p["best"] == q["best"] and p["n_used"] == q["n_used"]
    assert np.array_equal(p["loss"], q["loss"]) and np.array_equal(p["binder2"], q["binder2"])
    assert np.array_equal(p["z"], q["z"])


SAMPLERS = [("collapsed", lambda X, **kw: bm.gibbs_collapsed(X, 14, 3, burnin=4, seed=5, **kw), 3),
            ("dp", lambda X, **kw: bm.gibbs_dp(X, 14, burnin=4, seed=5, maxK=10, **kw), 10),
            ("sb", lambda X, **kw: bm.gibbs_stickbreaking(X, 14, 4, burnin=4, seed=5, **kw), 4),
            ("full", lambda X, **kw: bm.gibbs_full(X, 14, 3, burnin=4, seed=5, **kw), 3)]


@pytest.mark.parametrize("name,run,Kc", SAMPLERS, ids=[s[0] for s in SAMPLERS])
@pytest.mark.parametrize("crit", ["binder", "vi"])
def test_through_a_run(name, run, Kc, crit):
    X = _data()
    idx = [5, 0, 17, 5, 599]
    plain = run(X)
    got = run(X, partition=crit, partition_stride=2, similarity_of=idx)
    for k in ("z", "theta", "alpha", "pi"):
        if k in plain:
            assert np.array_equal(plain[k], got[k], equal_nan=True), k
    assert "partition" not in plain
    p = got["partition"]
    S = got["z"].shape[0]
    assert p["n_used"] == S and p["criterion"] == crit and np.array_equal(p["z"], got["z"][p["best"]])
    _same_summary(p, bm.partition_distances(got["z"], crit, 2, Kc=Kc))
    assert np.array_equal(p["similarity"], bm.posterior_similarity(got["z"], idx))
    assert np.array_equal(p["similarity"], ref.similarity(got["z"], idx))


def test_dp_without_burnin_leaves_the_unassigned_row_out():
    X = _data()
    plain = bm.gibbs_dp(X, 9, burnin=0, seed=6, maxK=10)
    got = bm.gibbs_dp(X, 9, burnin=0, seed=6, maxK=10, partition="binder", similarity_of=[1, 2, 3])
    assert np.array_equal(plain["z"], got["z"]) and np.all(got["z"][0] == bm.NA_INTEGER)
    p = got["partition"]
    S = got["z"].shape[0]
    assert p["n_used"] == S - 1 and p["loss"].shape == (S - 1,)
    q = bm.partition_distances(got["z"][1:], "binder", Kc=10)
    assert p["best"] == q["best"] + 1 and np.array_equal(p["loss"], q["loss"]) and np.array_equal(p["binder2"], q["binder2"])
    assert np.array_equal(p["z"], got["z"][p["best"]])
    assert np.array_equal(p["similarity"], ref.similarity(got["z"][1:], [1, 2, 3]))
    # the finite collapsed sampler's row 0 is the initial allocation, a partition: it is used
    got = bm.gibbs_collapsed(X, 9, 3, burnin=0, seed=6, partition="vi")
    assert got["partition"]["n_used"] == got["z"].shape[0]
    _same_summary(got["partition"], bm.partition_distances(got["z"], "vi", Kc=3))


@pytest.mark.parametrize("name", ["sb", "full"])
def test_explicit_samplers_without_burnin_leave_the_unassigned_row_out(name):
    X = _data()
    fn = bm.gibbs_stickbreaking if name == "sb" else bm.gibbs_full
    plain = fn(X, 9, 4, burnin=0, seed=6)
    got = fn(X, 9, 4, burnin=0, seed=6, partition="vi", partition_stride=3, similarity_of=[4, 4, 9])
    for k in ("z", "theta", "alpha", "pi"):
        assert np.array_equal(plain[k], got[k], equal_nan=True), k
    assert np.all(got["z"][0] == bm.NA_INTEGER)
    p = got["partition"]
    S = got["z"].shape[0]
    assert p["n_used"] == S - 1 and p["loss"].shape == (-(-(S - 1) // 3),)
    q = bm.partition_distances(got["z"][1:], "vi", 3, Kc=4)
    assert p["best"] == q["best"] + 1 and np.array_equal(p["loss"], q["loss"]) and np.array_equal(p["binder2"], q["binder2"])
    assert np.array_equal(p["z"], got["z"][p["best"]])
    assert np.array_equal(p["similarity"], ref.similarity(got["z"][1:], [4, 4, 9]))


def test_stickbreaking_with_newdata_and_with_device_relabelling():
    X = _data()
    Xnew = _data(50, seed=22)
    kw = dict(burnin=10, seed=8, newdata=Xnew, relabel=True, stephens="device", burnrelabel=5)
    base = bm.gibbs_stickbreaking(X, 30, 4, **kw)
    got = bm.gibbs_stickbreaking(X, 30, 4, partition="vi", **kw)
    for k in ("z", "theta", "alpha", "pi", "z_original", "permutations"):
        assert np.array_equal(base[k], got[k], equal_nan=True), k
    assert np.array_equal(base["predictive"]["lppd"], got["predictive"]["lppd"])
    p = got["partition"]
    _same_summary(p, bm.partition_distances(got["z_original"], "vi", Kc=4))
    assert np.array_equal(p["z"], got["z_original"][p["best"]])


def test_with_newdata_and_with_device_relabelling():
    X = _data()
    Xnew = _data(50, seed=22)
    base = bm.gibbs_collapsed(X, 30, 3, burnin=10, seed=8, newdata=Xnew, relabel=True, stephens="device")
    got = bm.gibbs_collapsed(X, 30, 3, burnin=10, seed=8, newdata=Xnew, relabel=True, stephens="device", partition="binder")
    for k in ("z", "theta", "alpha", "z_original", "permutations"):
        assert np.array_equal(base[k], got[k], equal_nan=True), k
    assert np.array_equal(base["predictive"]["lppd"], got["predictive"]["lppd"])
    p = got["partition"]
    _same_summary(p, bm.partition_distances(got["z_original"], "binder", Kc=3))
    assert np.array_equal(p["z"], got["z_original"][p["best"]])
    # the relabelled trace is the same partitions: the same losses
    assert np.array_equal(p["binder2"], bm.partition_distances(got["z"], "binder", Kc=3)["binder2"])


def test_two_chains_are_pooled():
    X = _data()
    plain = bm.gibbs_collapsed(X, 14, 3, burnin=4, seed=5, chains=2)
    got = bm.gibbs_collapsed(X, 14, 3, burnin=4, seed=5, chains=2, partition="binder")
    zz = np.concatenate([o["z"] for o in got], axis=0)
    assert all(np.array_equal(a["z"], b["z"]) for a, b in zip(plain, got))
    q = bm.partition_distances(zz, "binder")
    p = got[0]["partition"]
    S = got[0]["z"].shape[0]
    assert p is got[1]["partition"] and p["n_used"] == 2 * S
    assert p["chain"] * S + p["best"] == q["best"] and np.array_equal(p["binder2"], q["binder2"])
    assert np.array_equal(p["z"], got[p["chain"]]["z"][p["best"]])


def test_report_the_medoid_against_the_generating_allocation():
    """Information for DESIGN.md section 13, no assertion on the figures: on the shuffled K = 4, N = 20 000, P = 12
    mixture, started from the generating allocation, B(z_best, truth) beside the smallest, median and largest
    B(z_t, truth) of the kept sweeps."""
    N, P, K = 20000, 12, 4
    X, labels, _, _ = synth(N, P, K, 77)
    truth = (labels + 1).astype(np.int32)
    got = bm.gibbs_collapsed(X, 160, K, burnin=80, seed=11, initial_K=truth, partition="binder")
    stack = np.asfortranarray(np.concatenate([truth[None, :], got["z"]], axis=0))
    d = bm.partition_distances(stack, "binder", stride=stack.shape[0], distances=True, Kc=K)["distances"][0, 1:]
    best = got["partition"]["best"]
    print("B(z_best, truth) = %d; over the %d kept sweeps B(z_t, truth): min %d, median %d, max %d (pairs: %d)"
          % (d[best], d.size, d.min(), np.median(d), d.max(), N * (N - 1) // 2))
    assert d[best] == ref.binder(got["z"][best], truth, K)
