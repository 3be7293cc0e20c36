"""Credible ball and row-to-cluster similarity on the device (include/bmm_mcmc.h "credible ball").
Every integer -- 2 B per draw, the clusters per draw, sim -- equals the NumPy restatement tests/credible_ball_ref.py
with ==, under both criteria, on credible_ball_ref.CASES (tests/test_credible_ball_cpu.py proves through the plan that
they reach every form of the kernels a small shape can reach); the VI distances lie within partition_ref.vi_bound of
partition_ref.vi; the radius and the three bounds equal ball() of the restatement applied to the distances the device
returned.  The new numbers are held to the existing kernels too: the search's start totals and the posterior
similarity counts.  Through a run: the armed ball equals the stand-alone call on the returned trace and leaves
everything else as it was."""
import functools

import numpy as np
import pytest

import bmm_mcmc_amd as bm
import credible_ball_ref as cbr
import partition_ref as pr
from util import synth

pytestmark = pytest.mark.gpu
BOUNDS = ("horizontal", "upper", "lower")
CRITS = ("binder", "vi")


@functools.lru_cache(maxsize=None)
def _case(case):
    z, centre, subset = cbr.case_trace(case)
    for a in (z, centre, subset):
        a.setflags(write=False)
    return z, centre, subset


@functools.lru_cache(maxsize=None)
def _want(case):
    """the restatement of a case, computed once: d2 and k per draw, the VI per draw, sim of all rows"""
    Kc, Ka, N, S, _ = case
    z, centre, _ = _case(case)
    d2, _, k = cbr.distances(centre, z, max(Kc, Ka), "binder")
    vi = [pr.vi(centre, row, max(Kc, Ka)) for row in z]
    return d2, k, vi, cbr.sim(centre, z, Ka)


@functools.lru_cache(maxsize=None)
def _got(case, crit):
    Kc, Ka, N, S, _ = case
    z, centre, _ = _case(case)
    return bm.credible_ball(z, centre, crit, membership=True, Kc=Kc, max_clusters=Ka)


def _ball(opt, fn, *args, **kw):
    """fn(*args, **kw) with credible_ball=opt among the run's options"""
    with bm.run_options(credible_ball=opt):
        return fn(*args, **kw)


def _same_ball(p, q, skip=("centre",)):
    assert sorted(p) == sorted(q)
    for k in p:
        if k in skip:
            continue
        if k in BOUNDS:
            assert sorted(p[k]) == sorted(q[k]) == ["distance", "n_clusters", "sweep", "ties", "z"]
            for f in p[k]:
                assert np.array_equal(p[k][f], q[k][f]), (k, f)
        else:
            assert np.array_equal(p[k], q[k], equal_nan=k == "membership"), k


@pytest.mark.parametrize("crit", CRITS)
@pytest.mark.parametrize("case", cbr.CASES, ids=cbr.case_id)
def test_the_integers_equal_the_restatement(case, crit):
    Kc, Ka, N, S, _ = case
    z, centre, _ = _case(case)
    d2, k, vi, sim = _want(case)
    got = _got(case, crit)
    assert got["criterion"] == crit and got["level"] == 0.95 and got["n_used"] == S and got["centre"] == "given"
    assert [int(v) for v in got["binder2"]] == d2 and all(type(v) is int for v in got["binder2"])
    assert [int(v) for v in got["n_clusters"]] == k
    assert got["sim"].dtype == np.uint64 and got["sim"].shape == (N, Ka)
    assert np.array_equal(got["sim"].astype(object), sim)
    assert [int(v) for v in got["sizes"]] == [int(v) for v in np.bincount(centre - 1, minlength=Ka)]
    assert np.array_equal(got["rows"], np.arange(N))
    if crit == "binder":
        assert [float(v) for v in got["distance"]] == [v / 2 for v in d2]
    else:
        err = max(abs(float(g) - w) for g, w in zip(got["distance"], vi))
        print("vi %s: largest |distance - partition_ref.vi| = %.3g (bound %.3g)" % (cbr.case_id(case), err, pr.vi_bound(Kc, N)))
        assert err <= pr.vi_bound(Kc, N)
        assert [float(v) == 0.0 for v in got["distance"]] == [v == 0 for v in d2]
    if N <= 300:  # membership from sim, cell by cell by the restatement's loop
        assert np.array_equal(got["membership"], cbr.membership(sim, centre, S), equal_nan=True)
    own = got["membership"][np.arange(N), centre - 1]
    assert np.all((own >= 0) & (own <= 1) | np.isnan(own))
    assert np.isnan(got["membership"][:, np.asarray(got["sizes"]) == 0]).all()


@pytest.mark.parametrize("crit", CRITS)
@pytest.mark.parametrize("case", cbr.CASES, ids=cbr.case_id)
def test_the_ball_is_ball_of_the_returned_distances(case, crit):
    Kc, Ka, N, S, _ = case
    z, centre, _ = _case(case)
    for level in (0.95, 1.0, 0.5, 1e-9):
        got = _got(case, crit) if level == 0.95 else bm.credible_ball(z, centre, crit, level=level, Kc=Kc, max_clusters=Ka)
        D = [int(v) for v in got["binder2"]] if crit == "binder" else [float(v) for v in got["distance"]]
        want = cbr.ball(D, [int(v) for v in got["n_clusters"]], level)
        print("%s %s level %g: radius %.6g, %d of %d inside (m = %d), bounds %s"
              % (crit, cbr.case_id(case), level, got["radius"], got["n_in"], S, want["m"],
                 [(got[q]["sweep"], got[q]["ties"], got[q]["n_clusters"]) for q in BOUNDS]))
        assert got["radius"] == float(got["distance"][want["at"]])
        assert got["n_in"] == want["n_in"] >= want["m"]
        for q in BOUNDS:
            b = got[q]
            assert (b["sweep"], b["ties"], b["n_clusters"]) == (want[q]["sweep"], want[q]["ties"], want[q]["n_clusters"]), q
            assert b["distance"] == float(got["distance"][b["sweep"]])
            assert np.array_equal(b["z"], z[b["sweep"]]) and b["z"].dtype == np.int32
        assert got["horizontal"]["distance"] == got["radius"]
    if S == 300:  # every draw is there ten times: the radius is tied, and the centre, a draw, is at distance 0
        got = _got(case, crit)
        assert got["n_in"] > 285 and got["horizontal"]["ties"] % 10 == 0
        assert bm.credible_ball(z, centre, crit, level=1e-9, Kc=Kc)["n_in"] % 10 == 0
        assert bm.credible_ball(z, centre, crit, level=1e-9, Kc=Kc)["radius"] == 0.0


@pytest.mark.parametrize("crit", CRITS)
@pytest.mark.parametrize("case", cbr.CASES, ids=cbr.case_id)
def test_against_the_search_totals(case, crit):
    """the distances add up to what k_ps_reduce gives the search for the same centre"""
    Kc, Ka, N, S, _ = case
    z, centre, _ = _case(case)
    got = _got(case, crit)
    s = bm.partition_search(z, crit, start=centre, max_passes=1, max_clusters=Ka, Kc=Kc)
    assert sum(got["binder2"]) == s["start_binder2"]
    assert abs(float(np.mean(got["distance"])) - s["start_loss"]) <= 1e-12 * abs(s["start_loss"])


def test_against_the_posterior_similarity_counts():
    case = cbr.CASES[0]
    Kc, Ka, N, S, _ = case
    assert N == 257
    z, centre, _ = _case(case)
    cnt = bm.posterior_similarity(z, np.arange(N)).astype(np.uint64)
    for crit in CRITS:
        sim = _got(case, crit)["sim"]
        for a in range(Ka):
            assert np.array_equal(sim[:, a], cnt[:, centre == a + 1].sum(axis=1, dtype=np.uint64)), a


@pytest.mark.parametrize("crit", CRITS)
@pytest.mark.parametrize("case", cbr.CASES, ids=cbr.case_id)
def test_a_subset_equals_the_same_rows_of_the_full_result(case, crit):
    Kc, Ka, N, S, _ = case
    z, centre, subset = _case(case)
    assert subset[0] == subset[-1]
    full = _got(case, crit)
    got = bm.credible_ball(z, centre, crit, membership_of=subset, Kc=Kc, max_clusters=Ka)
    assert np.array_equal(got["rows"], subset) and got["sim"].shape == (len(subset), Ka)
    assert np.array_equal(got["sim"], full["sim"][subset])
    assert np.array_equal(got["membership"], full["membership"][subset], equal_nan=True)
    _same_ball(got, full, skip=("centre", "sim", "membership", "rows"))


def test_two_calls_give_the_same_bytes():
    for case in cbr.CASES[:3]:
        Kc, Ka, N, S, _ = case
        z, centre, _ = _case(case)
        for crit in CRITS:
            a = _got(case, crit)
            b = bm.credible_ball(z, centre, crit, membership=True, Kc=Kc, max_clusters=Ka)
            _same_ball(a, b, skip=())
            assert a["distance"].tobytes() == b["distance"].tobytes() and a["sim"].tobytes() == b["sim"].tobytes()


def test_without_membership_there_is_no_similarity():
    case = cbr.CASES[0]
    z, centre, _ = _case(case)
    got = bm.credible_ball(z, centre, "vi", Kc=case[0], max_clusters=case[1])
    full = _got(case, "vi")
    assert sorted(set(full) - set(got)) == ["membership", "rows", "sim", "sizes"]
    _same_ball(got, {k: full[k] for k in got})


def _data(N=600, P=8, K=3, seed=21):
    return synth(N, P, K, seed)[0]


RUNS = [("collapsed", lambda X, **kw: bm.gibbs_collapsed(X, 14, 3, burnin=4, seed=5, **kw), 3),
        ("dp", lambda X, **kw: bm.gibbs_dp(X, 14, burnin=4, seed=5, maxK=10, **kw), 10)]


@pytest.mark.parametrize("search", [False, True], ids=["visited", "search"])
@pytest.mark.parametrize("name,run,Kc", RUNS, ids=[r[0] for r in RUNS])
@pytest.mark.parametrize("crit", CRITS)
def test_through_a_run(name, run, Kc, crit, search):
    X = _data()
    kw = dict(partition=crit, **({"partition_search": True} if search else {}))
    base = run(X, **kw)
    got = _ball({"level": 0.9, "membership": True}, run, X, **kw)
    for k in ("z", "theta", "alpha"):
        assert base[k].tobytes() == got[k].tobytes(), k
    assert "credible_ball" not in base["partition"]
    for k in base["partition"]:
        if k == "search":
            for f in base["partition"]["search"]:
                assert np.array_equal(base["partition"]["search"][f], got["partition"]["search"][f]), f
        else:
            assert np.asarray(base["partition"][k]).tobytes() == np.asarray(got["partition"][k]).tobytes(), k
    b = got["partition"]["credible_ball"]
    assert b["centre"] == ("search" if search else "visited") and b["level"] == 0.9 and b["n_used"] == 10
    centre = got["partition"]["search"]["z"] if search else got["partition"]["z"]
    alone = bm.credible_ball(got["z"], centre, crit, level=0.9, membership=True, Kc=Kc, max_clusters=Kc)
    _same_ball(b, alone)
    # a level alone, and rows of the similarity
    got = _ball(0.5, run, X, **kw)
    assert "sim" not in got["partition"]["credible_ball"]
    _same_ball(got["partition"]["credible_ball"], bm.credible_ball(got["z"], centre, crit, level=0.5, Kc=Kc, max_clusters=Kc))
    got = _ball({"membership_of": [599, 0, 7, 0]}, run, X, **kw)
    _same_ball(got["partition"]["credible_ball"],
               bm.credible_ball(got["z"], centre, crit, membership_of=[599, 0, 7, 0], Kc=Kc, max_clusters=Kc))


def test_the_other_wrappers_take_it_too():
    X = _data()
    for got, Kc in ((_ball(True, bm.gibbs_stickbreaking, X, 14, 4, burnin=4, seed=5, partition="vi"), 4),
                    (_ball(True, bm.gibbs_full, X, 14, 3, burnin=4, seed=5, partition="binder"), 3),
                    (_ball(True, bm.gibbs_allocation, X, 14, 5, burnin=4, seed=5, partition="vi"), 5)):
        p = got["partition"]
        _same_ball(p["credible_ball"], bm.credible_ball(got["z"], p["z"], p["criterion"], Kc=Kc, max_clusters=Kc))


def test_two_chains_are_pooled():
    X = _data()
    for search in (False, True):
        kw = dict(partition="binder", **({"partition_search": True} if search else {}))
        base = bm.gibbs_collapsed(X, 14, 3, burnin=4, seed=5, chains=2, **kw)
        got = _ball({"membership": True}, bm.gibbs_collapsed, X, 14, 3, burnin=4, seed=5, chains=2, **kw)
        zz = np.asfortranarray(np.concatenate([o["z"] for o in got], axis=0))
        assert all(a["z"].tobytes() == b["z"].tobytes() for a, b in zip(base, got))
        p = got[0]["partition"]
        assert p is got[1]["partition"] and p["credible_ball"]["n_used"] == 20
        assert p["credible_ball"]["centre"] == ("search" if search else "visited")
        centre = p["search"]["z"] if search else p["z"]
        _same_ball(p["credible_ball"], bm.credible_ball(zz, centre, "binder", membership=True, Kc=3, max_clusters=3))


def test_dp_without_burnin_leaves_the_unassigned_row_out():
    X = _data()
    got = _ball({"membership": True}, bm.gibbs_dp, X, 9, burnin=0, seed=6, maxK=10, partition="vi", partition_search=True)
    p = got["partition"]
    b = p["credible_ball"]
    assert np.all(got["z"][0] == bm.NA_INTEGER) and p["n_used"] == b["n_used"] == got["z"].shape[0] - 1
    assert len(b["distance"]) == len(b["binder2"]) == len(b["n_clusters"]) == 8
    alone = bm.credible_ball(got["z"][1:], p["search"]["z"], "vi", membership=True, Kc=10, max_clusters=10)
    for q in BOUNDS:  # the bounds name rows of the run's trace
        assert b[q]["sweep"] == alone[q]["sweep"] + 1 and np.array_equal(b[q]["z"], got["z"][b[q]["sweep"]])
        alone[q]["sweep"] += 1
    _same_ball(b, alone)


def test_report_the_ball_on_planted_data():
    """Information for DESIGN.md section 29, no gate on the figures: planted K = 4, N = 20 000, P = 12 with the rows
    shuffled, 80 kept sweeps -- the radius, the three bounds' cluster counts, and the share of rows whose largest
    membership is not their own cluster.  Only what must hold is asserted: a row's membership of its own cluster is a
    mean of frequencies."""
    N, P, K = 20000, 12, 4
    X, labels, _, _ = synth(N, P, K, 77)
    perm = np.random.default_rng(78).permutation(N)
    X = np.asfortranarray(X[perm])
    got = _ball({"membership": True}, bm.gibbs_collapsed, X, 160, K, burnin=80, seed=11, partition="vi", partition_search=True)
    b = got["partition"]["credible_ball"]
    c = got["partition"]["search"]["z"]
    mem = b["membership"]
    own = mem[np.arange(N), c - 1]
    top = np.nanargmax(np.where(np.isnan(mem), -1.0, mem), axis=1)
    print("VI ball at 0.95 around the searched estimate: radius %.6g, %d of %d inside; clusters horizontal / upper / lower = "
          "%d / %d / %d (ties %d / %d / %d); rows whose largest membership is another cluster: %.4f; mean own membership %.4f"
          % (b["radius"], b["n_in"], b["n_used"], b["horizontal"]["n_clusters"], b["upper"]["n_clusters"],
             b["lower"]["n_clusters"], b["horizontal"]["ties"], b["upper"]["ties"], b["lower"]["ties"],
             float(np.mean(top != c - 1)), float(np.nanmean(own))))
    assert np.all(((own >= 0) & (own <= 1)) | np.isnan(own))
