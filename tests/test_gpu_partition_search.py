"""Greedy search for the clustering point estimate on the device (include/bmm_mcmc.h "greedy search", DESIGN.md section
27).  Binder: the result, its exact total and the whole course of the search -- passes, batches, moved rows, totals,
converged -- equal the NumPy restatement tests/partition_search_ref.py with ==, on partition_search_ref.CASES
(tests/test_partition_search_ref.py proves they reach every form of the kernels that a device can be given), and the
total equals what the existing distance kernels give for the result.  VI: near-ties may be decided differently from a
NumPy sum, so it is held by what must be true -- the reported loss is the expected VI of the result by the existing
device distances, it is no worse than the start, a converged result passes the brute-force check, and two calls give
the same bits; decision by decision it is held to a restatement in tests/test_gpu_partition_search_vi.py, on cases
whose gaps exclude every near-tie.  Through a run: the armed search equals the stand-alone call and leaves everything
else as it was."""
import functools

import numpy as np
import pytest

import bmm_mcmc_amd as bm
import partition_ref as pr
import partition_search_ref as ref
from util import synth

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _trace(case):
    Kc, N, S = case[0], case[1], case[2]
    z, _ = ref.make_trace(Kc, N, S, ref.EPS, 100 + Kc)
    z.setflags(write=False)
    return z


def _device_total_of(z_hat, z, crit, Kc):
    """the candidate stacked as row 0 on the trace, through the existing kernels: (binder2, expected VI) of row 0
    over the S draws (its distance to itself is 0)"""
    stack = np.asfortranarray(np.concatenate([np.asarray(z_hat, dtype=np.int32)[None, :], z], axis=0))
    got = bm.partition_distances(stack, crit, stride=stack.shape[0], distances=True, Kc=Kc)
    return int(got["binder2"][0]), float(got["distances"][0, 1:].sum()) / z.shape[0]


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_binder_equals_the_restatement(case):
    Kc, N, S, batch, min_batch, _ = case
    z = _trace(case)
    start = ref.start_of(case, z)
    want = ref.search(z, Kc, "binder", start, batch, min_batch)
    got = bm.partition_search(z, "binder", start=start, batch=batch, min_batch=min_batch, Kc=Kc)
    print("binder %s: %d -> %d (%.3f of the start), %d passes, batches %s, moved %s, converged %s, %d clusters"
          % (ref.case_id(case), got["start_binder2"], got["binder2"],
             got["binder2"] / max(1, got["start_binder2"]), got["passes"], sorted(set(got["batch"]), reverse=True),
             got["moved"], got["converged"], got["n_clusters"]))
    assert got["start_binder2"] == want["start_binder2"]
    assert got["passes"] == want["passes"] and got["batch"] == want["batch"] and got["moved"] == want["moved"]
    assert got["total"] == want["pass_total"]
    assert got["converged"] == want["converged"] and got["n_clusters"] == want["n_clusters"]
    assert np.array_equal(got["z"], want["z"]) and got["z"].dtype == np.int32
    assert got["binder2"] == want["binder2"]
    assert got["loss"] == want["binder2"] / (2.0 * S) and got["start_loss"] == want["start_binder2"] / (2.0 * S)
    # the new totals held to the old kernels
    assert got["binder2"] == _device_total_of(got["z"], z, "binder", Kc)[0]
    if N >= 65:
        assert want["binder2"] < want["start_binder2"]  # the restatement alone says so ...
        assert got["binder2"] < got["start_binder2"]    # ... and so does the device


def _no_single_move_lowers_vi(z, c, Kc, bound):
    """brute force over every row and slot: the change of the fsum expected VI (the terms the move changes, summed
    with fsum) is no lower than minus the bound"""
    st = ref.State(z, c, Kc, Kc)
    for i in range(st.N):
        for a in range(Kc):
            assert st.move_delta_vi(i, a) / (st.S * st.N) >= -bound, (i, a)


@pytest.mark.parametrize("case", ref.CASES, ids=ref.case_id)
def test_vi_by_what_must_be_true(case):
    Kc, N, S, batch, min_batch, _ = case
    z = _trace(case)
    start = ref.start_of(case, z)
    got = bm.partition_search(z, "vi", start=start, batch=batch, min_batch=min_batch, Kc=Kc)
    bound = pr.vi_bound(Kc, N)
    b2, vi = _device_total_of(got["z"], z, "vi", Kc)
    print("vi %s: %.6g -> %.6g, |loss - device distances| = %.3g (bound %.3g), %d passes, batches %s, converged %s, %d clusters"
          % (ref.case_id(case), got["start_loss"], got["loss"], abs(got["loss"] - vi), bound, got["passes"],
             sorted(set(got["batch"]), reverse=True), got["converged"], got["n_clusters"]))
    assert abs(got["loss"] - vi) <= bound
    assert got["binder2"] == b2
    assert got["loss"] <= got["start_loss"]
    assert 1 <= got["passes"] <= 50 and len(got["batch"]) == len(got["moved"]) == len(got["total"]) == got["passes"]
    assert got["z"].min() >= 1 and got["z"].max() <= Kc and got["n_clusters"] == len(np.unique(got["z"]))
    if got["converged"]:
        assert got["moved"][-1] == 0
        if N <= 257:
            _no_single_move_lowers_vi(z, got["z"], Kc, bound)
    again = bm.partition_search(z, "vi", start=start, batch=batch, min_batch=min_batch, Kc=Kc)
    assert np.array_equal(again["z"], got["z"]) and again["loss"] == got["loss"] and again["total"] == got["total"]
    assert again["moved"] == got["moved"] and again["batch"] == got["batch"]


def test_more_slots_than_labels_and_fewer():
    """Ka above Kc: empty slots to open; a start inside Ka = 2 < Kc: the rows stay inside the two slots"""
    case = (3, 65, 17, 16, 1, "best")
    z = _trace(case)
    for Ka, start in ((7, None), (2, np.where(np.arange(65) % 2 == 0, 1, 2).astype(np.int32))):
        want = ref.search(z, 3, "binder", start, 16, 1, Ka=Ka)
        got = bm.partition_search(z, "binder", start=start, batch=16, min_batch=1, max_clusters=Ka, Kc=3)
        assert np.array_equal(got["z"], want["z"]) and got["total"] == want["pass_total"] and got["moved"] == want["moved"]
        assert got["z"].max() <= Ka


def _data(N=600, P=8, K=3, seed=21):
    return synth(N, P, K, seed)[0]


def _same_search(p, q):
    assert sorted(p) == sorted(q)
    for k in p:
        assert np.array_equal(p[k], q[k]) if k == "z" else p[k] == q[k], k


RUNS = [("collapsed", lambda X, **kw: bm.gibbs_collapsed(X, 14, 3, burnin=4, seed=5, **kw), 3),
        ("dp", lambda X, **kw: bm.gibbs_dp(X, 14, burnin=4, seed=5, maxK=10, **kw), 10),
        ("sb", lambda X, **kw: bm.gibbs_stickbreaking(X, 14, 4, burnin=4, seed=5, **kw), 4),
        ("full", lambda X, **kw: bm.gibbs_full(X, 14, 3, burnin=4, seed=5, **kw), 3)]


@pytest.mark.parametrize("name,run,Kc", RUNS, ids=[r[0] for r in RUNS])
@pytest.mark.parametrize("crit", ["binder", "vi"])
def test_through_a_run(name, run, Kc, crit):
    X = _data()
    base = run(X, partition=crit)
    got = run(X, partition=crit, partition_search=True)
    for k in ("z", "theta", "alpha", "pi"):
        if k in base:
            assert np.array_equal(base[k], got[k], equal_nan=True), k
    assert "search" not in base["partition"]
    for k in base["partition"]:
        assert np.array_equal(base["partition"][k], got["partition"][k]), k
    s = got["partition"]["search"]
    assert sorted(s) == ["batch", "binder2", "converged", "loss", "moved", "n_clusters", "passes", "start_binder2",
                         "start_loss", "total", "z"]
    _same_search(s, bm.partition_search(got["z"], crit, start=got["partition"]["z"], Kc=Kc))
    assert s["loss"] <= s["start_loss"]
    if crit == "binder":
        assert s["start_loss"] == got["partition"]["loss"].min() and s["start_binder2"] == int(got["partition"]["binder2"].min())
    else:
        assert abs(s["start_loss"] - got["partition"]["loss"].min()) <= pr.vi_bound(Kc, X.shape[0])
    # options in a dict
    got = run(X, partition=crit, partition_search={"batch": 50, "min_batch": 5, "max_passes": 7})
    _same_search(got["partition"]["search"],
                 bm.partition_search(got["z"], crit, start=got["partition"]["z"], batch=50, min_batch=5, max_passes=7, Kc=Kc))


def test_two_chains_are_pooled():
    X = _data()
    base = bm.gibbs_collapsed(X, 14, 3, burnin=4, seed=5, chains=2, partition="binder")
    got = bm.gibbs_collapsed(X, 14, 3, burnin=4, seed=5, chains=2, partition="binder", partition_search=True)
    zz = np.asfortranarray(np.concatenate([o["z"] for o in got], axis=0))
    assert all(np.array_equal(a["z"], b["z"]) for a, b in zip(base, got))
    p = got[0]["partition"]
    assert p is got[1]["partition"]
    for k in base[0]["partition"]:
        assert np.array_equal(base[0]["partition"][k], p[k]), k
    _same_search(p["search"], bm.partition_search(zz, "binder", start=p["z"], Kc=3))


def test_dp_without_burnin_leaves_the_unassigned_row_out():
    X = _data()
    got = bm.gibbs_dp(X, 9, burnin=0, seed=6, maxK=10, partition="binder", partition_search=True)
    assert np.all(got["z"][0] == bm.NA_INTEGER) and got["partition"]["n_used"] == got["z"].shape[0] - 1
    _same_search(got["partition"]["search"],
                 bm.partition_search(got["z"][1:], "binder", start=got["partition"]["z"], Kc=10))


def test_report_the_search_against_the_generating_allocation():
    """Information for DESIGN.md section 27, no assertion on the figures: the shape of section 13's medoid test (K = 4,
    N = 20 000, P = 12, 80 kept sweeps) -- B(z, truth) for the visited estimate and for the searched one."""
    N, P, K = 20000, 12, 4
    X, labels, _, _ = synth(N, P, K, 77)
    truth = (labels + 1).astype(np.int32)
    got = bm.gibbs_collapsed(X, 160, K, burnin=80, seed=11, initial_K=truth, partition="binder", partition_search=True)
    s = got["partition"]["search"]
    stack = np.asfortranarray(np.stack([truth, got["partition"]["z"], s["z"]]))
    d = bm.partition_distances(stack, "binder", stride=3, distances=True, Kc=K)["distances"][0]
    print("B(visited, truth) = %d, B(searched, truth) = %d; expected Binder loss %.6g -> %.6g in %d passes (moved %s), converged %s"
          % (d[1], d[2], s["start_loss"], s["loss"], s["passes"], s["moved"], s["converged"]))
