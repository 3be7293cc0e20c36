"""The posterior summary's restatement (tests/summary_ref.py) on hand-made traces whose answers are known, and what
of the feature needs no device: the pure byte and launch-shape functions, and the refusals that are answered before a
device is touched (include/bmm_mcmc.h "posterior summary")."""
import ctypes as C

import numpy as np
import pytest

import bmm_mcmc_amd as bm
import summary_ref as R
from bmm_mcmc_amd import _capi


def _swapping_trace(S=8, half=4):
    """two classes of three rows each whose labels swap from row `half` on"""
    a = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    return np.stack([a if s < half else 1 - a for s in range(S)])


def test_a_label_swap_is_undone_by_the_pivot_and_halves_the_memberships_without():
    z = _swapping_trace()
    got = R.summarise(z, 2, pivot="first")
    assert got["n_folded"] == 8 and np.array_equal(got["pivot"], z[0])
    assert np.array_equal(got["permutations"][:4], [[0, 1]] * 4) and np.array_equal(got["permutations"][4:], [[1, 0]] * 4)
    assert np.array_equal(got["agree"], [6] * 8)
    assert np.array_equal(got["n_max"], [8] * 6) and np.array_equal(got["z_hat"], z[0])  # all or nothing
    assert np.array_equal(got["counts"], 8 * np.eye(2, dtype=np.uint32)[z[0]])
    assert np.array_equal(got["size_sum"], [24, 24])
    plain = R.summarise(z, 2, pivot=None)
    assert plain["pivot"] is None and np.array_equal(plain["agree"], [0] * 8)
    assert np.array_equal(plain["permutations"], [[0, 1]] * 8)
    assert np.array_equal(plain["counts"], np.full((6, 2), 4))  # 50 / 50
    assert np.array_equal(plain["n_max"], [4] * 6) and np.array_equal(plain["z_hat"], [0] * 6)  # a tie: the lowest label


def test_the_stride_folds_every_mth_kept_row_and_leaves_the_others_unmarked():
    z = _swapping_trace(S=10, half=5)
    got = R.summarise(z, 2, stride=3)
    assert got["folded"] == [0, 3, 6, 9] and got["n_folded"] == 4
    assert np.array_equal(got["agree"], [6, -1, -1, 6, -1, -1, 6, -1, -1, 6])
    assert np.array_equal(got["permutations"][[1, 2, 4, 5, 7, 8]], [[0, 1]] * 6)  # the identity where nothing was folded
    assert np.array_equal(got["permutations"][[6, 9]], [[1, 0]] * 2)
    assert np.array_equal(got["n_max"], [4] * 6)
    got = R.summarise(z, 2, stride=3, first_fold=1)  # a run without burn-in: row 0 is the starting state
    assert got["folded"] == [3, 6, 9] and np.array_equal(got["pivot"], z[0])


def test_an_unassigned_first_row_is_neither_pivot_nor_folded():
    z = _swapping_trace()
    z[0] = -1
    got = R.summarise(z, 2, first_fold=1)
    assert np.array_equal(got["pivot"], z[1]) and got["folded"] == list(range(1, 8)) and got["agree"][0] == -1
    assert np.array_equal(got["n_max"], [7] * 6) and np.array_equal(got["size_sum"], [21, 21])
    z[3, 2] = -1  # one unassigned label inside a folded row is skipped
    got = R.summarise(z, 2, first_fold=1)
    assert got["n_max"][2] == 6 and got["agree"][3] == 5 and got["size_sum"].sum() == 41


def test_a_tie_in_z_hat_goes_to_the_lowest_label():
    z = np.array([[2, 1, 0], [1, 1, 0], [2, 0, 0], [1, 0, 1]], dtype=np.int32)
    got = R.summarise(z, 3, pivot=None)
    assert np.array_equal(got["counts"], [[0, 2, 2], [2, 2, 0], [3, 1, 0]])
    assert np.array_equal(got["z_hat"], [1, 0, 0]) and np.array_equal(got["n_max"], [2, 2, 3])


def test_the_profiles_follow_the_permutation_the_way_permute_theta_does():
    rng = np.random.default_rng(3)
    z, _, _ = R.E.noisy(5, 9, 200, 4, 0.2)
    theta = rng.random((4, 6, 9))
    theta[2, :, 4] = np.nan  # an empty label of the finite sampler
    alpha = rng.random(9)
    got = R.summarise(z, 4, theta, alpha, pivot=z[0], stride=2)
    assert any(not np.array_equal(got["permutations"][s], np.arange(4)) for s in got["folded"])
    relab = bm._permute_theta(theta, got["permutations"])
    want, want_sq, n = np.zeros((4, 6)), np.zeros((4, 6)), np.zeros(4, dtype=np.int32)
    for s in got["folded"]:
        t = relab[:, :, s]
        keep = ~np.isnan(t)
        want[keep] = want[keep] + t[keep]
        want_sq[keep] = want_sq[keep] + t[keep] * t[keep]
        n += keep[:, 0]
    assert np.array_equal(got["theta_sum"], want) and np.array_equal(got["theta_sq"], want_sq)
    assert np.array_equal(got["theta_n"], n) and n.min() == len(got["folded"]) - 1
    assert got["alpha_sum"][0] == sum(alpha[s] for s in got["folded"])
    for s in got["folded"]:  # the permutation of a row is ecr_ref's, and relabels it towards the pivot
        assert got["agree"][s] == (got["permutations"][s][z[s]] == z[0]).sum() >= (z[s] == z[0]).sum()


# ---------------------------------------------------------------- the pure functions
def test_without_the_trace_no_term_of_run_bytes_grows_with_S_times_N():
    # two shapes with the same S K P and the same N K whose S N differs 64-fold: the bytes may differ by the per-sweep
    # scalars (alpha, and the summary's agreement and permutation: (16 + 4 K) bytes a sweep) and the per-row vectors (the
    # pivot, z_hat, n_max: 12 bytes a row), the K P sums (three of them) and carving slack -- nothing near 4 S N
    a = dict(N=1 << 12, P=64, K=16, S=1 << 6)
    b = dict(N=1 << 15, P=64, K=2, S=1 << 9)
    assert a["S"] * a["K"] * a["P"] == b["S"] * b["K"] * b["P"] and a["N"] * a["K"] == b["N"] * b["K"]
    for sampler in ("collapsed", "dp", "stickbreaking", "full"):
        ba = bm.run_bytes(sampler, keep_trace=False, summary=True, **a)
        bb = bm.run_bytes(sampler, keep_trace=False, summary=True, **b)
        small = (12 * abs(b["N"] - a["N"]) + (16 + 4 * 16 + 8 * 16) * abs(b["S"] - a["S"])
                 + 24 * abs(b["K"] * b["P"] - a["K"] * a["P"]) + 64 * 256)
        assert abs(bb - ba) <= small < 4 * (b["S"] * b["N"] - a["S"] * a["N"]) // 100
        # ... and with it, exactly the trace and the staging of its way out more
        for q in (a, b):
            for summary in (False, True):
                more = bm.run_bytes(sampler, keep_trace=True, summary=summary, **q) - bm.run_bytes(sampler, keep_trace=False, summary=summary, **q)
                assert more == R.trace_bytes(q["S"], q["N"], q["K"]) >= 4 * q["S"] * q["N"]
    # growing S N at everything else fixed moves the run with a trace by exactly 4 dS N (the staging is at its cap)
    big = dict(sampler="collapsed", N=10 ** 7, P=100, K=20)
    assert bm.run_bytes(S=2000, **big) - bm.run_bytes(S=1000, **big) >= 4 * 1000 * 10 ** 7
    assert bm.run_bytes(S=1000, keep_trace=False, summary=True, **big) < 10 ** 9 < 40 * 10 ** 9 < bm.run_bytes(S=1000, **big)
    with pytest.raises(ValueError):
        bm.run_bytes("collapsed", 0, 1, 1, 1)


def test_summary_plan_is_pure_and_caps_the_grid():
    p = bm.summary_plan(4099, 12, 20)
    assert p == bm.summary_plan(4099, 12, 20)
    assert p["threads"] == 256 and p["fold_workgroups"] == 17 and p["pitch"] == 4160 and p["fold_lds_bytes"] == 80
    assert p["profile_workgroups"] == 1 and p["finish_workgroups"] == 17 and p["bytes_counts"] == 20 * 4160 * 4
    assert p["launches_pivot"] == 8 and p["launches_plain"] == 2
    cap = p["grid_cap"]
    one_trip = cap * p["threads"]
    assert bm.summary_plan(one_trip, 5, 3)["fold_workgroups"] == cap == bm.summary_plan(one_trip + 1, 5, 3)["fold_workgroups"]
    assert bm.summary_plan(one_trip - 256, 5, 3)["fold_workgroups"] == cap - 1
    assert bm.summary_plan(10 ** 7, 100, 20)["bytes_counts"] == 800_000_000
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1 << 32, 1, 1)):
        with pytest.raises(bm.BmmError) as e:
            bm.summary_plan(*bad)
        assert e.value.code == 1


# ---------------------------------------------------------------- refused before a device is touched
def _x(N=40, P=5):
    return np.asfortranarray((np.random.default_rng(0).random((N, P)) < 0.5).astype(np.int32))


RUNS = {"collapsed": lambda X, **kw: bm.gibbs_collapsed(X, 6, 3, seed=1, **kw),
        "dp": lambda X, **kw: bm.gibbs_dp(X, 6, maxK=5, seed=1, **kw),
        "stickbreaking": lambda X, **kw: bm.gibbs_stickbreaking(X, 6, 4, seed=1, **kw),
        "full": lambda X, **kw: bm.gibbs_full(X, 6, 3, seed=1, **kw)}


@pytest.mark.parametrize("sampler", sorted(RUNS))
def test_the_wrappers_refuse_what_they_cannot_run(sampler):
    run, X = RUNS[sampler], _x()
    for kw, word in (({"keep_trace": False}, "needs summary="),
                     ({"summary": True, "chains": 2}, "per chain"),
                     ({"summary": True, "relabel": "ecr"}, "two relabellings"),
                     ({"summary": True, "relabel": True}, "two relabellings"),
                     ({"summary": True, "keep_trace": False, "partition": "binder"}, "partition="),
                     ({"summary": True, "keep_trace": False, "partition": "binder", "similarity_of": [0, 1]}, "partition="),
                     ({"summary": "all"}, "summary must be"),
                     ({"summary": True, "summary_pivot": "last"}, "summary_pivot"),
                     ({"summary": True, "summary_pivot": np.ones(7, dtype=np.int32)}, "one label per observation")):
        with pytest.raises(ValueError, match=word):
            run(X, **kw)


@pytest.mark.parametrize("sampler", sorted(RUNS))
def test_the_library_refuses_the_rest_before_a_device_is_touched(sampler):
    run, X = RUNS[sampler], _x()
    K = {"collapsed": 3, "dp": 5, "stickbreaking": 4, "full": 3}[sampler]
    bad = np.ones(40, dtype=np.int32)
    bad[11] = K + 1
    for kw, word in (({"summary_stride": 0}, "stride must be >= 1"), ({"summary_pivot": bad}, r"pivot label %d at observation 11" % (K + 1)),
                     ({"summary_pivot": np.zeros(40, dtype=np.int32)}, "pivot label 0 at observation 0")):
        with pytest.raises(bm.BmmError, match=word) as e:
            run(X, summary=True, **kw)
        assert e.value.code == 1
    big = {"collapsed": lambda **kw: bm.gibbs_collapsed(X, 6, 129, seed=1, **kw), "dp": lambda **kw: bm.gibbs_dp(X, 6, maxK=129, seed=1, **kw),
           "stickbreaking": lambda **kw: bm.gibbs_stickbreaking(X, 6, 129, seed=1, **kw),
           "full": lambda **kw: bm.gibbs_full(X, 6, 129, seed=1, **kw)}[sampler]
    with pytest.raises(bm.BmmError, match=r"up to K = 128 \(got 129\)") as e:
        big(summary=True)
    assert e.value.code == 1


def _arm(stride=1, keep_trace=1):
    fold = bm._SummaryFold(40, 3, 5, None, stride, keep_trace=bool(keep_trace))
    fold.arm()
    return fold  # (keeps the buffers alive)


def test_two_relabellings_tempering_and_the_allocation_sampler_are_refused_with_their_codes():
    X = _x()
    keep = _arm()
    with pytest.raises(bm.BmmError, match="two relabellings") as e:  # ECR armed by the wrapper beside it
        bm.gibbs_collapsed(X, 6, 3, seed=1, relabel="ecr", ecr_pivot=np.ones(40, dtype=np.int32))
    assert e.value.code == 1
    keep = _arm(keep_trace=0)
    with pytest.raises(bm.BmmError, match="reads the label trace") as e:
        bm.gibbs_collapsed(X, 6, 3, seed=1, partition="binder")
    assert e.value.code == 1
    with pytest.raises(bm.BmmError, match="parallel tempering") as e:
        bm.gibbs_collapsed(X, 6, 3, seed=1, summary=True, temper=2)
    assert e.value.code == 2
    keep = _arm()
    with pytest.raises(bm.BmmError, match="allocation sampler") as e:
        bm.gibbs_allocation(X, 6, 3, seed=1)
    assert e.value.code == 2
    del keep


def test_a_null_z_out_is_refused_unless_a_summary_drops_the_trace():
    X, L = _x(), _capi.lib()
    z0 = np.ones(40, dtype=np.int32)
    theta, al = np.zeros((3, 5, 5), order="F"), np.zeros(5)
    args = (_capi.vp(X), C.c_int64(40), C.c_int(5), _capi.vp(z0), C.c_int(6), C.c_int(3), C.c_double(1.0), C.c_double(0.5),
            C.c_double(0.5), C.c_double(1.0), C.c_double(1.0), C.c_int(1), C.c_int64(0), C.c_uint64(1), C.c_int(0), None,
            _capi.vp(theta), _capi.vp(al))
    assert L.bmm_collapsed_run(*args) == 1 and b"null buffer" in L.bmm_last_error()  # nothing armed
    keep = _arm(keep_trace=1)
    assert L.bmm_collapsed_run(*args) == 1 and b"null buffer" in L.bmm_last_error()  # armed, but the trace is kept
    keep = _arm(stride=0, keep_trace=0)  # accepted as far as z_out goes: the next refusal answers
    assert L.bmm_collapsed_run(*args) == 1 and b"stride must be >= 1" in L.bmm_last_error()
    assert L.bmm_collapsed_run(*args) == 1 and b"null buffer" in L.bmm_last_error()  # ... and the call disarmed it
    del keep
