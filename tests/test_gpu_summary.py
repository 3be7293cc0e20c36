"""The posterior summary on the device (include/bmm_mcmc.h "posterior summary"): an armed run is an
unarmed run; its permutations and agreements are those of the pinned relabelling (bm.ecr_relabel, which
tests/test_gpu_ecr.py holds to tests/ecr_ref.py) of the same trace against the same pivot; its counts are the per-row
bincounts of that relabelled trace; everything else equals the restatement tests/summary_ref.py; a run without the
label trace returns the same summary.  Every comparison is ==: integers, and sums added in a stated order."""
import ctypes as C

import numpy as np
import pytest

import bmm_mcmc_amd as bm
import summary_ref as R
from bmm_mcmc_amd import _capi
from util import synth

pytestmark = pytest.mark.gpu

S_RUN = 17  # kept rows of a run without burn-in: the starting row, which is never folded, and 16 sweeps


def _data(N, P, seed=7):
    return synth(N, P, 3, seed)[0]


def _run(sampler, X, K, nsamples=S_RUN, burnin=0, seed=11, **kw):
    N, P = X.shape
    rng = np.random.default_rng(seed)
    if sampler == "collapsed":
        return bm.gibbs_collapsed(X, nsamples, K, burnin=burnin, seed=seed, initial_K=rng.integers(1, K + 1, N).astype(np.int32), **kw)
    if sampler == "dp":
        return bm.gibbs_dp(X, nsamples, burnin=burnin, maxK=K, seed=seed, **kw)
    pi0 = rng.dirichlet(np.ones(K))
    th0 = 0.1 + 0.8 * rng.random((K, P))
    fn = bm.gibbs_stickbreaking if sampler == "stickbreaking" else bm.gibbs_full
    return fn(X, nsamples, K, burnin=burnin, seed=seed, initial_pi=pi0, initial_theta=th0, **kw)


def _layout(dbg_lib, layout):
    if layout == "int32":
        dbg_lib.setenv("BMM_X_LAYOUT_INT32", "1")
    else:
        dbg_lib.delenv("BMM_X_LAYOUT_INT32", raising=False)


def _zero_based(z):
    """the trace 0-based, -1 wherever a label is not one of 1 .. (NA in the starting row of three samplers)"""
    return np.where(z >= 1, z - 1, -1).astype(np.int32)


def _check(out, K, pivot="first", stride=1, burnin=0):
    """an armed run with its trace kept, against the pinned relabelling and the restatement"""
    su, z, theta, alpha = out["summary"], out["z"], out["theta"], out["alpha"]
    S, N = z.shape
    z0 = _zero_based(z)
    rows = R.folded_rows(S, stride, 1 if burnin == 0 else 0)
    assert su["n_folded"] == len(rows) and su["agree"].dtype == np.int64 and su["permutations"].dtype == np.int32
    rest = [s for s in range(S) if s not in rows]
    assert np.array_equal(su["agree"][rest], [-1] * len(rest))
    assert np.array_equal(su["permutations"][rest], np.tile(np.arange(K), (len(rest), 1)))
    if pivot is None:
        assert su["pivot"] is None and np.array_equal(su["agree"][rows], [0] * len(rows))
        assert np.array_equal(su["permutations"][rows], np.tile(np.arange(K), (len(rows), 1)))
        relabelled = z[rows]
        given = None
    else:
        if isinstance(pivot, str):
            first = R.first_assigned(z0)
            assert first in (0, 1) and np.array_equal(su["pivot"], z[first])
        else:
            assert np.array_equal(su["pivot"], pivot)
        e = bm.ecr_relabel(z[rows], K, pivot=su["pivot"], theta=theta[:, :, rows])
        assert np.array_equal(e["permutations"], su["permutations"][rows])
        assert np.array_equal(e["agree"], su["agree"][rows])
        relabelled = e["z"]
        given = su["pivot"] - 1
    if "counts" in su:
        want = np.stack([(relabelled == k + 1).sum(axis=0) for k in range(K)], axis=1)  # the per-row bincounts, label by label
        assert su["counts"].dtype == np.uint32 and su["counts"].shape == (N, K) and np.array_equal(su["counts"], want)
    ref = R.summarise(z0, K, theta, alpha, pivot=given, stride=stride, first_fold=1 if burnin == 0 else 0,
                      permutations=None if pivot is None else su["permutations"])
    assert ref["folded"] == rows
    if pivot is not None:
        assert np.array_equal(ref["agree"], su["agree"])
    if "counts" in su:
        assert np.array_equal(su["counts"], ref["counts"])
    assert np.array_equal(su["z_hat"], ref["z_hat"] + 1) and np.array_equal(su["n_max"], ref["n_max"])
    assert su["size_sum"].dtype == np.int64 and np.array_equal(su["size_sum"], ref["size_sum"])
    assert su["theta_sum"].tobytes() == np.asfortranarray(ref["theta_sum"]).tobytes()
    assert su["theta_sq"].tobytes() == np.asfortranarray(ref["theta_sq"]).tobytes()
    assert np.array_equal(su["theta_n"], ref["theta_n"]) and su["alpha_sum"].tobytes() == ref["alpha_sum"].tobytes()
    return su


# (sampler, N, K, P): the smallest; past one workgroup (16 table copies); several slices (2 copies in an 8-row pass); 1
# copy; the generic table form; the cap; the DP and the two explicit samplers
SHAPES = [("collapsed", 1, 2, 3), ("collapsed", 257, 3, 50), ("collapsed", 4099, 20, 12), ("collapsed", 4099, 28, 7),
          ("collapsed", 1500, 111, 3), ("collapsed", 1500, 128, 4), ("dp", 2003, 30, 12), ("stickbreaking", 2003, 6, 33),
          ("full", 2003, 4, 12)]


@pytest.mark.parametrize("layout", ["bits", "int32"])
@pytest.mark.parametrize("sampler,N,K,P", SHAPES, ids=lambda v: str(v))
def test_every_shape_against_the_pinned_relabelling_and_the_restatement(dbg_lib, sampler, N, K, P, layout):
    _layout(dbg_lib, layout)
    X = _data(N, P)
    out = _run(sampler, X, K, summary="counts")
    su = _check(out, K)
    assert su["size_sum"].sum() == 16 * N
    plain = _run(sampler, X, K)  # armed versus unarmed: the same seed, the same bytes
    for k in ("z", "theta", "alpha"):
        assert out[k].tobytes() == plain[k].tobytes(), k


@pytest.mark.parametrize("layout", ["bits", "int32"])
def test_one_observation_past_a_trip_of_the_fold_grid(dbg_lib, layout):
    _layout(dbg_lib, layout)
    plan = bm.summary_plan(1, 5, 3)
    N = plan["grid_cap"] * plan["threads"] + 1
    assert bm.summary_plan(N, 5, 3)["fold_workgroups"] == plan["grid_cap"]
    X = _data(N, 5)
    out = _run("collapsed", X, 3, nsamples=5, summary="counts")
    su = _check(out, 3)
    assert su["n_folded"] == 4 and su["counts"][-1].sum() == 4 and su["n_max"][-1] >= 2


@pytest.mark.parametrize("sampler,K", [("collapsed", 4), ("dp", 8)])
@pytest.mark.parametrize("stride", [1, 3])
def test_stride_and_the_three_pivots(sampler, K, stride):
    X = _data(2003, 12)
    given = np.random.default_rng(2).integers(1, K + 1, 2003).astype(np.int32)
    for pivot in ("first", given, None):
        for burnin in (0, 4):
            out = _run(sampler, X, K, nsamples=S_RUN + burnin, burnin=burnin, summary="counts", summary_pivot=pivot, summary_stride=stride)
            su = _check(out, K, pivot=pivot, stride=stride, burnin=burnin)
            assert su["n_folded"] == len(range(0 if burnin else stride, S_RUN, stride))
            assert set(su) == {"pivot", "z_hat", "n_max", "n_folded", "size_sum", "pi_mean", "theta_sum", "theta_sq", "theta_n",
                               "theta_mean", "theta_sd", "alpha_mean", "alpha_sum", "agree", "permutations", "counts"}
            assert abs(su["pi_mean"].sum() - 1.0) < 1e-12 and su["alpha_mean"] == su["alpha_sum"][0] / su["n_folded"]
            used = su["theta_n"] > 0
            assert np.array_equal(su["theta_mean"][used], su["theta_sum"][used] / su["theta_n"][used, None])


def test_the_derived_fields_and_the_plain_summary_omit_the_counts():
    out = _run("collapsed", _data(500, 6), 3, summary=True)
    assert "counts" not in out["summary"]
    _check(out, 3)


def test_known_rows_pin_the_labelling_without_a_pivot():
    X, lab, _, _ = synth(1500, 14, 3, 5)
    known = np.zeros(1500, dtype=np.int32)
    held = np.concatenate([np.flatnonzero(lab == k)[:5] for k in range(3)])
    known[held] = lab[held] + 1
    out = _run("collapsed", X, 3, known=known, summary="counts", summary_pivot=None)
    su = _check(out, 3, pivot=None)
    assert np.array_equal(su["n_max"][held], [su["n_folded"]] * held.size) and np.array_equal(su["z_hat"][held], known[held])
    plain = _run("collapsed", X, 3, known=known)
    for k in ("z", "theta", "alpha"):
        assert out[k].tobytes() == plain[k].tobytes(), k


@pytest.mark.parametrize("kw", [{"allowed": True}, {"init": "kmodes"}, {"logpost": True}], ids=lambda v: next(iter(v)))
def test_it_composes_with_what_only_reads_or_acts_between_sweeps(kw):
    X = _data(1500, 14)
    kw = dict(kw)
    if "allowed" in kw:
        A = np.ones((1500, 3), dtype=bool)
        A[:40, 2] = False
        kw["allowed"] = A
    rng = np.random.default_rng(11)
    z0 = rng.integers(1, 4, 1500).astype(np.int32)
    base = dict(burnin=2, seed=11) if "init" in kw else dict(burnin=2, seed=11, initial_K=z0)
    armed = bm.gibbs_collapsed(X, 14, 3, summary="counts", **base, **kw)
    plain = bm.gibbs_collapsed(X, 14, 3, **base, **kw)
    for k in ("z", "theta", "alpha"):
        assert armed[k].tobytes() == plain[k].tobytes(), k
    if "logpost" in kw:
        assert armed["logpost"]["log_joint"].tobytes() == plain["logpost"]["log_joint"].tobytes()
    _check(armed, 3, burnin=2)


@pytest.mark.parametrize("sampler,K", [("collapsed", 4), ("dp", 8), ("stickbreaking", 6), ("full", 4)])
@pytest.mark.parametrize("burnin", [0, 3])
def test_without_the_label_trace_everything_else_is_the_same_bytes(sampler, K, burnin):
    X = _data(2003, 12)
    kw = dict(nsamples=S_RUN + burnin, burnin=burnin, summary="counts", summary_stride=2)
    kept = _run(sampler, X, K, **kw)
    lean = _run(sampler, X, K, keep_trace=False, **kw)
    assert lean["z"] is None and kept["z"] is not None
    for k in ("theta", "alpha") + (("pi",) if "pi" in kept else ()):
        assert lean[k].tobytes() == kept[k].tobytes(), k
    assert set(lean["summary"]) == set(kept["summary"])
    for k, v in kept["summary"].items():
        w = lean["summary"][k]
        assert (v.tobytes() == w.tobytes() and v.dtype == w.dtype) if isinstance(v, np.ndarray) else (v == w or (v != v and w != w)), k
    assert kept["summary"]["n_folded"] == len(R.folded_rows(S_RUN, 2, 0 if burnin else 1))


def test_a_resident_chain_folds_what_the_run_folds():
    N, P, K, burnin, S, stride = 2003, 12, 4, 3, 9, 2
    X = _data(N, P)
    z0 = np.random.default_rng(11).integers(1, K + 1, N).astype(np.int32)
    out = bm.gibbs_collapsed(X, burnin + S, K, burnin=burnin, seed=11, batch=250, initial_K=z0, summary="counts", summary_stride=stride)
    run = _check(out, K, stride=stride, burnin=burnin)
    with bm.Chain("collapsed", N, P, K, seed=11, batch=250) as c:
        c.set_data(X)
        c.set_initial_labels(z0)
        c.sweeps(burnin - 1)
        with pytest.raises(bm.BmmError) as e:
            c.sweeps_summary(1)
        assert e.value.code == 5  # not armed
        c.set_summary("first", stride=stride)
        with pytest.raises(bm.BmmError, match="no pivot yet") as e:
            c.summary_state()
        assert e.value.code == 5
        tr = c.sweeps_summary(S, trace=True)
        assert np.array_equal(tr["agree"], run["agree"]) and np.array_equal(tr["permutations"], run["permutations"])
        got = c.summary(counts=True)
        for k in ("pivot", "z_hat", "n_max", "size_sum", "theta_sum", "theta_sq", "theta_n", "alpha_sum", "counts"):
            assert got[k].tobytes() == run[k].tobytes(), k
        assert got["n_folded"] == run["n_folded"] == 5
        assert np.array_equal(c.labels(), out["z"][-1])
        st = c.summary_state()  # the present state against the pivot: the last folded row's answer, the fold untouched
        assert np.array_equal(st["permutation"], run["permutations"][-1]) and st["agree"] == run["agree"][-1]
        assert c.summary(counts=True)["counts"].tobytes() == run["counts"].tobytes()
        c.sweeps(2)  # armed, not folding
        assert c.summary()["n_folded"] == 5
        c.summary_reset()
        again = c.summary(counts=True)
        assert again["n_folded"] == 0 and not again["counts"].any() and not again["theta_sum"].any() and not again["n_max"].any()
        c.sweeps_summary(4)
        again = c.summary(counts=True)
        assert again["n_folded"] == 2 and np.array_equal(again["counts"].sum(axis=1), [2] * N)
        assert not np.array_equal(again["pivot"], run["pivot"])  # a new first state
        c.set_summary(on=False)
        with pytest.raises(bm.BmmError) as e:
            c.summary()
        assert e.value.code == 5


def test_refusals_return_their_codes_and_leave_the_next_run_alone():
    X = _data(600, 8)
    want = _run("collapsed", X, 3)

    def unarmed_is_unchanged():
        got = _run("collapsed", X, 3)
        for k in ("z", "theta", "alpha"):
            assert got[k].tobytes() == want[k].tobytes(), k

    bad = np.ones(600, dtype=np.int32)
    bad[5] = 4
    for kw, code, word in (({"summary_stride": 0}, 1, "stride"), ({"summary_pivot": bad}, 1, "pivot label 4 at observation 5"),
                           ({"temper": 2}, 2, "parallel tempering")):
        with pytest.raises(bm.BmmError, match=word) as e:
            _run("collapsed", X, 3, summary=True, **kw)
        assert e.value.code == code
        unarmed_is_unchanged()
    with pytest.raises(bm.BmmError, match=r"up to K = 128 \(got 129\)") as e:
        _run("collapsed", X, 129, summary=True)
    assert e.value.code == 1
    big = _run("collapsed", X, 129, nsamples=4, summary=True, summary_pivot=None)  # ... unless the pivot is None
    assert big["summary"]["n_folded"] == 3 and big["summary"]["size_sum"].sum() == 3 * 600
    for kw, word in (({"keep_trace": False}, "needs summary="), ({"summary": True, "chains": 2}, "per chain"),
                     ({"summary": True, "relabel": "ecr"}, "two relabellings"),
                     ({"summary": True, "keep_trace": False, "partition": "binder"}, "partition=")):
        with pytest.raises(ValueError, match=word):
            _run("collapsed", X, 3, **kw)
        unarmed_is_unchanged()
    # armed at the C interface beside what the wrapper arms: the library's own answers
    for keep_trace, kw, code, word in ((1, {"relabel": "ecr"}, 1, "two relabellings"), (0, {"partition": "binder"}, 1, "reads the label trace")):
        fold = bm._SummaryFold(600, 3, 8, "first", 1, keep_trace=bool(keep_trace))
        fold.arm()
        with pytest.raises(bm.BmmError, match=word) as e:
            _run("collapsed", X, 3, **kw)
        assert e.value.code == code
        unarmed_is_unchanged()
    fold = bm._SummaryFold(600, 3, 8, "first", 1)
    fold.arm()
    with pytest.raises(bm.BmmError, match="allocation sampler") as e:
        bm.gibbs_allocation(X, 6, 3, seed=1)
    assert e.value.code == 2
    unarmed_is_unchanged()
    fold.arm()  # a run of several chains disarms it, as it disarms ECR
    outs = bm.gibbs_collapsed(X, 6, 3, seed=1, chains=2)
    assert all("summary" not in o for o in outs)
    unarmed_is_unchanged()
    # the C entry point with z_out == NULL and nothing armed
    L = _capi.lib()
    z0 = np.ones(600, dtype=np.int32)
    theta, al = np.zeros((3, 8, 5), order="F"), np.zeros(5)
    rc = L.bmm_collapsed_run(_capi.vp(X), C.c_int64(600), C.c_int(8), _capi.vp(z0), C.c_int(6), C.c_int(3), C.c_double(1.0),
                             C.c_double(0.5), C.c_double(0.5), C.c_double(1.0), C.c_double(1.0), C.c_int(1), C.c_int64(0), C.c_uint64(1),
                             C.c_int(0), None, _capi.vp(theta), _capi.vp(al))
    assert rc == 1 and b"null buffer" in L.bmm_last_error()
    unarmed_is_unchanged()
    # resident chains: a sharded chain, the allocation sampler, a tempered chain
    with bm.Chain("full", 600, 8, 3, seed=1) as c:
        c.set_data(X)
        c.set_shard(1200, 0)
        with pytest.raises(bm.BmmError, match="sharded") as e:
            c.set_summary()
        assert e.value.code == 2
    with bm.Chain("collapsed", 600, 8, 3, seed=1) as c:
        c.set_data(X)
        c.set_temper(0.5)
        with pytest.raises(bm.BmmError, match="tempered") as e:
            c.set_summary()
        assert e.value.code == 2
    unarmed_is_unchanged()
