"""ECR relabelling on the device (include/bmm_mcmc.h "ECR") held to the NumPy restatement
tests/ecr_ref.py.  Everything is an integer, so everything is compared exactly: permutations, agreements, tables,
the relabelled trace, the pivot, the iteration count and the convergence flag -- in every form of the kernels (the
cases are ecr_ref.CASES; tests/test_ecr_ref.py proves they reach every form and converge in the restatement), through
a run of each of the four samplers, and across several chains."""
import numpy as np
import pytest

import bmm_mcmc_amd as bm
import ecr_ref as E
from util import load_dataset, synth

pytestmark = pytest.mark.gpu


def _same(got, want, with_tables=True):
    assert np.array_equal(got["permutations"], want["permutations"])
    assert np.array_equal(got["agree"], want["agree"]) and got["agree"].dtype == np.int64
    assert np.array_equal(got["pivot"], want["pivot"] + 1)
    assert np.array_equal(got["z"], want["z"] + 1)
    assert got["iterations"] == want["iterations"] and got["converged"] == want["converged"]
    if with_tables:
        assert got["tables"].dtype == np.uint32 and np.array_equal(got["tables"], want["tables"])


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_every_form_against_the_restatement(case):
    z, pivot, want = E.solved(case)
    assert want["converged"]
    got = bm.ecr_relabel(z + 1, case["K"], None if pivot is None else pivot + 1, tables=True)
    _same(got, want)
    assert all(sorted(p) == list(range(case["K"])) for p in got["permutations"])
    assert np.array_equal(got["agree"], (got["z"] == got["pivot"][None, :]).sum(axis=1))


@pytest.mark.parametrize("case", [E.CASES[5], E.CASES[14], E.CASES[17]], ids=E.case_id)
def test_the_same_call_twice_gives_the_same_bytes(case):
    z, pivot, _ = E.solved(case)
    a = bm.ecr_relabel(z + 1, case["K"], None if pivot is None else pivot + 1, tables=True)
    b = bm.ecr_relabel(z + 1, case["K"], None if pivot is None else pivot + 1, tables=True)
    for k in ("permutations", "agree", "pivot", "z", "tables"):
        assert a[k].tobytes() == b[k].tobytes()
    assert (a["iterations"], a["converged"]) == (b["iterations"], b["converged"])


def test_max_iter_caps_the_loop_and_theta_follows():
    case = E.CASES[5]
    z, _, _ = E.solved(case)
    want = E.ecr(z, case["K"], None, max_iter=1)
    S, K = z.shape[0], case["K"]
    theta = np.random.default_rng(1).random((K, 4, S))
    got = bm.ecr_relabel(z + 1, K, max_iter=1, theta=theta, tables=True)
    _same(got, want)
    assert got["iterations"] == 1 and not got["converged"]
    for s in range(S):
        assert np.array_equal(got["theta"][got["permutations"][s], :, s], theta[:, :, s])


def test_bad_input_is_refused_naming_the_cause():
    z = np.asfortranarray(np.random.default_rng(0).integers(1, 4, (5, 40)), dtype=np.int32)
    bad = z.copy(order="F")
    bad[2, 7] = 0
    with pytest.raises(bm.BmmError, match=r"label 0 at row 2, observation 7") as e:
        bm.ecr_relabel(bad, 3)
    assert e.value.code == 1
    bad[2, 7] = 4
    with pytest.raises(bm.BmmError, match=r"label 4 at row 2, observation 7.*outside 1 \.\. 3") as e:
        bm.ecr_relabel(bad, 3)
    assert e.value.code == 1
    with pytest.raises(bm.BmmError, match=r"K must be in 1 \.\. 128 \(got 129\)") as e:
        bm.ecr_relabel(z, 129)
    assert e.value.code == 1
    with pytest.raises(bm.BmmError, match=r"max_iter must be >= 1") as e:
        bm.ecr_relabel(z, 3, max_iter=0)
    assert e.value.code == 1
    pv = np.ones(40, dtype=np.int32)
    pv[11] = 9
    with pytest.raises(bm.BmmError, match=r"pivot label 9 at observation 11") as e:
        bm.ecr_relabel(z, 3, pivot=pv)
    assert e.value.code == 1
    assert bm.ecr_relabel(z, 3, pivot=np.ones(40, dtype=np.int32), max_iter=0)["iterations"] == 1  # no loop to cap


# ---- through a run ---------------------------------------------------------------------------------------------------
N_RUN, P_RUN = 2003, 12
SAMPLERS = {
    "collapsed": (lambda X, **kw: bm.gibbs_collapsed(X, 30, 4, **kw), 4),
    "dp": (lambda X, **kw: bm.gibbs_dp(X, 30, maxK=8, **kw), 8),
    "stickbreaking": (lambda X, **kw: bm.gibbs_stickbreaking(X, 30, 6, **kw), 6),
    "full": (lambda X, **kw: bm.gibbs_full(X, 30, 4, **kw), 4),
}


@pytest.fixture(scope="module")
def data():
    X, labels, _, _ = synth(N_RUN, P_RUN, 3, 11)
    return X, (labels + 1).astype(np.int32)


@pytest.mark.parametrize("burnin,pivot", [(0, "iterative"), (5, "partition"), (0, "given"), (0, "partition")])
@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_a_run_equals_the_stand_alone_call_on_its_trace(data, sampler, burnin, pivot):
    X, truth = data
    run, K = SAMPLERS[sampler]
    kw = dict(burnin=burnin, seed=77)
    if pivot == "partition":
        kw["partition"] = "binder"
    plain = run(X, **kw)
    out = run(X, relabel="ecr", ecr_pivot=truth if pivot == "given" else pivot, **kw)
    S = 30 - burnin
    assert out["z_original"].tobytes() == plain["z"].tobytes()
    assert out["theta_original"].tobytes() == plain["theta"].tobytes()
    assert out["alpha"].tobytes() == plain["alpha"].tobytes()
    first = 1 if burnin == 0 and sampler != "collapsed" else 0
    ecr = out["ecr"]
    assert ecr["n_used"] == S - first
    if first:
        assert np.array_equal(out["permutations"][0], np.arange(K)) and ecr["agree"][0] == 0
        assert np.array_equal(out["z"][0], out["z_original"][0])
    pv = {"iterative": None, "partition": out["partition"]["z"] if pivot == "partition" else None, "given": truth}[pivot]
    alone = bm.ecr_relabel(out["z_original"][first:], K, pv)
    assert np.array_equal(out["permutations"][first:], alone["permutations"])
    assert np.array_equal(out["z"][first:], alone["z"])
    assert np.array_equal(ecr["agree"][first:], alone["agree"])
    assert np.array_equal(ecr["pivot"], alone["pivot"])
    assert (ecr["iterations"], ecr["converged"]) == (alone["iterations"], alone["converged"])
    assert ecr["converged"]
    th, th0, pm = out["theta"], out["theta_original"], out["permutations"]
    for s in range(S):
        assert th[pm[s], :, s].tobytes() == th0[:, :, s].tobytes()
    # ... and the stand-alone call equals the restatement on the same trace
    want = E.ecr(out["z_original"][first:] - 1, K, None if pv is None else pv - 1)
    _same(alone, want, with_tables=False)


@pytest.mark.parametrize("pivot", ["iterative", "partition"])
@pytest.mark.parametrize("sampler", ["collapsed", "dp", "full"])
def test_several_chains_share_one_pivot(data, sampler, pivot):
    X, _ = data
    run, K = SAMPLERS[sampler]
    kw = dict(burnin=8, seed=5, chains=3)
    if pivot == "partition":
        kw["partition"] = "vi"
    plain = run(X, **kw)
    outs = run(X, relabel="ecr", ecr_pivot=pivot, **kw)
    assert len(outs) == 3
    for o, p in zip(outs, plain):
        assert o["z_original"].tobytes() == p["z"].tobytes() and o["theta_original"].tobytes() == p["theta"].tobytes()
    stacked = np.concatenate([o["z_original"] for o in outs], axis=0)
    pv = outs[0]["partition"]["z"] if pivot == "partition" else None
    alone = bm.ecr_relabel(stacked, K, pv)
    S = 22
    for c, o in enumerate(outs):
        assert np.array_equal(o["permutations"], alone["permutations"][c * S:(c + 1) * S])
        assert np.array_equal(o["z"], alone["z"][c * S:(c + 1) * S])
        assert np.array_equal(o["ecr"]["agree"], alone["agree"][c * S:(c + 1) * S])
        assert np.array_equal(o["ecr"]["pivot"], alone["pivot"])
        assert o["ecr"]["iterations"] == alone["iterations"] and o["ecr"]["converged"] == alone["converged"]
        assert o["ecr"]["n_used"] == 3 * S
        for s in range(S):
            assert o["theta"][o["permutations"][s], :, s].tobytes() == o["theta_original"][:, :, s].tobytes()


def test_refusals(data):
    X, _ = data
    with pytest.raises(ValueError, match="two relabellings"):
        bm.gibbs_collapsed(X, 30, 4, burnin=10, relabel="ecr", stephens="device", seed=1)
    with pytest.raises(ValueError, match="partition"):
        bm.gibbs_dp(X, 30, burnin=10, relabel="ecr", ecr_pivot="partition", seed=1)
    with pytest.raises(ValueError, match="partition"):
        bm.gibbs_full(X, 30, 4, burnin=10, relabel="ecr", ecr_pivot="partition", chains=2, seed=1)
    with pytest.raises(bm.BmmError) as e:
        bm.gibbs_allocation(X, 30, 6, burnin=10, relabel="ecr", seed=1)
    assert e.value.code == 2
    # the library's own refusals, behind the wrappers': armed by hand
    ec = bm._Ecr((bm._ECR_ITERATIVE, None, 50), X.shape[0], 4, X.shape[1], 20)
    ec.arm()
    with pytest.raises(bm.BmmError, match="two relabellings") as e:
        bm.gibbs_collapsed(X, 30, 4, burnin=10, relabel=True, stephens="device", seed=1)
    assert e.value.code == 1
    ec = bm._Ecr((bm._ECR_PARTITION, None, 50), X.shape[0], 4, X.shape[1], 20)
    ec.arm()
    with pytest.raises(bm.BmmError, match="needs an armed partition summary") as e:
        bm.gibbs_collapsed(X, 30, 4, burnin=10, seed=1)
    assert e.value.code == 1
    ec = bm._Ecr((bm._ECR_ITERATIVE, None, 0), X.shape[0], 4, X.shape[1], 20)
    ec.arm()
    with pytest.raises(bm.BmmError, match="max_iter must be >= 1") as e:
        bm.gibbs_collapsed(X, 30, 4, burnin=10, seed=1)
    assert e.value.code == 1
    # whatever a call returned, nothing stays armed: the next plain run is a plain run
    out = bm.gibbs_collapsed(X, 30, 4, burnin=10, seed=1)
    assert "ecr" not in out and "z_original" not in out
    # a run of several chains disarms it too
    ec = bm._Ecr((bm._ECR_ITERATIVE, None, 50), X.shape[0], 4, X.shape[1], 20)
    ec.arm()
    bm.gibbs_collapsed(X, 30, 4, burnin=10, seed=1, chains=2)
    before = ec.z_orig.copy()
    out = bm.gibbs_collapsed(X, 30, 4, burnin=10, seed=1)
    assert "ecr" not in out and np.array_equal(ec.z_orig, before)


def test_ecr_combines_with_the_other_options(data):
    X, _ = data
    Xn = X[:50]
    a = bm.gibbs_collapsed(X, 30, 4, burnin=5, seed=3, newdata=Xn, loo=True, init="kmodes")
    b = bm.gibbs_collapsed(X, 30, 4, burnin=5, seed=3, newdata=Xn, loo=True, init="kmodes", relabel="ecr")
    assert b["z_original"].tobytes() == a["z"].tobytes()
    assert b["predictive"]["lppd"].tobytes() == a["predictive"]["lppd"].tobytes()
    assert b["loo"]["log_cpo"].tobytes() == a["loo"]["log_cpo"].tobytes()
    a = bm.gibbs_dp(X, 30, maxK=8, burnin=5, seed=3, split_merge=2)
    b = bm.gibbs_dp(X, 30, maxK=8, burnin=5, seed=3, split_merge=2, relabel="ecr")
    assert b["z_original"].tobytes() == a["z"].tobytes() and b["split_merge"] == a["split_merge"]
    a = bm.gibbs_collapsed(X, 30, 4, burnin=5, seed=3, select_features=True)
    b = bm.gibbs_collapsed(X, 30, 4, burnin=5, seed=3, select_features=True, relabel="ecr")
    assert b["z_original"].tobytes() == a["z"].tobytes()
    assert b["features"]["gamma"].tobytes() == a["features"]["gamma"].tobytes()


def test_agreement_before_and_after_is_printed():
    """Information only: the smallest share of observations on which a kept sweep agrees with the pivot, as sampled
    and relabelled, for a K = 3 run on K3_N1000_P5."""
    X = load_dataset("K3_N1000_P5")
    out = bm.gibbs_collapsed(X, 120, 3, burnin=20, seed=9, relabel="ecr")
    N = X.shape[0]
    before = (out["z_original"] == out["ecr"]["pivot"][None, :]).sum(axis=1) / N
    after = out["ecr"]["agree"] / N
    print("K3_N1000_P5, K = 3, 100 kept sweeps, %d iterations: min agree / N as sampled %.4f, relabelled %.4f"
          % (out["ecr"]["iterations"], before.min(), after.min()))
