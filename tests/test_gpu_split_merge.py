"""Split-merge moves of the DP chain on the device (include/bmm_mcmc.h "split-merge moves")
against the NumPy restatement (tests/split_merge_ref.py) and against the exact posterior by enumeration."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_merge_checks as chk  # noqa: E402
import split_merge_ref as ref  # noqa: E402
from test_split_merge_ref import seven_observations  # noqa: E402

pytestmark = pytest.mark.gpu

BETA = GAMMA = 0.5
ALPHA = 1.3


@pytest.fixture(scope="module")
def bmm():
    import importlib
    return importlib.import_module("bmm-mcmc_amd")


def _mixture(N, P, thetas, seed):
    rng = np.random.default_rng(seed)
    comp = rng.integers(len(thetas), size=N)
    X = (rng.random((N, P)) < np.asarray(thetas)[comp][:, None]).astype(np.int32)
    return np.asfortranarray(X), comp


def _recount(X, z1, K):
    z = np.asarray(z1) - 1
    Nk = np.bincount(z, minlength=K).astype(np.int32)
    S = np.zeros((K, X.shape[1]), dtype=np.int32)
    np.add.at(S, z, X)
    return Nk, S


@pytest.mark.parametrize("P", [37, 130])
def test_step_diagnostics_against_the_restatement(bmm, P):
    N, K, scans, seed = 300, 8, 2, 17
    X, _ = _mixture(N, P, [0.2, 0.5, 0.8], 4)
    with bmm.Chain("dp", N, P, K, alpha=ALPHA, beta=BETA, gamma=GAMMA, batch=16, seed=seed) as c:
        c.set_data(X)
        c.sweeps(3)
        c.set_split_merge(1, scans)  # the scans of the manual moves ...
        c.set_split_merge(0, scans)  # ... and nothing armed
        kinds = set()
        for step in range(40):
            z_before = c.labels()
            d = c.split_merge_step(sides=True)
            assert (d["sweep"], d["move"]) == (4, step)
            r = ref.move(X, z_before - 1, K, ALPHA, BETA, GAMMA, scans, ref.PhiloxDraws(seed, d["sweep"], d["move"]))
            kinds.add(d["kind"])
            # the integer parts, exactly
            assert d["rows"] == r["rows"] and d["kind"] == r["kind"]
            assert d["log_u"] == pytest.approx(r["log_u"], abs=4 * chk.EPS * max(1.0, abs(r["log_u"])))
            if d["kind"] == "skipped":
                np.testing.assert_array_equal(c.labels(), z_before)
                continue
            assert d["labels"] == (r["labels"][0] + 1, r["labels"][1] + 1)
            assert d["members"] == r["members"] and d["n_before"] == r["n_before"] and d["n_after"] == r["n_after"]
            np.testing.assert_array_equal(d["launch_side"], r["launch_side"])
            np.testing.assert_array_equal(d["proposal_side"], r["proposal_side"])
            # the three sums.  Bound: every lgamma_ term is within LGAMMA_ULPS ulps of max(1, |term|), the log within
            # LOG_ULPS, and adding n terms in binary64 loses at most n ulps of the sum of their magnitudes; scipy's own
            # error is taken as no larger than lgamma_'s.  So |difference| <= 2 (LGAMMA_ULPS + n) eps (sum |terms| + n).
            tot, n = r["abs_terms"]
            bound = 2.0 * (chk.LGAMMA_ULPS + n) * chk.EPS * (tot + n)
            print("step %d %s: log_prior %.3e log_lik %.3e (bound %.3e)" % (step, d["kind"], abs(d["log_prior"] - r["log_prior"]),
                                                                           abs(d["log_lik"] - r["log_lik"]), bound))
            assert abs(d["log_prior"] - r["log_prior"]) <= bound
            assert abs(d["log_lik"] - r["log_lik"]) <= bound
            # log q: per member 4 P + 2 logs of magnitude below log(bg + N) + |log prior| each, a difference and a sum per
            # feature, then exp and log of the draw (1 ulp each on a value below 1 + |diff|)
            m = d["members"]
            per_member = (4 * P + 8) * (chk.LOG_ULPS + 2.0) * chk.EPS * (math.log(BETA + GAMMA + N) + abs(math.log(BETA)) + 1.0) * 2.0
            bound_q = m * per_member + m * chk.EPS * max(1.0, abs(r["log_q"]))
            print("         log_q %.3e (bound %.3e)" % (abs(d["log_q"] - r["log_q"]), bound_q))
            assert abs(d["log_q"] - r["log_q"]) <= bound_q
            # the decision, on the device's own numbers
            sign = -1.0 if d["kind"] == "split" else 1.0
            assert d["log_r"] == (d["log_prior"] + d["log_lik"]) + sign * d["log_q"]
            assert d["accepted"] == (d["log_u"] < d["log_r"])
            # the state afterwards
            z_after = c.labels()
            Nk, S = c.counts()
            Nk_ref, S_ref = _recount(X, z_after, K)
            np.testing.assert_array_equal(Nk, Nk_ref)
            np.testing.assert_array_equal(S, S_ref)
            outside = d["launch_side"] == 255
            np.testing.assert_array_equal(z_after[outside], z_before[outside])
            if d["accepted"] == r["accepted"]:
                np.testing.assert_array_equal(z_after - 1, r["z"])
            if not d["accepted"]:
                np.testing.assert_array_equal(z_after, z_before)
        assert {"split", "merge"} <= kinds
        st = c.split_merge_stats()
        assert st["split_proposed"] + st["merge_proposed"] + st["skipped"] == 40


def test_lgamma_on_the_device_is_bit_equal_to_the_host_build(bmm, tmp_path):
    import ctypes as C
    _capi = sys.modules["bmm-mcmc_amd"]._capi
    x = chk.lgamma_arguments()
    out = np.zeros_like(x)
    _capi.check(_capi.lib().bmm_device_math(0, 5, _capi.vp(x), None, _capi.vp(out), C.c_int64(len(x))))
    host = chk.lgamma_host(chk.build_lgamma_host(tmp_path), x, tmp_path)
    np.testing.assert_array_equal(out.view(np.uint64), host.view(np.uint64))
    assert chk.lgamma_error_ulps(out, x).max() <= chk.LGAMMA_ULPS


@pytest.fixture(scope="module")
def enumeration():
    X = seven_observations()
    parts, w = chk.exact_posterior(X, ALPHA, BETA, GAMMA)
    return np.asfortranarray(X), parts, w


@pytest.mark.parametrize("scans", [0, 2])
def test_moves_alone_sample_the_exact_posterior(bmm, enumeration, scans):
    X, parts, w = enumeration
    with bmm.Chain("dp", 7, 3, 30, alpha=ALPHA, beta=BETA, gamma=GAMMA, batch=1, seed=101 + scans) as c:
        c.set_data(X)
        c.sweeps(1)
        c.set_split_merge(1, scans)
        c.set_split_merge(0, scans)
        visited = []
        for _ in range(50_000):
            c.split_merge(1)
            visited.append(ref.canon(c.labels()))
        st = c.split_merge_stats()
        assert st["skipped"] == 0 and st["split_accepted"] > 1000 and st["merge_accepted"] > 1000
    chk.check_against_enumeration(visited, parts, w)


def test_batch_1_sweeps_with_two_moves_each_sample_the_exact_posterior(bmm, enumeration):
    X, parts, w = enumeration
    out = bmm.gibbs_dp(X, 25_001, alpha=ALPHA, beta=BETA, gamma=GAMMA, burnin=1, maxK=30, batch=1, seed=9, split_merge=2,
                       split_merge_scans=2)
    st = out["split_merge"]
    assert st["split_proposed"] + st["merge_proposed"] + st["skipped"] == 2 * (25_001 - 2)
    chk.check_against_enumeration([ref.canon(row) for row in out["z"]], parts, w)


PLANT_SCANS = 2


def _planted(kind, rng, comp):
    if kind == "cut":   # one component cut at random into two labels: the move must merge them
        return np.where(comp == 0, 1 + rng.integers(2, size=len(comp)), 3).astype(np.int32)
    return np.ones(len(comp), dtype=np.int32)  # both components under one label: the move must split it


def _agrees(z1, comp):
    labels = np.unique(z1)
    if len(labels) != 2:
        return False
    a = np.mean((z1 == labels[0]) == (comp == 0))
    return max(a, 1.0 - a) >= 0.999


@pytest.mark.parametrize("kind", ["cut", "one"])
def test_planted_states_are_repaired_within_400_moves(bmm, kind):
    N, P = 4096, 32
    X, comp = _mixture(N, P, [0.15, 0.85], 8)
    z0 = _planted(kind, np.random.default_rng(2), comp)
    # the restatement gets there with these scans (the choice of PLANT_SCANS): moves only, on the CPU
    zr = z0.astype(np.int64) - 1
    rng = np.random.default_rng(1)
    ok = False
    for _ in range(400):
        r = ref.move(X, zr, 30, 1.0, BETA, GAMMA, PLANT_SCANS, ref.RngDraws(rng))
        ok = ok or (r["accepted"] and r["kind"] == ("merge" if kind == "cut" else "split"))
        zr = r["z"]
    assert ok and _agrees(zr + 1, comp)
    with bmm.Chain("dp", N, P, 30, alpha=1.0, beta=BETA, gamma=GAMMA, seed=5) as c:
        c.set_data(X)
        c.sweeps(1)
        c.set_labels(z0)
        np.testing.assert_array_equal(c.labels(), z0)
        Nk, S = c.counts()
        Nk_ref, S_ref = _recount(X, z0, 30)
        np.testing.assert_array_equal(Nk, Nk_ref)
        np.testing.assert_array_equal(S, S_ref)
        c.set_split_merge(1, PLANT_SCANS)
        c.set_split_merge(0, PLANT_SCANS)
        c.split_merge(400)
        st = c.split_merge_stats()
        assert st["merge_accepted" if kind == "cut" else "split_accepted"] >= 1
        z = c.labels()
        assert _agrees(z, comp)
        Nk, S = c.counts()
        Nk_ref, S_ref = _recount(X, z, 30)
        np.testing.assert_array_equal(Nk, Nk_ref)
        np.testing.assert_array_equal(S, S_ref)


def test_no_free_label_is_counted_as_skipped_and_changes_nothing(bmm):
    N, P = 500, 20
    X, comp = _mixture(N, P, [0.2, 0.8], 3)
    with bmm.Chain("dp", N, P, 2, alpha=1.0, beta=BETA, gamma=GAMMA, seed=1) as c:
        c.set_data(X)
        c.sweeps(1)
        c.set_labels((comp + 1).astype(np.int32))
        z0, (Nk0, S0) = c.labels(), c.counts()
        skipped = 0
        for _ in range(30):
            d = c.split_merge_step()
            same = z0[d["rows"][0]] == z0[d["rows"][1]]
            assert (d["kind"] == "skipped") == same or d["accepted"]
            if d["accepted"]:
                break  # a merge went through: labels are no longer both in use
            skipped += d["kind"] == "skipped"
            np.testing.assert_array_equal(c.labels(), z0)
        assert skipped >= 1 and c.split_merge_stats()["skipped"] == skipped
        if not d["accepted"]:
            Nk, S = c.counts()
            np.testing.assert_array_equal(Nk, Nk0)
            np.testing.assert_array_equal(S, S0)


def test_same_seed_same_bits(bmm):
    N, P = 1500, 45
    X, _ = _mixture(N, P, [0.2, 0.5, 0.8], 6)
    runs = []
    for _ in range(2):
        with bmm.Chain("dp", N, P, 20, alpha=1.0, beta=BETA, gamma=GAMMA, seed=77) as c:
            c.set_data(X)
            c.set_split_merge(3, 2)
            c.sweeps(6)
            d = c.split_merge_step()
            runs.append((c.labels(), c.counts(), c.split_merge_stats(), d))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1][0], runs[1][1][0])
    np.testing.assert_array_equal(runs[0][1][1], runs[1][1][1])
    assert runs[0][2] == runs[1][2] and runs[0][2]["split_proposed"] + runs[0][2]["merge_proposed"] > 0
    assert runs[0][3] == runs[1][3]  # log_q and the rest, bit for bit


def test_whole_route_records_theta_and_labels_that_belong_together(bmm):
    N, P, K = 600, 24, 30
    X, _ = _mixture(N, P, [0.2, 0.8], 12)
    out = bmm.gibbs_dp(X, 60, alpha=1.0, beta=BETA, gamma=GAMMA, maxK=K, seed=4, split_merge=2)
    st = out["split_merge"]
    assert st["split_proposed"] + st["merge_proposed"] + st["skipped"] == 2 * 58
    for s in range(out["z"].shape[0]):
        Nk, S = _recount(X, out["z"][s], K)
        want = np.where(Nk[:, None] > 0, S / np.maximum(Nk, 1)[:, None], 0.0)
        np.testing.assert_array_equal(out["theta"][:, :, s], want)
    with pytest.raises(ValueError):
        bmm.gibbs_dp(X, 10, alpha=1.0, maxK=K, seed=4, split_merge=2, chains=2)


def test_refusals(bmm):
    _capi = sys.modules["bmm-mcmc_amd"]._capi
    X, _ = _mixture(64, 8, [0.3, 0.7], 1)
    with bmm.Chain("collapsed", 64, 8, 3, alpha=1.0, seed=1) as c:
        c.set_data(X)
        with pytest.raises(_capi.BmmError) as e:
            c.set_split_merge(1, 2)
        assert e.value.code == 2  # BMM_E_UNSUPPORTED
        with pytest.raises(_capi.BmmError) as e:
            c.set_labels(np.ones(64, dtype=np.int32))
        assert e.value.code == 2
    with bmm.Chain("dp", 64, 8, 5, alpha=1.0, seed=1, x_layout="int32") as c:
        c.set_data(X)
        c.sweeps(1)
        with pytest.raises(_capi.BmmError) as e:
            c.split_merge(1)
        assert e.value.code == 2
    with bmm.Chain("dp", 64, 8, 5, alpha=1.0, seed=1) as c:
        c.set_data(X)
        for call in (lambda: c.split_merge(1), lambda: c.split_merge_step(), lambda: c.set_labels(np.ones(64, dtype=np.int32))):
            with pytest.raises(_capi.BmmError) as e:
                call()
            assert e.value.code == 5  # BMM_E_STATE: unseated
        c.sweeps(1)
        bad = np.ones(64, dtype=np.int32)
        bad[10] = 6
        z0 = c.labels()
        with pytest.raises(_capi.BmmError) as e:
            c.set_labels(bad)
        assert e.value.code == 1 and "z[10]" in str(e.value)
        np.testing.assert_array_equal(c.labels(), z0)
    with bmm.Chain("stickbreaking", 64, 8, 5, alpha=1.0, seed=1) as c:
        with pytest.raises(_capi.BmmError) as e:
            c.set_split_merge(1, 2)
        assert e.value.code == 2
        c.set_shard(128, 0)
        with pytest.raises(_capi.BmmError) as e:
            c.set_split_merge(1, 2)
        assert e.value.code == 5  # a sharded chain
