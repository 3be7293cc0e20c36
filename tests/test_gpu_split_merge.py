"""Split-merge moves of the DP chain on the device (include/bmm_mcmc.h "split-merge moves")
against the NumPy restatement (tests/split_merge_ref.py) and against the exact posterior by enumeration."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_merge_cases as cases  # noqa: E402
import split_merge_checks as chk  # noqa: E402
import split_merge_ref as ref  # noqa: E402
from test_split_merge_ref import seven_observations  # noqa: E402

pytestmark = pytest.mark.gpu

# the one source of the replayed chains' constants and data, shared with the CPU pre-check of the cases
ALPHA, BETA, GAMMA = cases.ALPHA, cases.BETA, cases.GAMMA
_mixture = cases.mixture


@pytest.fixture(scope="module")
def bmm():
    import importlib
    return importlib.import_module("bmm-mcmc_amd")


def _recount(X, z1, K):
    z = np.asarray(z1) - 1
    Nk = np.bincount(z, minlength=K).astype(np.int32)
    S = np.zeros((K, X.shape[1]), dtype=np.int32)
    np.add.at(S, z, X)
    return Nk, S


def _integer_parts(c, d, r, z_before):
    """the parts of a device step that are pure functions of seed, counters and labels, against the restatement's,
    exactly; False for a skipped move (which must have changed nothing)"""
    assert d["rows"] == r["rows"] and d["kind"] == r["kind"]
    assert d["log_u"] == pytest.approx(r["log_u"], abs=4 * chk.EPS * max(1.0, abs(r["log_u"])))
    if d["kind"] == "skipped":
        np.testing.assert_array_equal(c.labels(), z_before)
        return False
    assert d["labels"] == (r["labels"][0] + 1, r["labels"][1] + 1)
    assert d["members"] == r["members"] and d["n_before"] == r["n_before"] and d["n_after"] == r["n_after"]
    np.testing.assert_array_equal(d["launch_side"], r["launch_side"])
    np.testing.assert_array_equal(d["proposal_side"], r["proposal_side"])
    return True


def _replay(bmm, N, P, K, scans, X, seed, prepare=None):
    """cases.SWEEPS sweeps at batch cases.BATCH, `prepare(chain)` if given, then 40 manual moves (or, `scans` a tuple
    of (scans, steps) phases, the steps of every phase on the one chain), each against the restatement fed with the
    labels before it.  Returns what split_merge_cases.check_reached wants to see of every move."""
    phases = ((scans, 40),) if isinstance(scans, int) else tuple(scans)
    total = sum(n for _, n in phases)
    worst = {"log_prior": 0.0, "log_lik": 0.0, "log_q": 0.0}
    seen = []
    with bmm.Chain("dp", N, P, K, alpha=ALPHA, beta=BETA, gamma=GAMMA, batch=cases.BATCH, seed=seed) as c:
        c.set_data(X)
        c.sweeps(cases.SWEEPS)
        if prepare is not None:
            prepare(c)
        kinds = set()
        done = 0  # moves made so far, over all phases: the move counter of the next one
        for phase_scans, n_steps in phases:
            c.set_split_merge(1, phase_scans)  # the scans of the manual moves ...
            c.set_split_merge(0, phase_scans)  # ... and nothing armed
            for _ in range(n_steps):
                step, done = done, done + 1
                z_before = c.labels()
                d = c.split_merge_step(sides=True)
                assert (d["sweep"], d["move"]) == (cases.SWEEPS + 1, step)
                r = ref.move(X, z_before - 1, K, ALPHA, BETA, GAMMA, phase_scans, ref.PhiloxDraws(seed, d["sweep"], d["move"]))
                kinds.add(d["kind"])
                seen.append((d["kind"], d["labels"], d["members"], d["launch_side"]))
                # the integer parts, exactly
                if not _integer_parts(c, d, r, z_before):
                    continue
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
                for key, b in (("log_prior", bound), ("log_lik", bound), ("log_q", bound_q)):
                    if b > 0.0:
                        worst[key] = max(worst[key], abs(d[key] - r[key]) / b)
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
        assert done == total and {"split", "merge"} <= kinds
        st = c.split_merge_stats()
        assert st["split_proposed"] + st["merge_proposed"] + st["skipped"] == total
    print("N=%d P=%d K=%d scans=%s: worst error as a share of its bound: log_prior %.3g, log_lik %.3g, log_q %.3g"
          % (N, P, K, [s for s, _ in phases], worst["log_prior"], worst["log_lik"], worst["log_q"]))
    return seen


def _replay_case(bmm, case):
    prepare = None
    if case.plant is not None:
        def prepare(c):
            z0 = case.plant(case.N)
            c.set_labels(z0)
            np.testing.assert_array_equal(c.labels(), z0)
    seen = _replay(bmm, case.N, case.P, case.K, cases.scans_of(case), cases.data(case), case.seed, prepare)
    assert len(seen) == cases.steps_of(case)
    cases.check_reached(case, seen)


@pytest.mark.parametrize("P", [37, 130])
def test_step_diagnostics_against_the_restatement(bmm, P):
    case = cases.BY_NAME["original-P%d" % P]
    assert (case.N, case.K, case.phases, case.seed, case.data_seed) == (300, 8, ((2, 40),), 17, 4)
    _replay_case(bmm, case)


# the shapes past one trip of the kernels' loops (tests/split_merge_cases.py says what each one reaches, and
# tests/test_split_merge_cases.py that the restatement alone gets there with the case's seed).  The side bytes of every
# member are compared exactly: no member of any case has so far drawn a uniform within rounding of exp(lp0).
@pytest.mark.parametrize("name", [c.name for c in cases.CASES if not c.name.startswith("original")])
def test_step_diagnostics_past_one_trip_of_the_loops(bmm, name):
    _replay_case(bmm, cases.BY_NAME[name])


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
    Xw, _ = _mixture(64, 1025, [0.3, 0.7], 1)
    with bmm.Chain("dp", 64, 1025, 5, alpha=1.0, seed=1) as c:  # one feature past the 1024 the moves are offered for
        c.set_data(Xw)
        c.sweeps(1)
        for call in (lambda: c.set_split_merge(1, 2), lambda: c.split_merge(1), lambda: c.split_merge_step()):
            with pytest.raises(_capi.BmmError) as e:
                call()
            assert e.value.code == 2 and "1024" in str(e.value)
        c.sweeps(1)                            # and the chain still sweeps
        assert c.sweep_index == 2
        Nk, S = c.counts()
        Nk_ref, S_ref = _recount(Xw, c.labels(), 5)
        np.testing.assert_array_equal(Nk, Nk_ref)
        np.testing.assert_array_equal(S, S_ref)
    with bmm.Chain("stickbreaking", 64, 8, 5, alpha=1.0, seed=1) as c:
        with pytest.raises(_capi.BmmError) as e:
            c.set_split_merge(1, 2)
        assert e.value.code == 2
        c.set_shard(128, 0)
        with pytest.raises(_capi.BmmError) as e:
            c.set_split_merge(1, 2)
        assert e.value.code == 5  # a sharded chain
