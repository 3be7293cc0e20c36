"""The allocation sampler on the device (include/bmm_mcmc.h "allocation sampler") against the
finite collapsed chain where the two must agree, the NumPy restatement (tests/alloc_ref.py) and the exact posterior by
enumeration."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_cases as cases  # noqa: E402
import alloc_checks as chk  # noqa: E402
import alloc_ref as ref  # noqa: E402
import split_merge_checks as smchk  # noqa: E402
from split_merge_cases import mixture  # noqa: E402
from test_split_merge_ref import seven_observations  # noqa: E402

pytestmark = pytest.mark.gpu
BETA, GAMMA = cases.BETA, cases.GAMMA


@pytest.fixture(scope="module")
def bmm():
    import importlib
    return importlib.import_module("bmm-mcmc_amd")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("alloc_host")
    return chk.build_host(d), d


def _recount(X, z1, K):
    z = np.asarray(z1) - 1
    Nk = np.bincount(z, minlength=K).astype(np.int32)
    S = np.zeros((K, X.shape[1]), dtype=np.int32)
    np.add.at(S, z, X)
    return Nk, S


# ---------------------------------------------------------------- 1. the tie to the collapsed chain
@pytest.mark.parametrize("P", cases.TIE_P)  # 130: above 128 features the sweeps run on the generic kernel
@pytest.mark.parametrize("batch", [1, 64])
def test_moves_off_and_no_label_empty_is_the_collapsed_chain_bit_for_bit(bmm, batch, P):
    """maxK = K = 4 and a = 0.25: K a = 1 and a are exact in binary, so the constants carry the bits of the collapsed
    sampler at alpha = 1 (tests/test_alloc_ref.py::test_tie_seed_keeps_every_label_occupied shows with the oracle that no
    label empties or is left with one row)."""
    N, K = cases.TIE_N, 4
    X, z0 = cases.tie_start(P)
    runs = []
    for armed in (False, True):
        with bmm.Chain("collapsed", N, P, K, alpha=0.25 if armed else 1.0, beta=BETA, gamma=GAMMA, batch=batch, seed=cases.TIE_SEED) as c:
            c.set_data(X)
            c.set_initial_labels(z0)
            if armed:
                c.set_alloc("uniform", 0)
                assert c.k() == 4 and not c.kernel_shape()["builds_own_tables"]
            rows = []
            for _ in range(8):
                c.sweeps(1)
                Nk, S = c.counts()
                assert Nk.min() > 1  # no label emptied or left with one row: there the two samplers differ by design
                rows.append((c.labels(), Nk, S))
            runs.append(rows)
    for (z_a, Nk_a, S_a), (z_b, Nk_b, S_b) in zip(*runs):
        np.testing.assert_array_equal(z_a, z_b)
        np.testing.assert_array_equal(Nk_a, Nk_b)
        np.testing.assert_array_equal(S_a, S_b)
    # theta-hat is S / Nk of equal integers; the whole route records it
    a = bmm.gibbs_collapsed(X, 9, K, alpha=1.0, beta=BETA, gamma=GAMMA, burnin=0, seed=cases.TIE_SEED, batch=batch, initial_K=z0)
    b = bmm.gibbs_allocation(X, 9, K, a=0.25, prior_k="uniform", K0=4, moves=0, beta=BETA, gamma=GAMMA, burnin=0,
                             seed=cases.TIE_SEED, batch=batch, initial_K=z0)
    np.testing.assert_array_equal(a["z"], b["z"])
    np.testing.assert_array_equal(a["theta"].view(np.uint64), b["theta"].view(np.uint64))
    assert (b["K"] == 4).all() and (b["k_used"] == 4).all()


# ---------------------------------------------------------------- 2., 3. exact posteriors by enumeration
A7 = 0.7


@pytest.fixture(scope="module")
def seven():
    return np.asfortranarray(seven_observations().astype(np.int32))


def test_open_empties_sample_the_dirichlet_multinomial_posterior(bmm, seven):
    X = seven
    parts, w, _ = ref.exact_posterior(X, 3, A7, BETA, GAMMA, ref.uniform_prior(3), fixed_K=3)
    out = bmm.gibbs_allocation(X, 30_001, 3, a=A7, prior_k="uniform", K0=3, moves=0, beta=BETA, gamma=GAMMA, burnin=1,
                               batch=1, seed=5)
    assert (out["K"] == 3).all()
    smchk.check_against_enumeration([ref.sm.canon(r) for r in out["z"]], parts, w)
    # a label that was empty is occupied again: the finite collapsed sampler gives it probability 0 for ever
    occ = np.stack([(out["z"] == k + 1).any(axis=1) for k in range(3)], axis=1)
    assert any((~occ[:-1, k] & occ[1:, k]).any() for k in range(3))


@pytest.mark.parametrize("prior", ["poisson", "uniform"])
@pytest.mark.parametrize("sweeps", [False, True])
def test_unknown_K_samples_the_exact_posterior(bmm, seven, prior, sweeps):
    X, maxK = seven, 4
    lp = ref.poisson_prior(maxK) if prior == "poisson" else ref.uniform_prior(maxK)
    np.testing.assert_allclose(bmm.log_prior_k(prior, maxK), lp, atol=1e-15)
    parts, w, pk = ref.exact_posterior(X, maxK, A7, BETA, GAMMA, lp)
    if sweeps:
        out = bmm.gibbs_allocation(X, 30_001, maxK, a=A7, prior_k=prior, K0=2, moves=1, beta=BETA, gamma=GAMMA, burnin=1,
                                   batch=1, seed=11)
        Ks, visited = out["K"], [ref.sm.canon(r) for r in out["z"]]
        st = out["moves"]
        assert st["eject_proposed"] + st["absorb_proposed"] == 30_001 - 2
        np.testing.assert_allclose(out["k_posterior"], np.bincount(Ks, minlength=maxK + 1)[1:] / len(Ks))
    else:
        Ks, visited = [], []
        with bmm.Chain("collapsed", 7, 3, maxK, alpha=A7, beta=BETA, gamma=GAMMA, batch=1, seed=13) as c:
            c.set_data(X)
            c.set_initial_labels(np.array([1, 2, 1, 2, 1, 2, 1], dtype=np.int32))
            c.set_alloc(prior, 0)
            c.set_k(2)
            for _ in range(50_000):
                c.alloc(1)
                Ks.append(c.k())
                visited.append(ref.sm.canon(c.labels()))
            st = c.alloc_stats()
        assert st["eject_accepted"] > 1000 and st["absorb_accepted"] > 1000
    chk.check_k_posterior(Ks, pk)
    smchk.check_against_enumeration(visited, parts, w)


# ---------------------------------------------------------------- 4., 5. step replay
def _replay(bmm, host, case):
    exe, tmp = host
    X, z1, lp = cases.start(case)
    N, P, maxK = case.N, case.P, case.maxK
    seen, worst = [], 0.0
    with bmm.Chain("collapsed", N, P, maxK, alpha=case.a, beta=BETA, gamma=GAMMA, seed=case.seed) as c:
        c.set_data(X)
        c.set_initial_labels(z1)
        c.set_alloc(np.exp(lp), 0, case.e)
        c.set_k(case.K0)
        assert c.k() == case.K0
        for step in range(cases.STEPS):
            z_before, K_before = c.labels(), c.k()
            d = c.alloc_step(sides=True)
            assert (d["sweep"], d["move"], d["k_before"]) == (1, step, K_before)
            h = chk.host_draws(exe, tmp, case.seed, 1, step, K_before, maxK, case.e)
            r = ref.move(X, z_before - 1, K_before, maxK, case.a, BETA, GAMMA, case.e, lp, ref.PhiloxDraws(case.seed, 1, step, pe=h["pe"]))
            # the integer parts, exactly
            assert d["kind"] == r["kind"] and d["labels"] == (r["labels"][0] + 1, r["labels"][1] + 1)
            assert d["pe_bits"] == h["pe_bits"]
            assert d["log_u"] == pytest.approx(r["log_u"], abs=4 * smchk.EPS * max(1.0, abs(r["log_u"])))
            np.testing.assert_array_equal(d["side"], r["side"])
            assert d["members"] == r["members"] and d["n_before"] == r["n_before"] and d["n_after"] == r["n_after"]
            # the sums: every lgamma_ term within LGAMMA_ULPS ulps of max(1, |term|), n additions, scipy no worse
            tot, n = r["abs_terms"]
            bound = 2.0 * (smchk.LGAMMA_ULPS + n) * smchk.EPS * (tot + n)
            print("step %d %s K=%d: log_prior %.3e log_lik %.3e log_q %.3e (bound %.3e)" % (
                step, d["kind"], K_before, abs(d["log_prior"] - r["log_prior"]), abs(d["log_lik"] - r["log_lik"]),
                abs(d["log_q"] - r["log_q"]), bound))
            for key in ("log_prior", "log_lik", "log_q"):
                assert abs(d[key] - r[key]) <= bound
                worst = max(worst, abs(d[key] - r[key]) / bound)
            assert d["log_move"] == pytest.approx(r["log_move"], abs=4 * smchk.EPS)
            # the decision, on the device's own numbers
            if d["kind"] == "eject":
                assert d["log_r"] == ((d["log_prior"] + d["log_lik"]) + d["log_move"]) - d["log_q"]
            else:
                assert d["log_r"] == ((d["log_prior"] + d["log_lik"]) - d["log_move"]) + d["log_q"]
            assert d["accepted"] == (d["log_u"] < d["log_r"])
            # the state afterwards
            z_after, K_after = c.labels(), c.k()
            assert K_after == d["k_after"] == (K_before + (1 if d["kind"] == "eject" else -1) if d["accepted"] else K_before)
            Nk, S = c.counts()
            Nk_ref, S_ref = _recount(X, z_after, maxK)
            np.testing.assert_array_equal(Nk, Nk_ref)
            np.testing.assert_array_equal(S, S_ref)
            assert z_after.max() <= K_after
            np.testing.assert_array_equal(z_after - 1, r["z_proposed"] if d["accepted"] else z_before - 1)
            seen.append(dict(r, accepted=d["accepted"]))
        st = c.alloc_stats()
        assert st["eject_proposed"] + st["absorb_proposed"] == cases.STEPS
        c.sweeps(2)  # and the chain sweeps on from there
        Nk, S = c.counts()
        Nk_ref, S_ref = _recount(X, c.labels(), maxK)
        np.testing.assert_array_equal(Nk, Nk_ref)
        np.testing.assert_array_equal(S, S_ref)
        assert c.labels().max() <= c.k()
    print("%s: worst error as a share of its bound %.3g" % (case.name, worst))
    cases.check_reached(case, z1, seen)


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_step_diagnostics_against_the_restatement(bmm, host, name):
    _replay(bmm, host, cases.BY_NAME[name])


# ---------------------------------------------------------------- 6. same seed, same bits
def test_armed_route_equals_manual_steps_and_repeats(bmm):
    N, P, maxK = 1500, 45, 12
    X, _ = mixture(N, P, [0.2, 0.5, 0.8], 6)
    z0 = np.random.default_rng(1).integers(1, 4, N).astype(np.int32)

    def run(manual):
        with bmm.Chain("collapsed", N, P, maxK, alpha=0.5, beta=BETA, gamma=GAMMA, seed=77) as c:
            c.set_data(X)
            c.set_initial_labels(z0)
            c.set_alloc("poisson", 0 if manual else 2, 1.5)
            c.set_k(3)
            for j in range(1, 7):
                if manual and j >= 2:
                    c.alloc(2)
                c.sweeps(1)
            return c.labels(), c.counts(), c.k(), c.alloc_stats()
    a, b, m = run(False), run(False), run(True)
    for x, y in ((a, b), (a, m)):
        np.testing.assert_array_equal(x[0], y[0])
        np.testing.assert_array_equal(x[1][0], y[1][0])
        np.testing.assert_array_equal(x[1][1], y[1][1])
        assert x[2:] == y[2:]
    assert a[3]["eject_proposed"] + a[3]["absorb_proposed"] == 10


@pytest.mark.parametrize("burnin", [0, 2])
def test_whole_route_twice_and_its_partition_summary(bmm, burnin):
    N, P, maxK = 600, 24, 10
    X, _ = mixture(N, P, [0.2, 0.8], 12)
    kw = dict(a=0.5, prior_k="poisson", K0=3, moves=2, beta=BETA, gamma=GAMMA, burnin=burnin, seed=4, partition="vi")
    a, b = bmm.gibbs_allocation(X, 40, maxK, **kw), bmm.gibbs_allocation(X, 40, maxK, **kw)
    for key in ("z", "K", "k_used"):
        np.testing.assert_array_equal(a[key], b[key])
    np.testing.assert_array_equal(a["theta"].view(np.uint64), b["theta"].view(np.uint64))
    assert a["moves"] == b["moves"] and sum(a["moves"][k] for k in ("eject_proposed", "absorb_proposed")) == 2 * 38
    assert a["z"].shape == (40 - burnin, N) and (a["z"].max(axis=1) <= a["K"]).all()
    if burnin == 0:
        assert a["K"][0] == 3  # trace row 0: the starting state
    for s in range(a["z"].shape[0]):  # theta-hat and the labels of a kept sweep belong together; NaN where a label is empty
        if burnin == 0 and s == 0:
            continue
        Nk, S = _recount(X, a["z"][s], maxK)
        with np.errstate(invalid="ignore", divide="ignore"):
            want = S / Nk[:, None].astype(np.float64)
        np.testing.assert_array_equal(a["theta"][:, :, s], want)
        assert a["k_used"][s] == (Nk > 0).sum()
    d = bmm.partition_distances(a["z"], criterion="vi", Kc=maxK)  # (the sums run in an order fixed by Kc: the run's is maxK)
    np.testing.assert_array_equal(a["partition"]["loss"], d["loss"])
    assert a["partition"]["best"] == d["best"]


# ---------------------------------------------------------------- 7. refusals
def test_refusals(bmm):
    _capi = sys.modules["bmm-mcmc_amd"]._capi
    X, _ = mixture(64, 8, [0.3, 0.7], 1)
    z0 = np.ones(64, dtype=np.int32)

    def code(call):
        with pytest.raises(_capi.BmmError) as e:
            call()
        return e.value.code
    with bmm.Chain("collapsed", 64, 8, 5, alpha=None, seed=1) as c:  # alpha = 0: the concentration's update
        c.set_data(X)
        c.set_initial_labels(z0)
        assert code(lambda: c.set_alloc()) == 2
    for sampler in ("dp", "stickbreaking", "full"):
        with bmm.Chain(sampler, 64, 8, 5, alpha=1.0, seed=1) as c:
            assert code(lambda: c.set_alloc()) == 2
    with bmm.Chain("collapsed", 64, 8, 5, alpha=1.0, seed=1, x_layout="int32") as c:
        c.set_data(X)
        c.set_initial_labels(z0)
        assert code(lambda: c.set_alloc()) == 2
    with bmm.Chain("collapsed", 64, 8, 65, alpha=1.0, seed=1) as c:  # maxK above 64
        c.set_data(X)
        c.set_initial_labels(z0)
        assert code(lambda: c.set_alloc()) == 2
    with bmm.Chain("collapsed", 64, 8, 5, alpha=1.0, seed=1) as c:
        assert code(lambda: c.set_alloc()) == 5   # no data, no labels: unseated
        c.set_data(X)
        assert code(lambda: c.set_alloc()) == 5
        assert code(lambda: c.alloc_step()) == 5
        c.set_initial_labels(z0)
        assert code(lambda: c.alloc_step()) == 5  # not armed
        c.set_feature_select(True, 0.5)
        assert code(lambda: c.set_alloc()) == 2   # select_features
    with bmm.Chain("collapsed", 64, 8, 5, alpha=1.0, seed=1) as c:
        c.set_data(X)
        c.set_initial_labels(z0)
        c.set_loo(True)
        assert code(lambda: c.set_alloc()) == 2   # loo
    with bmm.Chain("collapsed", 64, 8, 5, alpha=1.0, seed=1) as c:
        c.set_data(X)
        c.set_initial_labels(z0)
        c.set_newdata(X[:4])
        assert code(lambda: c.set_alloc()) == 2   # newdata
    with bmm.Chain("collapsed", 64, 8, 5, alpha=1.0, seed=1) as c:  # ... and on an armed chain
        c.set_data(X)
        c.set_initial_labels(z0)
        c.set_alloc()
        assert code(lambda: c.init_labels()) == 2  # a device start, also before the chain has started
        assert code(lambda: c.set_feature_select(True, 0.5)) == 2
        assert code(lambda: c.set_loo(True)) == 2
        assert code(lambda: c.set_newdata(X[:4])) == 2
        assert code(lambda: c.set_split_merge(1, 2)) == 2
        assert code(lambda: c.sweep_probs()) == 2  # relabel: the probability hand-off
        assert code(lambda: c.set_k(0)) == 1 and code(lambda: c.set_k(6)) == 1
        c.set_k(1)
        assert c.k() == 1
        c.sweeps(1)
    with bmm.Chain("collapsed", 64, 8, 5, alpha=1.0, seed=1) as c:
        c.set_data(X)
        c.set_initial_labels(np.full(64, 3, dtype=np.int32))
        c.set_alloc()
        assert code(lambda: c.set_k(2)) == 1       # label 3 is occupied
    c = bmm.Chain("stickbreaking", 64, 8, 5, alpha=1.0, seed=1)
    c.set_shard(128, 0)
    assert code(lambda: c.set_alloc()) == 5        # a sharded chain
    c.close()
    Xw, _ = mixture(64, 1025, [0.3, 0.7], 1)
    with bmm.Chain("collapsed", 64, 1025, 5, alpha=1.0, seed=1) as c:  # one feature past the 1024
        c.set_data(Xw)
        c.set_initial_labels(z0)
        e = None
        with pytest.raises(_capi.BmmError) as e:
            c.set_alloc()
        assert e.value.code == 2 and "1024" in str(e.value)
        c.sweeps(2)                                # and the chain still sweeps
        assert c.sweep_index == 2
        Nk, S = c.counts()
        Nk_ref, S_ref = _recount(Xw, c.labels(), 5)
        np.testing.assert_array_equal(Nk, Nk_ref)
        np.testing.assert_array_equal(S, S_ref)
    for kw, err in ((dict(maxK=65), _capi.BmmError), (dict(maxK=5, K0=6), ValueError), (dict(maxK=5, prior_k=[1, 1, 0, 1, 1]), ValueError)):
        with pytest.raises(err):
            bmm.gibbs_allocation(X, 5, kw.pop("maxK"), **kw)
    with pytest.raises(_capi.BmmError) as e:
        bmm.gibbs_allocation(Xw, 5, 5)
    assert e.value.code == 2
    # what a run is armed with: split-merge moves and a device start are refused by the run, which disarms them
    for arm in (lambda: _capi.lib().bmm_set_split_merge(1, 2), lambda: _capi.lib().bmm_set_init(1, 3)):
        _capi.check(arm())
        assert code(lambda: bmm.gibbs_allocation(X, 5, 5, seed=1)) == 2
        out = bmm.gibbs_allocation(X, 5, 5, seed=1)  # disarmed: the next run goes through
        assert out["z"].shape[1] == 64 and (out["K"] >= 1).all()
