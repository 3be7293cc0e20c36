"""Split-merge moves of the allocation sampler on the device (include/bmm_mcmc.h "split-merge moves of the allocation
sampler") against the NumPy restatement (tests/alloc_split_ref.py), the host build of the spec,
the oracle chain's sweep, logpost_state() and the exact posterior by enumeration."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_checks as achk  # noqa: E402
import alloc_ref as al  # noqa: E402
import alloc_split_cases as cases  # noqa: E402
import alloc_split_checks as chk  # noqa: E402
import alloc_split_ref as ref  # noqa: E402
import split_merge_checks as smchk  # noqa: E402
from alloc_sweep_cases import planted  # noqa: E402
from test_gpu_logpost import _accepted, _chain, _check_state, _mixture  # noqa: E402
from test_split_merge_ref import seven_observations  # noqa: E402

pytestmark = pytest.mark.gpu
BETA, GAMMA, A7 = cases.BETA, cases.GAMMA, cases.A7


@pytest.fixture(scope="module")
def bmm():
    import importlib
    return importlib.import_module("bmm_mcmc_amd")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("alloc_split_host")
    return chk.build_host(d), d


def _recount(X, z1, K):
    z = np.asarray(z1) - 1
    Nk = np.bincount(z, minlength=K).astype(np.int32)
    S = np.zeros((K, X.shape[1]), dtype=np.int32)
    np.add.at(S, z, X)
    return Nk, S


def _armed(bmm, case, batch=None):
    X, z1 = cases.start(case.name)
    c = bmm.Chain("collapsed", case.N, case.P, case.maxK, alpha=case.a, beta=case.beta, gamma=case.gamma, batch=batch, seed=case.seed)
    try:
        c.set_data(X)
        c.set_initial_labels(z1)
        c.set_alloc(np.exp(cases.log_prior_of(case)), 0)
        c.set_k(case.K0)
        c.set_alloc_split_merge(0, case.scans)  # the scans of the manual moves, nothing armed
    except BaseException:
        c.close()
        raise
    return c, X


# ---------------------------------------------------------------- 4. moves stepped by hand against the restatement
@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_step_diagnostics_against_the_restatement(bmm, host, name):
    case = cases.BY_NAME[name]
    exe, tmp = host
    lp = cases.log_prior_of(case)
    N, P, maxK = case.N, case.P, case.maxK
    seen, prior_args, prior_got = [], [], []
    worst = {"log_lik": 0.0, "log_q": 0.0}
    c, X = _armed(bmm, case)
    with c:
        for step in range(case.steps):
            z_before, K_before = c.labels(), c.k()
            d = c.alloc_split_merge_step(sides=True)
            assert (d["sweep"], d["move"], d["k_before"]) == (1, step, K_before)
            r = ref.move(X, z_before - 1, K_before, maxK, case.a, case.beta, case.gamma, lp, case.scans,
                         ref.PhiloxDraws(case.seed, 1, step), launch=None if d["kind"] == "skipped" else d["launch_side"])
            seen.append(dict(r, accepted=d["accepted"]))
            # the integer parts, exactly
            assert d["rows"] == r["rows"] and d["kind"] == r["kind"]
            assert d["labels"] == (r["labels"][0] + 1, r["labels"][1] + 1)
            assert d["log_u"] == pytest.approx(r["log_u"], abs=4 * smchk.EPS * max(1.0, abs(r["log_u"])))
            if d["kind"] == "skipped":
                assert not d["accepted"] and d["k_after"] == K_before == maxK and d["moved"] == -1
                np.testing.assert_array_equal(c.labels(), z_before)
                assert c.k() == K_before
                continue
            assert d["members"] == r["members"] and d["n_before"] == r["n_before"] and d["n_after"] == r["n_after"]
            np.testing.assert_array_equal(d["launch_side"], r["launch_side"])  # (the restated launch draw is the device's)
            np.testing.assert_array_equal(d["launch_side"], ref.move(X, z_before - 1, K_before, maxK, case.a, case.beta, case.gamma, lp, 0,
                                                                     ref.PhiloxDraws(case.seed, 1, step))["launch_side"])
            np.testing.assert_array_equal(d["proposal_side"], r["proposal_side"])
            prior_args.append(r["prior_args"])
            prior_got.append(d["log_prior"])
            # log_lik.  Bound: every lgamma_ term is within LGAMMA_ULPS ulps of max(1, |term|), and adding n terms in
            # binary64 loses at most n ulps of the sum of their magnitudes; scipy's own error is taken as no larger than
            # lgamma_'s.  So |difference| <= 2 (LGAMMA_ULPS + n) eps (sum |terms| + n): the DP move's bound.
            tot, n = r["abs_terms"]
            bound = 2.0 * (smchk.LGAMMA_ULPS + n) * smchk.EPS * (tot + n)
            # log q, as the DP move's: per member 4 P + 2 logs of magnitude below log(bg + N + a) + |log prior| each, a
            # difference and a sum per feature, then exp and log of the draw
            m = d["members"]
            mag = math.log(case.beta + case.gamma + N + case.a) + max(abs(math.log(case.beta)), abs(math.log(case.gamma)), abs(math.log(case.a))) + 1.0
            per_member = (4 * P + 8) * (smchk.LOG_ULPS + 2.0) * smchk.EPS * mag * 2.0
            bound_q = m * per_member + m * smchk.EPS * max(1.0, abs(r["log_q"]))
            print("step %d %s K=%d: log_lik %.3e (bound %.3e) log_q %.3e (bound %.3e)" % (
                step, d["kind"], K_before, abs(d["log_lik"] - r["log_lik"]), bound, abs(d["log_q"] - r["log_q"]), bound_q))
            assert abs(d["log_lik"] - r["log_lik"]) <= bound
            assert abs(d["log_q"] - r["log_q"]) <= bound_q
            worst["log_lik"] = max(worst["log_lik"], abs(d["log_lik"] - r["log_lik"]) / bound)
            if bound_q > 0.0:
                worst["log_q"] = max(worst["log_q"], abs(d["log_q"] - r["log_q"]) / bound_q)
            # the decision, on the device's own numbers, and the restatement's
            sign = -1.0 if d["kind"] == "split" else 1.0
            assert d["log_r"] == (d["log_prior"] + d["log_lik"]) + sign * d["log_q"]
            assert d["accepted"] == (d["log_u"] < d["log_r"]) == r["accepted"]
            assert (d["k_after"], d["moved"]) == (r["k_after"], r["moved"] + 1 if r["moved"] >= 0 else -1)
            # the state afterwards
            z_after = c.labels()
            np.testing.assert_array_equal(z_after - 1, r["z"])
            assert c.k() == d["k_after"] and z_after.max() <= d["k_after"]
            Nk, S = c.counts()
            Nk_ref, S_ref = _recount(X, z_after, maxK)
            np.testing.assert_array_equal(Nk, Nk_ref)
            np.testing.assert_array_equal(S, S_ref)
        st = c.alloc_split_merge_stats()
        assert st["proposed_splits"] + st["proposed_merges"] + st["skipped"] == case.steps
        assert st["skipped"] == sum(r["kind"] == ref.SKIPPED for r in seen)
        assert st["accepted_splits"] == sum(r["kind"] == ref.SPLIT and r["accepted"] for r in seen)
        assert st["accepted_merges"] == sum(r["kind"] == ref.MERGE and r["accepted"] for r in seen)
        c.sweeps(2)  # and the chain sweeps on from there
        Nk, S = c.counts()
        Nk_ref, S_ref = _recount(X, c.labels(), maxK)
        np.testing.assert_array_equal(Nk, Nk_ref)
        np.testing.assert_array_equal(S, S_ref)
        assert c.labels().max() <= c.k()
    # log_prior: the bits of the host build of the spec
    if prior_args:
        want = chk.host_prior(exe, tmp, prior_args, case.a, lp)
        np.testing.assert_array_equal(np.array(prior_got, dtype=np.float64).view(np.uint64), want)
    print("%s: worst error as a share of its bound: log_lik %.3g, log_q %.3g" % (name, worst["log_lik"], worst["log_q"]))
    cases.check_reached(case, seen)


# ---------------------------------------------------------------- 5. a sweep after an accepted move
@pytest.mark.parametrize("name,batch", [("N255-P32-maxK13", 100), ("N257-P130-maxK64", 257)])
@pytest.mark.parametrize("what", ["split", "moved-merge"])
def test_a_sweep_after_an_accepted_move_is_the_oracle_chain(bmm, oracle, name, batch, what):
    """the committed Nk, S and K feed the next table build: one sweep from the labels and the K read off the chain"""
    case = cases.BY_NAME[name]

    def wanted(r):
        return r["accepted"] and (r["kind"] == ref.SPLIT if what == "split" else (r["kind"] == ref.MERGE and r["moved"] >= 0))
    first = next(m for m, r in enumerate(cases.restated_steps(case)) if wanted(r))  # the restatement says where it is
    c, X = _armed(bmm, case, batch=batch)
    with c:
        c.alloc_split_merge(first)
        d = c.alloc_split_merge_step()
        assert d["move"] == first and d["accepted"] and d["kind"] == what.split("-")[-1] and (what == "split" or d["moved"] >= 1)
        z, K = c.labels(), c.k()
        assert K == d["k_after"]
        want = oracle.alloc(X, z, 2, case.maxK, K, case.a, case.beta, case.gamma, 0, case.seed, batch=batch, first_sweep=1)["z"][1]
        c.sweeps(1)
        got = c.labels()
        assert np.array_equal(got, want), (name, what, int((got != want).sum()))
        assert c.k() == K
        Nk, S = c.counts()
        Nk_ref, S_ref = _recount(X, got, case.maxK)
        np.testing.assert_array_equal(Nk, Nk_ref)
        np.testing.assert_array_equal(S, S_ref)


# ---------------------------------------------------------------- 6. the tie to logpost_state()
def test_an_accepted_move_changes_the_log_joint_by_what_the_step_reports(bmm):
    N, P, maxK, a = 300, 16, 6, 0.9
    lpk = bmm.log_prior_k("poisson", maxK)

    def state(c):
        return _check_state(c, "allocation", 0.5, 0.8, False, k_open=c.k(), log_prior_k=lpk)
    # a split of one label over two well separated components; a merge of two labels cut through one component
    setups = {"split": (_mixture(N, P, [0.15, 0.85], 4)[0], 1, 1), "merge": (_mixture(N, P, [0.5], 4)[0], 2, 2)}
    for kind, (X, labels, k0) in setups.items():
        with _chain(bmm, "collapsed", X, maxK, a, 0.5, 0.8, seed=9, labels=labels) as c:
            c.set_alloc("poisson", 0, 1.0)
            c.set_k(k0)
            c.set_alloc_split_merge(0, 2)
            got = _accepted(c.alloc_split_merge_step, lambda: state(c), [kind], 300)
            assert kind in got
            (r0, b0, _), d, (r1, b1, _) = got[kind]
            delta = (r1[0] + r1[1]) - (r0[0] + r0[1])
            # the labelled log joint carries no lumping factor
            lump = -math.log(d["k_before"] + 1) if kind == "split" else math.log(d["k_before"])
            want = (d["log_lik"] + d["log_prior"]) + lump
            print(kind, delta, want, b0 + b1)
            assert abs(delta - want) <= b0 + b1


# ---------------------------------------------------------------- 7. the device against the enumeration
@pytest.fixture(scope="module")
def seven():
    return np.asfortranarray(seven_observations().astype(np.int32))


@pytest.mark.parametrize("prior", ["poisson", "uniform"])
def test_sweeps_with_both_moves_sample_the_exact_posterior(bmm, seven, prior):
    X, maxK = seven, 4
    lp = al.poisson_prior(maxK) if prior == "poisson" else al.uniform_prior(maxK)
    parts, w, pk = al.exact_posterior(X, maxK, A7, BETA, GAMMA, lp)
    out = bmm.gibbs_allocation(X, 30_001, maxK, a=A7, prior_k=prior, K0=2, moves=1, beta=BETA, gamma=GAMMA, burnin=1, batch=1,
                               seed=11, split_merge=1, split_merge_scans=1)
    st = out["split_merge"]
    print(st)
    assert st["proposed_splits"] + st["proposed_merges"] + st["skipped"] == 30_001 - 2
    assert st["accepted_splits"] > 300 and st["accepted_merges"] > 300
    achk.check_k_posterior(out["K"], pk)
    smchk.check_against_enumeration([al.sm.canon(r) for r in out["z"]], parts, w)


def test_moves_alone_sample_the_states_with_no_empty_component(bmm, seven):
    X, maxK = seven, 4
    lp = al.poisson_prior(maxK)
    parts, w, pk = ref.exact_posterior_no_empty(X, maxK, A7, BETA, GAMMA, lp)
    Ks, visited = [], []
    with bmm.Chain("collapsed", 7, 3, maxK, alpha=A7, beta=BETA, gamma=GAMMA, batch=1, seed=13) as c:
        c.set_data(X)
        c.set_initial_labels(np.array([1, 2, 1, 2, 1, 2, 1], dtype=np.int32))
        c.set_alloc("poisson", 0)
        c.set_k(2)  # K = t: no empty component, and the move keeps it so
        c.set_alloc_split_merge(0, 1)
        for _ in range(30_000):
            c.alloc_split_merge(1)
            Ks.append(c.k())
            visited.append(al.sm.canon(c.labels()))
        st = c.alloc_split_merge_stats()
    print(st)
    assert all(K == max(p) + 1 for K, p in zip(Ks, visited))
    assert st["accepted_splits"] > 500 and st["accepted_merges"] > 500
    achk.check_k_posterior(Ks, pk)
    smchk.check_against_enumeration(visited, parts, w)


# ---------------------------------------------------------------- 8. routes and reproducibility
def test_the_run_equals_a_resident_chain_stepped_by_hand_and_repeats(bmm):
    N, P, maxK, S, batch = 1500, 45, 12, 12, 400
    X, _ = planted(N, P, 4, 0, 1, 0, N, 6)  # four crisp components under one label: splits are accepted
    z0 = np.ones(N, dtype=np.int32)
    kw = dict(a=0.5, prior_k="poisson", K0=1, moves=1, eject_a=1.5, beta=BETA, gamma=GAMMA, burnin=0, seed=77, batch=batch, initial_K=z0)
    a = bmm.gibbs_allocation(X, S, maxK, split_merge=2, split_merge_scans=2, **kw)
    b = bmm.gibbs_allocation(X, S, maxK, split_merge=2, split_merge_scans=2, **kw)
    for key in ("z", "K", "k_used", "theta"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["moves"] == b["moves"] and a["split_merge"] == b["split_merge"]
    st = a["split_merge"]
    assert st["proposed_splits"] + st["proposed_merges"] + st["skipped"] == 2 * (S - 2) and st["accepted_splits"] + st["accepted_merges"] > 0
    with bmm.Chain("collapsed", N, P, maxK, alpha=0.5, beta=BETA, gamma=GAMMA, batch=batch, seed=77) as c:
        c.set_data(X)
        c.set_initial_labels(z0)
        c.set_alloc("poisson", 0, 1.5)
        c.set_k(1)
        c.set_alloc_split_merge(0, 2)
        for j in range(1, S):
            if j >= 2:
                c.alloc(1)
                c.alloc_split_merge(2)
            c.sweeps(1)
            z = c.labels()
            assert np.array_equal(z, a["z"][j]), j
            assert c.k() == a["K"][j] and len(np.unique(z)) == a["k_used"][j]
        assert c.alloc_split_merge_stats() == st and c.alloc_stats() == a["moves"]
    # armed on the resident chain, the sweeps enqueue the same moves
    with bmm.Chain("collapsed", N, P, maxK, alpha=0.5, beta=BETA, gamma=GAMMA, batch=batch, seed=77) as c:
        c.set_data(X)
        c.set_initial_labels(z0)
        c.set_alloc("poisson", 1, 1.5)
        c.set_k(1)
        c.set_alloc_split_merge(2, 2)
        c.sweeps(S - 1)
        assert np.array_equal(c.labels(), a["z"][S - 1]) and c.k() == a["K"][S - 1]
        assert c.alloc_split_merge_stats() == st
    # split_merge = 0 is the call without the argument
    p, q = bmm.gibbs_allocation(X, S, maxK, split_merge=0, **kw), bmm.gibbs_allocation(X, S, maxK, **kw)
    for key in ("z", "K", "k_used", "theta"):
        assert p[key].tobytes() == q[key].tobytes(), key
    assert p["moves"] == q["moves"] and "split_merge" not in p and "split_merge" not in q
    # and with logpost= the rows of the trace are there
    r = bmm.gibbs_allocation(X, S, maxK, split_merge=2, split_merge_scans=2, logpost=True, **kw)
    assert r["z"].tobytes() == a["z"].tobytes() and "logpost" in r


def test_refusals(bmm):
    X, _ = _mixture(64, 8, [0.3, 0.7], 1)
    z0 = np.ones(64, dtype=np.int32)
    with bmm.Chain("collapsed", 64, 8, 3, alpha=1.0, seed=1) as c:
        c.set_data(X)
        c.set_initial_labels(z0)
        for call in (lambda: c.set_alloc_split_merge(1, 2), lambda: c.alloc_split_merge(1), lambda: c.alloc_split_merge_step()):
            with pytest.raises(bmm.BmmError) as e:
                call()
            assert e.value.code == 5  # BMM_E_STATE: not armed
        c.set_alloc("poisson", 0)
        with pytest.raises(bmm.BmmError) as e:  # the DP chain's moves stay refused on an armed chain
            c.set_split_merge(1, 2)
        assert e.value.code == 2
        with pytest.raises(bmm.BmmError) as e:
            c.set_alloc_split_merge(-1, 2)
        assert e.value.code == 1
    with bmm.Chain("collapsed", 64, 8, 3, alpha=1.0, seed=1) as c:  # unseated: no initial labels
        c.set_data(X)
        with pytest.raises(bmm.BmmError) as e:
            c.set_alloc_split_merge(1, 2)
        assert e.value.code == 5
    with bmm.Chain("dp", 64, 8, 5, alpha=1.0, seed=1) as c:
        c.set_data(X)
        with pytest.raises(bmm.BmmError) as e:
            c.set_alloc_split_merge(1, 2)
        assert e.value.code == 2
    with bmm.Chain("collapsed", 1, 8, 3, alpha=1.0, seed=1) as c:  # one row
        c.set_data(np.asfortranarray(X[:1]))
        c.set_initial_labels(z0[:1])
        c.set_alloc("poisson", 0)
        with pytest.raises(bmm.BmmError) as e:
            c.alloc_split_merge(1)
        assert e.value.code == 1


# ---------------------------------------------------------------- 9. the point of the feature
def test_planted_components_are_found_from_one_label_at_N_2000(bmm):
    """tests/test_alloc_split_ref.py fixes the data and the budget on the CPU: the restatement's chain ends with k_used ==
    PLANT_COMPS for all of ten seeds within half of PLANT_SWEEPS.  The device's chain is another one (default batch, other
    draws): eight of its ten must get there."""
    N, P, comps, maxK, sweeps = cases.PLANT_N, cases.PLANT_P, cases.PLANT_COMPS, cases.PLANT_MAXK, cases.PLANT_SWEEPS
    X, _ = planted(N, P, comps, 0, 1, 0, N, cases.PLANT_DATA_SEED)
    z0 = np.ones(N, dtype=np.int32)
    kw = dict(a=1.0, prior_k="poisson", K0=1, beta=BETA, gamma=GAMMA, burnin=0, initial_K=z0)
    ends, plain = [], []
    for seed in cases.PLANT_SEEDS:
        out = bmm.gibbs_allocation(X, sweeps + 1, maxK, moves=1, split_merge=2, seed=seed, **kw)
        ends.append(int(out["k_used"][-1]))
        plain.append(int(bmm.gibbs_allocation(X, sweeps + 1, maxK, moves=4, split_merge=0, seed=seed, **kw)["k_used"][-1]))
    print("k_used after %d sweeps, split_merge=2: %s; split_merge=0, moves=4: %s" % (sweeps, ends, plain))
    assert sum(k == comps for k in ends) >= 8
