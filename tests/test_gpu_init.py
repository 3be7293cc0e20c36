"""The k-modes++ initial allocation on the device (include/bmm_mcmc.h "initial allocation")
against the NumPy restatement (tests/init_ref.py): everything is integer, so every comparison is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import init_cases as cases  # noqa: E402
import init_ref as ref  # noqa: E402

import bmm_mcmc_amd as bm  # noqa: E402
from bmm_mcmc_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED, E_STATE = 1, 2, 5
ROUTE = "partial-workgroup"  # the case the route tests run on


def _collapsed(name, seed=None, batch=None):
    c = cases.BY_NAME[name]
    ch = bm.Chain("collapsed", c.N, c.P, c.K, seed=c.seed if seed is None else seed, batch=batch)
    ch.set_data(cases.data(name))
    return ch


def _same(got, labels1, want):
    assert np.array_equal(labels1 - 1, want["labels"])
    assert np.array_equal(got["rows"], want["rows"])
    assert np.array_equal(got["centres"], want["centres"])
    assert np.array_equal(got["Nk"], want["Nk"])
    for k in ("k_eff", "rounds_run", "changed_last", "cost"):
        assert got[k] == want[k], (k, got[k], want[k])


@pytest.mark.parametrize("name", cases.RUNNABLE)
def test_device_equals_restatement(name):
    case, want = cases.BY_NAME[name], cases.restated(name)
    with _collapsed(name) as ch:
        got = ch.init_labels("kmodes", centres=case.Kc, iters=case.iters)
        _same(got, ch.labels(), want)
        cases.check_reached(case, {**want, **{k: got[k] for k in ("rows", "k_eff", "rounds_run", "changed_last", "cost")}})
        ch.sweeps(1)  # the chain starts from these labels
        assert ch.counts()[0].sum() == case.N


def test_past_the_centre_limit_is_refused_and_the_chain_runs_on():
    case = cases.BY_NAME["centres-past-limit"]
    cases.check_reached(case)
    with _collapsed(case.name) as ch:
        with pytest.raises(_capi.BmmError) as e:
            ch.init_labels("kmodes", centres=case.Kc)
        assert e.value.code == E_UNSUPPORTED
        ch.set_initial_labels(np.random.default_rng(1).integers(1, case.K + 1, case.N))
        ch.sweeps(1)
        assert ch.counts()[0].sum() == case.N


def test_ties_go_to_the_lower_label():
    name = "lowest-label-ties"
    want = cases.restated(name)
    X = cases.data(name)
    with _collapsed(name) as ch:
        got = ch.init_labels("kmodes", centres=2)
        z = ch.labels() - 1
    D = ref.distances(X, got["centres"])
    tied = D[:, 0] == D[:, 1]
    assert tied.sum() == want["ties"] > 0 and np.all(z[tied] == 0)


def test_same_seed_same_bits_twice():
    out = []
    for _ in range(2):
        with _collapsed(ROUTE) as ch:
            got = ch.init_labels()
            out.append((ch.labels(), got["rows"], got["centres"], got["Nk"], got["cost"]))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("batch", [None, 64])
def test_chain_after_init_equals_chain_given_the_restated_labels(batch):
    want = cases.restated(ROUTE)
    with _collapsed(ROUTE, batch=batch) as a, _collapsed(ROUTE, batch=batch) as b:
        a.init_labels(iters=cases.BY_NAME[ROUTE].iters)
        b.set_initial_labels(want["labels"] + 1)
        for _ in range(5):
            a.sweeps(1)
            b.sweeps(1)
            assert a.labels().tobytes() == b.labels().tobytes()
            for x, y in zip(a.counts(), b.counts()):
                assert x.tobytes() == y.tobytes()
            assert np.float64(a.alpha()).tobytes() == np.float64(b.alpha()).tobytes()


def _resident_trace(name, nsamples, seed):
    """z, theta-hat inputs (counts) and alpha of the resident chain after each of nsamples - 1 sweeps"""
    with _collapsed(name, seed=seed) as ch:
        ch.init_labels()
        rows = [ch.labels()]
        alphas = [None]
        for _ in range(nsamples - 1):
            ch.sweeps(1)
            rows.append(ch.labels())
            alphas.append(ch.alpha())
    return rows, alphas


@pytest.mark.parametrize("burnin", [0, 3])
def test_run_with_init_returns_the_resident_chain(burnin):
    c = cases.BY_NAME[ROUTE]
    X = cases.data(ROUTE)
    nsamples = 6
    out = bm.gibbs_collapsed(X, nsamples, c.K, burnin=burnin, seed=c.seed, init="kmodes")
    rows, alphas = _resident_trace(ROUTE, nsamples, c.seed)
    want = cases.restated(ROUTE)
    for k in ("k_eff", "rounds_run", "changed_last", "cost"):
        assert out["init"][k] == want[k]
    given = bm.gibbs_collapsed(X, nsamples, c.K, burnin=burnin, seed=c.seed, initial_K=want["labels"] + 1)
    for s in range(nsamples - burnin):
        j = s + burnin
        assert np.array_equal(out["z"][s], rows[j])
        if j > 0:
            assert out["alpha"][s, 0] == alphas[j]
    # ... and in every kept row the z, theta and alpha of a run handed the restatement's labels
    assert out["z"].tobytes() == given["z"].tobytes()
    assert np.array_equal(out["theta"], given["theta"], equal_nan=True)
    assert np.array_equal(out["alpha"], given["alpha"])


def test_run_with_init_combines_with_loo_and_partition():
    c = cases.BY_NAME[ROUTE]
    X = cases.data(ROUTE)
    plain = bm.gibbs_collapsed(X, 6, c.K, burnin=2, seed=c.seed, init="kmodes")
    for extra in ({"loo": True}, {"partition": "vi"}):
        out = bm.gibbs_collapsed(X, 6, c.K, burnin=2, seed=c.seed, init="kmodes", **extra)
        assert out["z"].tobytes() == plain["z"].tobytes()
        assert np.array_equal(out["theta"], plain["theta"], equal_nan=True)
        assert np.array_equal(out["alpha"], plain["alpha"])
        assert out["init"]["cost"] == plain["init"]["cost"]


def test_two_chains_match_two_single_calls():
    c = cases.BY_NAME[ROUTE]
    X = cases.data(ROUTE)
    both = bm.gibbs_collapsed(X, 5, c.K, burnin=1, seed=c.seed, init="kmodes", chains=2)
    for k in range(2):
        one = bm.gibbs_collapsed(X, 5, c.K, burnin=1, seed=c.seed + k, init="kmodes")
        assert both[k]["z"].tobytes() == one["z"].tobytes()
        assert np.array_equal(both[k]["theta"], one["theta"], equal_nan=True)
        assert np.array_equal(both[k]["alpha"], one["alpha"])
        assert both[k]["init"]["cost"] == one["init"]["cost"]


def test_seated_dp_chain_takes_the_allocation_and_sweeps():
    c = cases.BY_NAME[ROUTE]
    X = cases.data(ROUTE)
    want = ref.kmodes(X, 5, c.seed, 10)
    with bm.Chain("dp", c.N, c.P, 12, alpha=1.0, seed=c.seed) as ch:
        ch.set_data(X)
        ch.sweeps(2)
        got = ch.init_labels(centres=5)
        _same(got, ch.labels(), want)
        Nk, S = ch.counts()
        wNk, wS = ref.counts(X, want["labels"], 12)
        assert np.array_equal(Nk, wNk) and np.array_equal(np.asarray(S).reshape(12, c.P), wS)
        ch.sweeps(2)
        assert ch.counts()[0].sum() == c.N


def _refused(ch, code, **kw):
    with pytest.raises(_capi.BmmError) as e:
        ch.init_labels(**kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals_and_the_chain_works_afterwards():
    """Every row of the refusals table but "a chain inside a run": a run creates, owns and destroys its chain, so no
    caller of the public interface ever holds a chain in that state, and the row cannot be reached from a test.  (The
    check is there for the library's own run path, which initialises through the internal call beneath it.)"""
    c = cases.BY_NAME[ROUTE]
    X = cases.data(ROUTE)
    z0 = np.random.default_rng(0).integers(1, c.K + 1, c.N)
    for sampler in ("stickbreaking", "full"):
        with bm.Chain(sampler, c.N, c.P, c.K, seed=1) as ch:
            ch.set_data(X)
            _refused(ch, E_UNSUPPORTED)
            ch.set_initial_params(np.full(c.K, 1.0 / c.K), np.full((c.K, c.P), 0.5))
            ch.sweeps(1)
            ch.sync()
    with bm.Chain("full", c.N, c.P, c.K, seed=1) as ch:  # sharded (one rank holding every row: nothing to all-reduce)
        ch.set_data(X)
        ch.set_shard(c.N, 0)
        _refused(ch, E_STATE)
        ch.set_initial_params(np.full(c.K, 1.0 / c.K), np.full((c.K, c.P), 0.5))
        ch.shard_resample()
        ch.shard_finish()
        ch.sync()
        assert np.all(np.isfinite(ch.params()[0]))
    with bm.Chain("collapsed", c.N, c.P, c.K, seed=1, x_layout="int32") as ch:
        ch.set_data(X)
        _refused(ch, E_UNSUPPORTED)
        ch.set_initial_labels(z0)
        ch.sweeps(1)
        assert ch.counts()[0].sum() == c.N
    with _collapsed(ROUTE) as ch:
        _refused(ch, E_ARG, centres=c.K + 1)
        _refused(ch, E_ARG, centres=-1)
        _refused(ch, E_ARG, iters=-1)
        ch.set_initial_labels(z0)
        ch.sweeps(1)
        _refused(ch, E_STATE)  # already started
        ch.sweeps(1)
        assert ch.counts()[0].sum() == c.N
    with bm.Chain("dp", c.N, c.P, 12, alpha=1.0, seed=1) as ch:
        ch.set_data(X)
        _refused(ch, E_STATE, centres=4)  # unseated
        ch.sweeps(1)
        _refused(ch, E_ARG)               # n_centres must be given
        _refused(ch, E_ARG, centres=13)
        ch.sweeps(1)
        assert ch.counts()[0].sum() == c.N


def test_armed_start_is_refused_by_the_other_runs_and_disarmed():
    c = cases.BY_NAME[ROUTE]
    X = cases.data(ROUTE)
    L = _capi.lib()
    _capi.check(L.bmm_set_init(1, 3))
    with pytest.raises(_capi.BmmError) as e:  # a DP run made while armed: refused, and the thread is disarmed
        bm.gibbs_dp(X, 3, maxK=8, seed=1)
    assert e.value.code == E_UNSUPPORTED
    plain = bm.gibbs_collapsed(X, 3, c.K, burnin=0, seed=c.seed)  # disarmed by the refused call: a random start
    again = bm.gibbs_collapsed(X, 3, c.K, burnin=0, seed=c.seed)
    assert plain["z"].tobytes() == again["z"].tobytes() and "init" not in plain


def test_python_refusals():
    c = cases.BY_NAME[ROUTE]
    X = cases.data(ROUTE)
    with pytest.raises(ValueError):
        bm.gibbs_dp(X, 3, init="kmodes")
    with pytest.raises(ValueError):
        bm.gibbs_stickbreaking(X, 3, 4, init="kmodes")
    with pytest.raises(ValueError):
        bm.gibbs_full(X, 3, 4, init="kmodes")
    with pytest.raises(ValueError):
        bm.gibbs_collapsed(X, 3, c.K, init="kmodes", initial_K=np.ones(c.N, dtype=np.int32))
    with pytest.raises(ValueError):
        bm.gibbs_collapsed(X, 3, c.K, init="kmeans")
