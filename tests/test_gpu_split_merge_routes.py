"""The armed routes of the split-merge moves tied to the manual moves that
tests/test_gpu_split_merge.py replays exactly: an armed sweep is the manual moves followed by the plain sweep, the
one-call run is the resident armed chain, and the summaries of a run (leave-one-out, predictive, point estimate)
neither disturb nor are disturbed by the moves.  Inside a run the moves ahead of sweep j work on a copy of the recorded
row j - 1, which sweep j then reads: every comparison here is byte for byte, so moves applied to the recorded row, or
not applied to what the sweep reads, show in the first kept row after an accepted move."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bmm_mcmc_amd as bm  # noqa: E402
import loo_ref as lref  # noqa: E402
import predictive_ref as pref  # noqa: E402
import split_merge_ref as ref  # noqa: E402
from test_gpu_loo import RTOL, _check_fold  # noqa: E402
from test_gpu_partition import _same_summary  # noqa: E402
from test_gpu_predict import _check_fold_lppd  # noqa: E402
from test_gpu_split_merge import _integer_parts, _recount  # noqa: E402

pytestmark = pytest.mark.gpu

BETA = GAMMA = 0.5
N, P, MAXK, MOVES, SCANS = 700, 24, 30, 3, 2
NSAMPLES = 12  # a one-call run: sweeps 1 .. 11
M_HELD = 65
# On a mixture with overlapping components (rates 0.2 / 0.5 / 0.8) no move of a chain of this size is accepted: the
# restatement, on the labels the oracle's chain holds after sweep 1, rejects all three moves ahead of sweep 2 for each
# of twelve chain seeds, and a route whose moves never change a label cannot show where they were applied.  Of six
# crisp components (every rate 0.05 or 0.95) sweep 1 leaves some under one label, and a split of such a label is
# accepted.  Chain seed 2 is the first of 29, 1, 2 for which the restatement accepts a move ahead of sweep 2 (the third
# one, a split, log r = 697) at the default batch and at batch 64 alike.
SEED = 2
# On data this crisp a chain accepts one move and is done: of the chain seeds 2, 1, 29, 3 .. 12 none accepts a second one
# within eleven sweeps.  A run with burn-in 4 lets the moves ahead of sweeps 2 .. 4 work in place, so chain seed 2 cannot
# show where its later moves were applied; chain seed 1 accepts its move ahead of sweep 5, the first one whose moves
# work on a copy of a kept row there.  (burn-in, chain seed) of the one-call runs:
RUNS = [(0, SEED), (1, SEED), (4, 1)]


def _crisp(n, seed=12):
    rng = np.random.default_rng(seed)
    rates = np.where(rng.random((6, P)) < 0.5, 0.05, 0.95)
    comp = rng.integers(6, size=n)
    return np.asfortranarray((rng.random((n, P)) < rates[comp]).astype(np.int32))


@pytest.fixture(scope="module")
def X():
    return np.asfortranarray(_crisp(N + M_HELD)[:N])


def _theta_hat(Nk, S):
    return np.where(Nk[:, None] > 0, S / np.maximum(Nk, 1)[:, None], 0.0)


def _state(c):
    Nk, S = c.counts()
    return c.labels(), Nk, S, c.alpha()


def _accepted(stats):
    return stats["split_accepted"] + stats["merge_accepted"]


def _armed(X, sweeps, batch=None, seed=SEED):
    """chain A: armed from the start, one sweep at a time; the state after every sweep, the counters at the end, and
    the sweeps ahead of which a move was accepted (from the counters after every sweep)"""
    with bm.Chain("dp", N, P, MAXK, beta=BETA, gamma=GAMMA, batch=batch, seed=seed) as c:
        c.set_data(X)
        c.set_split_merge(MOVES, SCANS)
        states, accepted_at, before = [], set(), 0
        for j in range(1, sweeps + 1):
            c.sweeps(1)
            states.append(_state(c))
            now = _accepted(c.split_merge_stats())
            if now > before:
                accepted_at.add(j)
            before = now
        return states, c.split_merge_stats(), accepted_at


@pytest.fixture(scope="module")
def residents(X):
    """chain A over the sweeps of the one-call run for every chain seed of RUNS, computed once and left unchanged:
    {seed: (states, counters, sweeps ahead of which a move was accepted)}"""
    out = {}
    for seed in sorted({seed for _, seed in RUNS}):
        states, stats, accepted_at = _armed(X, NSAMPLES - 1, seed=seed)
        assert stats["split_proposed"] + stats["merge_proposed"] + stats["skipped"] == MOVES * (NSAMPLES - 2)
        print("chain seed %d: moves accepted ahead of sweeps %s; counters %s" % (seed, sorted(accepted_at), stats))
        out[seed] = states, stats, accepted_at
    return out


@pytest.fixture(scope="module")
def resident(residents):
    states, stats, accepted_at = residents[SEED]
    assert 2 in accepted_at, accepted_at  # (as the restatement has it)
    return states, stats


def _same_state(a, b, tag):
    for x, y, what in zip(a[:3], b[:3], ("labels", "Nk", "S")):
        assert x.tobytes() == y.tobytes(), (tag, what)
    assert np.float64(a[3]).tobytes() == np.float64(b[3]).tobytes(), (tag, "alpha")


@pytest.mark.parametrize("batch", [None, 64])
def test_an_armed_sweep_is_the_manual_moves_and_then_the_plain_sweep(X, resident, batch):
    sweeps = 8
    states_a, stats_a, accepted_a = _armed(X, sweeps, batch)
    if batch is None:  # the chain the one-call runs are held to
        for j in range(sweeps):
            _same_state(states_a[j], resident[0][j], "armed twice, sweep %d" % (j + 1))
    accepted_at = set()
    with bm.Chain("dp", N, P, MAXK, beta=BETA, gamma=GAMMA, batch=batch, seed=SEED) as c:
        c.set_data(X)
        c.set_split_merge(1, SCANS)  # the scans of the manual moves ...
        c.set_split_merge(0, SCANS)  # ... and nothing armed
        if batch is not None:
            assert c.batch == batch and N > 2 * batch
        for j in range(1, sweeps + 1):
            if j >= 2:
                for m in range(MOVES):
                    z_before = c.labels()
                    alpha = c.alpha()
                    d = c.split_merge_step(sides=True)
                    assert (d["sweep"], d["move"]) == (j, m)
                    r = ref.move(X, z_before - 1, MAXK, alpha, BETA, GAMMA, SCANS, ref.PhiloxDraws(SEED, j, m))
                    if not _integer_parts(c, d, r, z_before):
                        continue
                    if d["accepted"]:
                        accepted_at.add(j)
                    if d["accepted"] == r["accepted"]:
                        np.testing.assert_array_equal(c.labels() - 1, r["z"])
                    else:  # (a log_r within rounding of log_u: never seen; the device's own decision stands)
                        print("sweep %d move %d: device %r restatement %r, log_r %r log_u %r" % (j, m, d["accepted"], r["accepted"], d["log_r"], d["log_u"]))
            c.sweeps(1)
            _same_state(_state(c), states_a[j - 1], "after sweep %d" % j)
        assert c.split_merge_stats() == stats_a
        print("batch %r: accepted moves ahead of sweeps %s; counters %s" % (batch, sorted(accepted_at), stats_a))
        assert 2 in accepted_at  # (as the restatement has it; without an accepted move the two routes could not differ)
        assert accepted_at == accepted_a


def _run(X, burnin, seed=SEED, **kw):
    return bm.gibbs_dp(X, NSAMPLES, burnin=burnin, maxK=MAXK, seed=seed, split_merge=MOVES, split_merge_scans=SCANS, **kw)


@pytest.mark.parametrize("burnin,seed", RUNS)
def test_the_one_call_run_is_the_resident_armed_chain(X, residents, burnin, seed):
    """burnin = b: the moves ahead of sweeps 2 .. b work in place, those from sweep b + 1 on a copy of a kept row"""
    states, stats, accepted_at = residents[seed]
    # the comparison can tell where the moves were applied only behind a move accepted on the copying side
    assert any(j >= max(burnin + 1, 2) for j in accepted_at), (burnin, accepted_at)
    out = _run(X, burnin, seed)
    assert out["z"].shape == (NSAMPLES - burnin, N)
    if burnin == 0:
        assert np.all(out["z"][0] == bm.NA_INTEGER)  # the unassigned starting row: no sweep stands behind it
    for j in range(max(burnin, 1), NSAMPLES):
        z, Nk, S, alpha = states[j - 1]
        s = j - burnin
        assert out["z"][s].tobytes() == z.tobytes(), "kept row %d (sweep %d)" % (s, j)
        np.testing.assert_array_equal(out["theta"][:, :, s], _theta_hat(Nk, S), err_msg="sweep %d" % j)
        assert out["alpha"][s, 0] == alpha, j
    assert out["split_merge"] == stats


@pytest.fixture(scope="module")
def held():
    return np.asfortranarray(_crisp(N + M_HELD)[N:])  # 65 more rows of the same mixture


@pytest.fixture(scope="module")
def plain(X, resident):
    return _run(X, 1)


def _chain_untouched(out, plain):
    for k in ("z", "theta", "alpha"):
        assert out[k].tobytes() == plain[k].tobytes(), k
    assert out["split_merge"] == plain["split_merge"]


def _row_state(X, out, s):
    Nk, S = _recount(X, out["z"][s], MAXK)
    return Nk, S, float(out["alpha"][s, 0])


def _check_loo(X, out, lo):
    """as test_the_fold of tests/test_gpu_loo.py, and every row of the trace against the restatement fed with the kept
    state it belongs to (as _check_state there)"""
    trace = lo["ell"]
    n = NSAMPLES - 1
    _check_fold("dp", trace, lo, n, N)
    for s in range(n):
        Nk, S, alpha = _row_state(X, out, s)
        np.testing.assert_allclose(trace[s], lref.counting_ell(X, out["z"][s], Nk, S, alpha, BETA, GAMMA, "dp"), rtol=RTOL)


def _check_predictive(X, held, out, pr):
    """as test_the_fold of tests/test_gpu_predict.py, and every row of the trace against the restatement (as
    _check_state there)"""
    n = NSAMPLES - 1
    _check_fold_lppd("dp", pr["logdens"], pr["lppd"], n, M_HELD)
    for s in range(n):
        Nk, S, alpha = _row_state(X, out, s)
        np.testing.assert_allclose(pr["logdens"][s], pref.logdens(pref.dp_terms(held, Nk, S, alpha, N, BETA, GAMMA)), rtol=RTOL)


def _check_partition(out):
    p = out["partition"]
    assert p["criterion"] == "vi" and p["n_used"] == NSAMPLES - 1
    assert np.array_equal(p["z"], out["z"][p["best"]])
    _same_summary(p, bm.partition_distances(out["z"], "vi", Kc=MAXK))


def test_the_moves_with_the_leave_one_out_summary(X, plain):
    out = _run(X, 1, loo="trace")
    _chain_untouched(out, plain)
    _check_loo(X, out, out["loo"])
    short = _run(X, 1, loo=True)
    _chain_untouched(short, plain)
    assert "ell" not in short["loo"]
    for key in short["loo"]:
        assert np.asarray(short["loo"][key]).tobytes() == np.asarray(out["loo"][key]).tobytes(), key


def test_the_moves_with_the_predictive_of_held_out_rows(X, held, plain):
    out = _run(X, 1, newdata=held, predictive_trace=True)
    _chain_untouched(out, plain)
    _check_predictive(X, held, out, out["predictive"])
    short = _run(X, 1, newdata=held)
    _chain_untouched(short, plain)
    assert short["predictive"]["lppd"].tobytes() == out["predictive"]["lppd"].tobytes()


def test_the_moves_with_the_point_estimate(X, plain):
    out = _run(X, 1, partition="vi")
    _chain_untouched(out, plain)
    _check_partition(out)


def test_the_moves_with_all_three_summaries_at_once(X, held, plain):
    out = _run(X, 1, loo="trace", newdata=held, predictive_trace=True, partition="vi")
    _chain_untouched(out, plain)
    _check_loo(X, out, out["loo"])
    _check_predictive(X, held, out, out["predictive"])
    _check_partition(out)
    alone = _run(X, 1, loo=True)["loo"]
    for key in alone:
        assert np.asarray(alone[key]).tobytes() == np.asarray(out["loo"][key]).tobytes(), key
