"""The replica ladder past one trip of its loops: exchanges at shapes that leave the first pass
and the 16-byte body of temper_swap, the refusal of a ninth rung, whole runs (`temper=`) replayed sweep by sweep by a
hand-built ladder of resident chains and compared in every kept row, and what the predictive and leave-one-out folds
of such a run see.  Full ladders and both parities of the 60-point replay, the table edges and the enumerated posterior
of three rungs are in tests/test_gpu_temper.py, whose helpers these tests use."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temper_ref as tr  # noqa: E402
import test_gpu_temper as tgt  # noqa: E402  (its chains, ladders and the whole-state exchange check)

pytestmark = pytest.mark.gpu

BETA = GAMMA = 0.5
ALPHA = 1.3
E_ARG = 1
LP_KEYS = ("log_lik", "log_prior", "log_hyper", "log_joint")


@pytest.fixture(scope="module")
def bmm():
    import importlib
    return importlib.import_module("bmm_mcmc_amd")  # (the module the dbg_lib fixture steers)


# ---------------------------------------------------------------- A. the exchange past its first trip
def _tails_differ(K, P, a, b):
    """the two states differ in the cells the scalar tails of temper_swap move: the last label, Nk[K - 1], S[K - 1, P - 1]"""
    za, zb = (np.frombuffer(s[0], dtype=np.int32) for s in (a, b))
    na, nb = (np.frombuffer(s[1], dtype=np.int32) for s in (a, b))
    sa, sb = (np.frombuffer(s[2], dtype=np.int32) for s in (a, b))
    return za[-1] != zb[-1] and na[K - 1] != nb[K - 1] and sa[K * P - 1] != sb[K * P - 1]


@pytest.mark.parametrize("accept", [True, False])
@pytest.mark.parametrize("sweeps", [0, 3])
@pytest.mark.parametrize("N,P,K", tr.SWAP_SHAPES)
def test_an_exchange_past_the_first_trip_and_the_aligned_body_of_the_swap(bmm, N, P, K, sweeps, accept):
    """tests/temper_ref.py SWAP_SHAPES says which loop of temper_swap each shape takes where; sweeps = 0: the counts
    of the starting allocation wait in all eight delta replicas.  The rejected twin (the hot rung holds the poor
    allocation at a power of 2^-10) must leave every byte in place."""
    X, z_a, z_b = tr.swap_case(N, P, K)
    chains, ladder = tgt._ladder(bmm, X, K, (1.0, tgt.NEARLY_ONE if accept else 2.0 ** -10), initials=[z_a, z_b])
    try:
        if sweeps == 0:
            a = np.float64(ALPHA).tobytes()
            before = [(z.tobytes(), None, None, a) for z in (z_a, z_b)]
        else:
            for c in chains:
                c.sweeps(sweeps)
            before = [tgt._state(c) for c in chains]
            assert _tails_differ(K, P, *before)
        rec, after = tgt._exchange_and_check(bmm, X, K, chains, ladder, before, [accept])
        print("N=%d P=%d K=%d after %d sweeps: d = %.3g, u = %.3g" % (N, P, K, sweeps, rec[0]["d"], rec[0]["u"]))
        assert rec[0]["proposed"] and (accept or rec[0]["d"] < -40.0)
        assert _tails_differ(K, P, *after)
    finally:
        tgt._close(chains, ladder)


@pytest.mark.parametrize("N,P,K", tr.SWAP_SHAPES)
def test_an_exchange_of_dp_chains_with_sampled_alpha_past_the_first_trip(bmm, N, P, K):
    X, z_a, z_b = tr.swap_case(N, P, K)
    chains, ladder = tgt._ladder(bmm, X, K, (1.0, tgt.NEARLY_ONE), sampler="dp", alpha=None)
    try:
        for c in chains:
            c.sweeps(1)
        chains[0].set_labels(z_a)     # (a DP chain takes labels between sweeps: the two states are the chosen ones)
        chains[1].set_labels(z_b)
        before = [tgt._state(c) for c in chains]
        assert before[0][0] == z_a.tobytes() and before[1][0] == z_b.tobytes()
        assert _tails_differ(K, P, *before) and before[0][3] != before[1][3]   # ... and two concentrations
        rec, after = tgt._exchange_and_check(bmm, X, K, chains, ladder, before, [True])
        assert rec[0]["proposed"] and after[0] == before[1] and after[1] == before[0]
    finally:
        tgt._close(chains, ladder)


def test_a_ninth_rung_is_refused_and_the_next_call_runs(bmm):
    assert bmm.TEMPER_MAX_RUNGS == 8
    N, P, K = 300, 8, 4
    X, _ = tr.mixture(N, P, [0.2, 0.5, 0.8], 3)
    z0 = np.random.default_rng(1).integers(1, K + 1, N).astype(np.int32)
    chains = []
    try:
        for r in range(9):
            chains.append(tgt._chain(bmm, "collapsed", X, K, None, 100 + r, initial=z0, share=chains[0] if chains else None))
            if r > 0:
                chains[r].set_temper(1.0 - 0.05 * r)
        with pytest.raises(bmm.BmmError) as e:
            bmm.Ladder(chains)
        assert e.value.code == E_ARG and "1 to 8" in str(e.value)
        with bmm.Ladder(chains[:8], seed=3) as lad:                     # the same chains make the full ladder afterwards
            lad.sweeps(2)
            assert lad.stats()["proposed"].tolist() == [1] * 7          # point 0: pairs 0, 2, 4, 6; point 1: pairs 1, 3, 5
            assert sorted(lad.stats()["walker"]) == list(range(8))
    finally:
        for c in chains[::-1]:
            c.close()
    nine = [1.0 - 0.05 * r for r in range(9)]
    for temper in (9, nine):
        with pytest.raises(bmm.BmmError) as e:
            bmm.gibbs_collapsed(X, 6, K=K, seed=1, initial_K=z0, temper=temper)
        assert e.value.code == E_ARG and "1 to 8" in str(e.value), temper
        with pytest.raises(bmm.BmmError) as e:
            bmm.gibbs_dp(X, 6, maxK=12, seed=1, temper=temper)
        assert e.value.code == E_ARG, temper
    plain = bmm.gibbs_collapsed(X, 6, K=K, seed=1, burnin=0, initial_K=z0)
    again = bmm.gibbs_collapsed(X, 6, K=K, seed=1, burnin=0, initial_K=z0)
    tgt._same(plain, again)
    assert "temper" not in again
    full = bmm.gibbs_collapsed(X, 6, K=K, seed=1, burnin=0, initial_K=z0, temper=8, temper_hottest=0.7)
    assert full["temper"]["proposed"].tolist() == [3, 2, 3, 2, 3, 2, 3]   # and the run takes eight: points 0 .. 4


# ---------------------------------------------------------------- B. a run replayed by a hand-built ladder
N, P, K = tr.REPLAY_SHAPE
SEED, BATCH = tr.REPLAY_SEED, tr.REPLAY_BATCH
SAMPLED = dict(alpha=None, a=2.0, b=1.5)
FIXED = dict(alpha=ALPHA)


def _data():
    X, _ = tr.mixture(N, P, tr.REPLAY_THETAS, tr.REPLAY_DATA_SEED)
    return X, np.random.default_rng(12).integers(1, K + 1, N).astype(np.int32)


def _run(bmm, sampler, X, z0, nsamples, burnin, prior, **kw):
    """the call under test; temper=, swap_every= and the options in kw"""
    if sampler == "collapsed":
        if kw.get("init", "random") == "random":
            kw["initial_K"] = z0
        return bmm.gibbs_collapsed(X, nsamples, K, beta=BETA, gamma=GAMMA, burnin=burnin, seed=SEED, batch=BATCH, **prior, **kw)
    return bmm.gibbs_dp(X, nsamples, beta=BETA, gamma=GAMMA, burnin=burnin, maxK=tr.REPLAY_MAXK, seed=SEED, batch=BATCH, **prior, **kw)


def _rungs(bmm, sampler, X, z0, powers, prior):
    """What temper_run_attach builds for such a call, from resident chains: rung r seeded SEED + r, the same prior
    arguments, the same explicit batch and (finite sampler) starting labels, rung 0 owning the data and the others
    sharing it, the ladder seeded as the run."""
    Kc = K if sampler == "collapsed" else tr.REPLAY_MAXK
    chains = []
    try:
        for r, b in enumerate(powers):
            c = bmm.Chain(sampler, N, P, Kc, beta=BETA, gamma=GAMMA, batch=BATCH, seed=SEED + r, **prior)
            chains.append(c)
            if r > 0:
                c.share_data(chains[0])
            else:
                c.set_data(X)
            if sampler == "collapsed":
                c.set_initial_labels(z0)
            if r > 0:
                c.set_temper(b)
        return chains, bmm.Ladder(chains, seed=SEED)
    except Exception:
        for c in chains[::-1]:
            c.close()
        raise


def _theta_hat(sampler, Nk, S):
    with np.errstate(invalid="ignore", divide="ignore"):
        th = S / Nk[:, None].astype(np.float64)       # NaN for an empty label of the finite sampler ...
    if sampler == "dp":
        th[Nk == 0] = 0.0                             # ... 0 for an unused one of the DP, as the run writes them
    return th


def _replay(bmm, sampler, X, z0, powers, prior, swap_every, burnin, nsamples, logpost=False, advance=None):
    """The run, one sweep at a time: every rung sweeps once, an exchange point behind every sweep whose index is a
    multiple of swap_every, and what rung 0 and the ladder hold after it written down for every kept sweep.
    `advance(c0, j)`: how rung 0 takes kept sweep j instead of sweeps(1) (the folds of section C); its results are
    returned as "folded", and "refolded" is what `advance.state(c0)` gives after the exchange point."""
    R, S = len(powers), nsamples - burnin
    Kc = K if sampler == "collapsed" else tr.REPLAY_MAXK
    rows = {"z": np.zeros((S, N), dtype=np.int32), "theta": np.full((Kc, P, S), np.nan), "alpha": np.full(S, np.nan),
            "loglik": np.full((S, R), np.nan), "walker_cold": np.zeros(S, dtype=np.int32), "logpost": np.full((S, 4), np.nan),
            "folded": [None] * S, "refolded": [None] * S}
    chains, ladder = _rungs(bmm, sampler, X, z0, powers, prior)
    try:
        c0 = chains[0]
        if advance is not None:
            advance.arm(c0)
        for j in range(1, nsamples):
            s = j - burnin
            for c in chains:
                if c is c0 and advance is not None and s >= 0:
                    rows["folded"][s] = advance(c0)
                else:
                    c.sweeps(1)
            point = j % swap_every == 0
            if point:
                ladder.exchange_step()
            if s < 0:
                continue
            rows["z"][s] = c0.labels()
            rows["theta"][:, :, s] = _theta_hat(sampler, *c0.counts())
            rows["alpha"][s] = c0.alpha()
            if point:
                rows["loglik"][s] = [c.logpost_state()["log_lik"] for c in chains]
            rows["walker_cold"][s] = ladder.stats()["walker"][0]
            if logpost:
                lp = c0.logpost_state()
                rows["logpost"][s] = [lp[k] for k in LP_KEYS]
            if advance is not None:
                rows["refolded"][s] = advance.state(c0)
        st = ladder.stats()
        rows["proposed"], rows["accepted"] = st["proposed"], st["accepted"]
        if advance is not None:
            rows["summary"] = advance.summary(c0)
        return rows
    finally:
        tgt._close(chains, ladder)


def _same_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(tgt._bits(got[~nan]), tgt._bits(want[~nan])), what


def _rows_equal(sampler, out, rows, burnin, z0, R, swap_every, logpost):
    """every kept row of the run `out` against the replay, bit for bit; the starting row of a run without burn-in is
    the starting state: no exchange, no log_lik, walker 0"""
    S = out["z"].shape[0]
    first = 1 if burnin == 0 else 0
    if first:
        if sampler == "collapsed":
            np.testing.assert_array_equal(out["z"][0], z0)
            assert np.all(np.isnan(out["theta"][:, :, 0]))
        else:
            assert np.all(out["z"][0] < 0) and np.all(out["theta"][:, :, 0] == 0.0)
        assert out["temper"]["walker_cold"][0] == 0
    np.testing.assert_array_equal(out["z"][first:], rows["z"][first:])
    _same_bits(out["theta"][:, :, first:], rows["theta"][:, :, first:], "theta")
    _same_bits(out["alpha"].ravel()[first:], rows["alpha"][first:], "alpha")
    tp = out["temper"]
    assert tp["loglik"].shape == (S, R)
    _same_bits(tp["loglik"], rows["loglik"], "loglik")
    points = np.array([(s + burnin) % swap_every == 0 and s + burnin >= 1 for s in range(S)])
    assert np.all(np.isfinite(tp["loglik"][points])) and np.all(np.isnan(tp["loglik"][~points]))   # every column, both ways
    np.testing.assert_array_equal(tp["walker_cold"], rows["walker_cold"])
    np.testing.assert_array_equal(tp["proposed"], rows["proposed"])
    np.testing.assert_array_equal(tp["accepted"], rows["accepted"])
    if logpost:
        lp = out["logpost"]
        for q, k in enumerate(LP_KEYS):
            _same_bits(lp[k], rows["logpost"][:, q], k)
        assert np.all(np.isfinite(rows["logpost"][first:]))
        assert lp["best"] == first + int(np.argmax(rows["logpost"][first:, 3]))   # the first maximum of log_joint
        np.testing.assert_array_equal(lp["z_map"], out["z"][lp["best"]])


def _run_and_replay(bmm, sampler, R, swap_every, burnin, prior, nsamples, logpost=False, init="random", walker_floor=0, env=None):
    X, z0 = _data()
    powers = tr.REPLAY_POWERS[R]
    extra = dict(init=init) if init != "random" else {}
    lpkw = dict(logpost=True) if logpost else {}
    for k, v in (env[1] if env else {}).items():
        env[0].setenv(k, v)
    try:
        plain = _run(bmm, sampler, X, z0, nsamples, burnin, prior, **extra)
        out = _run(bmm, sampler, X, z0, nsamples, burnin, prior, temper=list(powers), swap_every=swap_every, **extra, **lpkw)
    finally:
        for k in (env[1] if env else {}):
            env[0].delenv(k, raising=False)
    if init != "random":   # with burnin = 0 the run returns its starting allocation as z[0]
        assert burnin == 0 and sampler == "collapsed"
        np.testing.assert_array_equal(plain["z"][0], out["z"][0])
        z0 = np.ascontiguousarray(out["z"][0], dtype=np.int32)
    # first the pin without a ladder: one rung of this builder is the untempered run
    one = _replay(bmm, sampler, X, z0, (1.0,), prior, swap_every, burnin, nsamples)
    first = 1 if burnin == 0 else 0
    np.testing.assert_array_equal(plain["z"][first:], one["z"][first:])
    _same_bits(plain["theta"][:, :, first:], one["theta"][:, :, first:], "theta of the untempered run")
    _same_bits(plain["alpha"].ravel()[first:], one["alpha"][first:], "alpha of the untempered run")
    rows = _replay(bmm, sampler, X, z0, powers, prior, swap_every, burnin, nsamples, logpost=logpost)
    _rows_equal(sampler, out, rows, burnin, z0, R, swap_every, logpost)
    tp = out["temper"]
    moved = int(np.count_nonzero(np.diff(tp["walker_cold"])))
    print("%s R=%d swap_every=%d burnin=%d: proposed %s accepted %s, walker_cold changes %d times" %
          (sampler, R, swap_every, burnin, tp["proposed"], tp["accepted"], moved))
    assert moved >= walker_floor
    assert not np.array_equal(out["z"], plain["z"])    # (and the ladder is not the plain run)
    if prior is SAMPLED:
        assert len(np.unique(out["alpha"])) > 3
    return out


CASES = [("collapsed", 3, 1, 3, SAMPLED, True), ("collapsed", 3, 2, 0, FIXED, False), ("collapsed", 3, 3, 3, SAMPLED, True),
         ("collapsed", 3, 2, 3, SAMPLED, False), ("dp", 3, 1, 0, SAMPLED, True), ("dp", 3, 2, 3, SAMPLED, False),
         ("dp", 3, 3, 0, SAMPLED, True), ("collapsed", 8, 1, 3, SAMPLED, True), ("dp", 4, 1, 0, SAMPLED, False),
         ("collapsed", 4, 2, 0, SAMPLED, False)]


@pytest.mark.parametrize("sampler,R,swap_every,burnin,prior,logpost", CASES,
                         ids=["%s-R%d-every%d-burnin%d-%s%s" % (c[0], c[1], c[2], c[3], "sampled" if c[4] is SAMPLED else "fixed",
                                                               "-logpost" if c[5] else "") for c in CASES])
def test_every_kept_row_of_a_tempered_run_is_the_hand_built_ladders(bmm, sampler, R, swap_every, burnin, prior, logpost):
    """N = 301: rung 0's label row inside the run is a row of the trace, off a 16-byte boundary in three rows of four,
    while the helper's is aligned: the exchange takes the scalar loop of temper_swap for all of it."""
    base = (sampler, R, swap_every, burnin) == ("collapsed", 3, 1, 3)
    _run_and_replay(bmm, sampler, R, swap_every, burnin, prior, tr.REPLAY_SWEEPS if R == 3 else 24, logpost=logpost,
                    walker_floor=3 if base else 0)


def test_a_tempered_run_on_the_int32_layout_is_the_hand_built_ladders(bmm, dbg_lib):
    """The helpers of such a run borrow rung 0's device matrix; the hand-built ladder runs on bit planes (which form
    runs never changes a chain's values)."""
    dbg_lib.delenv("BMM_X_LAYOUT_INT32", raising=False)
    _run_and_replay(bmm, "collapsed", 3, 1, 3, SAMPLED, 24, logpost=True, env=(dbg_lib, {"BMM_X_LAYOUT_INT32": "1"}))
    _run_and_replay(bmm, "dp", 3, 1, 0, SAMPLED, 24, env=(dbg_lib, {"BMM_X_LAYOUT_INT32": "1"}))


def test_a_tempered_run_from_a_kmodes_start_is_the_hand_built_ladders(bmm):
    """The helpers copy the device's starting allocation from rung 0: every hand-built rung gets the run's own row 0."""
    out = _run_and_replay(bmm, "collapsed", 3, 1, 0, SAMPLED, 24, logpost=True, init="kmodes")
    assert "init" in out and not np.array_equal(out["z"][0], _data()[1])


def test_a_tempered_run_with_the_progress_hook_armed_returns_the_same_bytes(bmm, capfd):
    X, z0 = _data()
    powers = list(tr.REPLAY_POWERS[3])
    for sampler in ("collapsed", "dp"):
        want = _run(bmm, sampler, X, z0, 16, 3, SAMPLED, temper=powers, swap_every=2, logpost=True)
        capfd.readouterr()
        old = bmm.set_progress(2)
        try:
            got = _run(bmm, sampler, X, z0, 16, 3, SAMPLED, temper=powers, swap_every=2, logpost=True)
        finally:
            bmm.set_progress(old)
        lines = capfd.readouterr().out.splitlines()
        assert [l.split("\t")[0] for l in lines] == ["Sample %d" % j for j in (3, 5, 7, 9, 11, 13, 15, 16)]
        tgt._same(got, want)
        for k in ("proposed", "accepted", "walker_cold", "loglik"):
            assert np.array_equal(got["temper"][k], want["temper"][k], equal_nan=True), k
        for k in LP_KEYS + ("best", "z_map"):
            assert np.array_equal(got["logpost"][k], want["logpost"][k], equal_nan=True), k
        assert want["temper"]["accepted"].sum() > 0


# ---------------------------------------------------------------- C. what the folds of a tempered run see
class _Predict:
    """rung 0 takes its kept sweeps through sweeps_predict(1, trace=True)"""

    def __init__(self, Xnew):
        self.Xnew = Xnew

    def arm(self, c):
        c.set_newdata(self.Xnew)

    def __call__(self, c):
        return c.sweeps_predict(1, trace=True)[0]

    def state(self, c):
        return c.predict_state()

    def summary(self, c):
        return c.predictive()


class _Loo:
    """... through sweeps_loo(1, trace=True)"""

    def arm(self, c):
        c.set_loo()

    def __call__(self, c):
        return c.sweeps_loo(1, trace=True)[0]

    def state(self, c):
        return c.loo_state()

    def summary(self, c):
        return c.loo()


def test_predictive_and_loo_folds_of_a_tempered_run_see_rung_0_before_the_exchange(bmm):
    """the two folds stay inside the sweep."""
    X, z0 = _data()
    Xnew, _ = tr.mixture(40, P, tr.REPLAY_THETAS, 77)
    powers, nsamples, burnin = tr.REPLAY_POWERS[3], 24, 2
    S = nsamples - burnin
    kw = dict(temper=list(powers), swap_every=1)
    plain = _run(bmm, "collapsed", X, z0, nsamples, burnin, SAMPLED, **kw)
    pred = _run(bmm, "collapsed", X, z0, nsamples, burnin, SAMPLED, newdata=Xnew, predictive_trace=True, **kw)
    loo = _run(bmm, "collapsed", X, z0, nsamples, burnin, SAMPLED, loo="trace", **kw)
    both = _run(bmm, "collapsed", X, z0, nsamples, burnin, SAMPLED, newdata=Xnew, loo=True, partition="binder", **kw)
    for o in (pred, loo, both):                       # the folds change nothing the run returns otherwise
        tgt._same(o, plain)
        for k in ("inv_temp", "proposed", "accepted", "walker_cold", "loglik"):
            assert np.array_equal(o["temper"][k], plain["temper"][k], equal_nan=True), k
    _same_bits(both["predictive"]["lppd"], pred["predictive"]["lppd"], "lppd with all three armed")
    _same_bits(both["loo"]["log_cpo"], loo["loo"]["log_cpo"], "log_cpo with all three armed")
    # an unexchanged control: the folding sweeps advance a chain exactly as sweeps(1) does
    for adv in (_Predict(Xnew), _Loo()):
        folded = _replay(bmm, "collapsed", X, z0, (1.0,), SAMPLED, 1, burnin, 8, advance=adv)
        swept = _replay(bmm, "collapsed", X, z0, (1.0,), SAMPLED, 1, burnin, 8)
        for k in ("z", "theta", "alpha"):
            assert np.array_equal(folded[k], swept[k], equal_nan=True), k
    # the ladder, rung 0 folding its kept sweeps: the run's rows are the ones taken before the exchange point
    for adv, got, summary, keys in ((_Predict(Xnew), pred["predictive"]["logdens"], pred["predictive"], ("lppd",)),
                                    (_Loo(), loo["loo"]["ell"], loo["loo"], ("log_cpo", "ess", "lppd", "mean", "var"))):
        rows = _replay(bmm, "collapsed", X, z0, powers, SAMPLED, 1, burnin, nsamples, advance=adv)
        np.testing.assert_array_equal(rows["z"], plain["z"])           # (the replay is the run)
        assert got.shape == (S, len(rows["folded"][0]))
        told = 0
        for s in range(S):
            _same_bits(got[s], rows["folded"][s], "row %d" % s)
            told += not np.array_equal(rows["folded"][s], rows["refolded"][s])
        print("%s: %d of %d rows would differ had the fold seen the state after the exchange" % (type(adv).__name__, told, S))
        assert told >= 3                                                # (the check can tell)
        for k in keys:
            _same_bits(summary[k], rows["summary"][k], k)
