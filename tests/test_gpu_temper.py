"""Parallel tempering on the device (include/bmm_mcmc.h "parallel tempering") against the NumPy
restatement (tests/temper_ref.py) and against the exact posterior by enumeration."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_merge_ref as smr  # noqa: E402
import temper_ref as tr  # noqa: E402
import test_gpu_feature_select as tfs  # noqa: E402  (its shapes, forms and seven-by-four data set)

pytestmark = pytest.mark.gpu

BETA = GAMMA = 0.5
ALPHA = 1.3
E_ARG, E_UNSUPPORTED, E_STATE = 1, 2, 5


@pytest.fixture(scope="module")
def bmm():
    import importlib
    return importlib.import_module("bmm_mcmc_amd")  # (the module the dbg_lib fixture steers)


def _chain(bmm, sampler, X, K, batch, seed, layout=None, initial=None, alpha=ALPHA, share=None):
    N, P = X.shape
    c = bmm.Chain(sampler, N, P, K, alpha=alpha, beta=BETA, gamma=GAMMA, batch=batch, seed=seed, x_layout=layout)
    if share is not None:
        c.share_data(share)
    else:
        c.set_data(X)
    if sampler == "collapsed":
        if initial is None:
            initial = np.random.default_rng(seed).integers(1, K + 1, N).astype(np.int32)
        c.set_initial_labels(initial)
    return c


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _state(c):
    Nk, S = c.counts()
    return c.labels().tobytes(), Nk.tobytes(), S.tobytes(), np.float64(c.alpha()).tobytes()


def _recount(X, z1, K):
    return tr.fsr.counts(X, np.asarray(z1) - 1, K)


# ---------------------------------------------------------------- 1. the tempered tables
POWERS = [1.0, 0.5, 2.0 ** -4, 0.3]


@pytest.mark.parametrize("layout", ["bits", "int32"])
@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
@pytest.mark.parametrize("N,P,K", tfs.SHAPES)
def test_tempered_probabilities_equal_the_restatement(bmm, N, P, K, sampler, layout):
    """batch = N: the probabilities of a sweep are a pure function of the labels before it."""
    X, _ = tfs._mixture(N, P, [0.2, 0.5, 0.8], 3)
    rows = np.unique(np.concatenate([np.arange(0, min(N, 130)), np.arange(max(0, N - 70), N), np.arange(1000, N, 997)]))
    rng = np.random.default_rng(7)
    with _chain(bmm, sampler, X, K, N, 11, layout) as c:
        c.sweeps(2)
        weighed = 0
        for b in POWERS:
            c.set_temper(b)
            assert c.temper() == (True, b)
            if sampler == "dp":  # an allocation that leaves the last label unused: every draw weighs the new-cluster option
                c.set_labels(rng.integers(1, K, N).astype(np.int32))
            z = c.labels() - 1
            probs = c.sweep_probs()
            want = tr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, b, sampler, rows=rows)
            got = probs[rows]
            big = want > 1e-300
            rel = np.abs(got[big] - want[big]) / want[big]
            print("%s %s %s N=%d P=%d K=%d b=%g worst relative %.2e" % (sampler, layout, c.kernel_shape(), N, P, K, b, rel.max()))
            assert rel.max() <= 1e-12
            assert np.all(got[~big] <= 1e-300)
            if sampler == "dp":  # (filed under the last label unless taking the row out has freed a smaller one)
                weighed += int(np.any((want[:, K - 1] > 0.0) & (got[:, K - 1] > 0.0)))
            if b == 0.3:  # and the check can tell: the untempered conditional is another one
                cold = tr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, 1.0, sampler, rows=rows)
                assert np.abs(cold - want).max() > 1e-6
        assert sampler != "dp" or weighed == len(POWERS)
        assert not c.kernel_shape()["builds_own_tables"]


@pytest.mark.parametrize("layout", ["bits", "int32"])
@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
def test_tempered_probabilities_at_the_table_edges(bmm, sampler, layout):
    """The edges of k_count_tables<TAB_TEMPER> on purpose (tests/temper_ref.py edge_case): an empty label (n = 0: both constants
    -inf, no term), a singleton (n = 1: nothing left with its row removed), a pair, a column of zeros (s = 0) and a
    column of ones (s = n) in every label.  The finite chain holds the allocation as its starting labels (only a DP
    chain takes labels between sweeps), so its first table build also folds the counts from the delta replicas.
    What the edges can show: a singleton or an empty label given a constant (its row would get weight the reference
    denies it).  The `have` guards at s = 0 and s = n - 1 of the own-cluster terms protect entries no draw reads (a row
    of the label with x = 1 makes s >= 1): dropping them changes no probability, here or anywhere."""
    N, P, K = tr.EDGE_SHAPE
    X, z = tr.edge_case()
    rows = np.unique(np.concatenate([tr.EDGE_ROWS["single"], tr.EDGE_ROWS["pair"], np.arange(0, 60), np.arange(N - 30, N)]))
    at = {name: [int(np.flatnonzero(rows == i)[0]) for i in ids] for name, ids in tr.EDGE_ROWS.items()}
    z1 = (z + 1).astype(np.int32)
    for b in POWERS:
        with _chain(bmm, sampler, X, K, N, 11, layout, initial=z1) as c:
            if sampler == "dp":
                c.sweeps(2)
                c.set_labels(z1)
            c.set_temper(b)
            np.testing.assert_array_equal(c.labels(), z1)
            probs = c.sweep_probs()
        want = tr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, b, sampler, rows=rows)
        got = probs[rows]
        # the edge is there, by the reference's own account
        if sampler == "collapsed":
            assert np.all(want[:, tr.EDGE_EMPTY] == 0.0) and want[at["single"][0], tr.EDGE_SINGLE] == 0.0
        else:
            assert np.all(want[:, tr.EDGE_EMPTY] > 0.0) and want[at["single"][0], tr.EDGE_SINGLE] == 0.0
        assert np.all(want[at["pair"], tr.EDGE_PAIR] > 0.0)
        big = want > 1e-300
        rel = np.abs(got[big] - want[big]) / want[big]
        for name, idx in at.items():
            print("%s %s b=%g %s rows: worst relative %.2e" % (sampler, layout, b, name, (np.abs(got[idx] - want[idx])[big[idx]] / want[idx][big[idx]]).max()))
        print("%s %s b=%g all %d rows: worst relative %.2e" % (sampler, layout, b, len(rows), rel.max()))
        assert rel.max() <= 1e-12
        assert np.all(got[~big] <= 1e-300)
        if sampler == "dp":
            assert np.all(got[:, tr.EDGE_EMPTY] > 0.0)


# ---------------------------------------------------------------- 2. every form
@pytest.mark.parametrize("env,sampler,N,P,K,batch", tfs.FORMS)
def test_every_form_power_one_is_the_unarmed_chain_and_a_power_is_the_same_chain_on_every_form(bmm, dbg_lib, env, sampler, N, P, K, batch):
    for k in tfs.SWITCHES:
        dbg_lib.delenv(k, raising=False)
    X, _ = tfs._mixture(N, P, [0.2, 0.5, 0.8], 5)

    def run(b):
        with tfs._chain(bmm, sampler, X, K, batch, 23) as c:
            if sampler == "dp":
                c.sweeps(1)
            if b is not None:
                c.set_temper(b)
            c.sweeps(5)
            return _state(c), c.kernel_shape()
    plain_unarmed, _ = run(None)      # the plain form of the shape first (no switch): what every other form must reproduce
    plain_warm, _ = run(0.3)
    assert plain_warm != plain_unarmed
    for k, v in env.items():
        dbg_lib.setenv(k, v)
    unarmed, shape = run(None)
    assert unarmed == plain_unarmed   # (which form runs never changes a chain's values)
    one, shape_one = run(1.0)
    warm, shape_warm = run(0.3)
    print(env, sampler, "unarmed:", shape, "armed:", shape_warm)
    assert one == unarmed             # labels, counts and alpha, byte for byte
    assert warm == plain_warm
    assert warm != unarmed
    assert not shape_one["builds_own_tables"] and not shape_warm["builds_own_tables"]


# ---------------------------------------------------------------- 3. the exchange decision
def _ladder(bmm, X, K, powers, sampler="collapsed", batch=None, seeds=None, initials=None, alpha=ALPHA, ladder_seed=5):
    chains = []
    for r, b in enumerate(powers):
        c = _chain(bmm, sampler, X, K, batch, (seeds or range(100, 100 + len(powers)))[r], initial=None if initials is None else initials[r],
                   alpha=alpha, share=chains[0] if chains else None)
        if r > 0:
            c.set_temper(b)
        chains.append(c)
    return chains, bmm.Ladder(chains, seed=ladder_seed)


def _close(chains, ladder):
    ladder.close()
    for c in chains[::-1]:
        c.close()


@pytest.mark.parametrize("R", sorted(tr.EXCHANGE_POWERS))
def test_sixty_exchange_points_replayed_from_the_rungs_own_rows(bmm, R):
    N, P, K = tr.EXCHANGE_SHAPE
    powers, seed = tr.EXCHANGE_POWERS[R], 5
    X, _ = tr.mixture(N, P, tr.EXCHANGE_THETAS, tr.EXCHANGE_DATA_SEED)
    z0 = (np.random.default_rng(11).integers(0, K, N) + 1).astype(np.int32)
    chains, ladder = _ladder(bmm, X, K, powers, initials=[z0] * R, ladder_seed=seed)
    try:
        proposed, accepted = np.zeros(R - 1, dtype=np.int64), np.zeros(R - 1, dtype=np.int64)
        walker = np.arange(R)
        for t in range(tr.EXCHANGE_STEPS):
            for c in chains:
                c.sweeps(1)
            L = [c.logpost_state()["log_lik"] for c in chains]
            before = [_state(c) for c in chains]
            for st in before:                                                     # every sweep went on from a whole state
                _counts_belong_to_the_labels(X, K, st)
            rec, _ = _exchange_and_check(bmm, X, K, chains, ladder, before, go_on=False)
            pairs = tr.proposed_pairs(R, t)
            assert pairs == list(range(t % 2, R - 1, 2))                        # parity alternates
            for r in range(R - 1):
                assert rec[r]["point"] == t and rec[r]["proposed"] == (r in pairs)
                if r not in pairs:
                    assert not rec[r]["accepted"] and np.isnan(rec[r]["d"]) and np.isnan(rec[r]["u"])
                    continue
                d = tr.log_ratio(powers[r], powers[r + 1], L[r], L[r + 1])
                u = tr.exchange_uniform(seed, r, t)
                assert _bits(rec[r]["d"]) == _bits(d), (t, r, rec[r]["d"], d)     # bit for bit from the rungs' own rows
                assert _bits(rec[r]["u"]) == _bits(u), (t, r, rec[r]["u"], u)
                acc = tr.accepts(d, u)
                assert rec[r]["accepted"] == acc, (t, r, d, u)
                proposed[r] += 1
                if acc:
                    accepted[r] += 1
                    walker[[r, r + 1]] = walker[[r + 1, r]]
            Lnew = [c.logpost_state()["log_lik"] for c in chains]                 # the states moved with the decisions
            want = list(L)
            for r in pairs:
                if rec[r]["accepted"]:
                    want[r], want[r + 1] = want[r + 1], want[r]
            np.testing.assert_array_equal(_bits(Lnew), _bits(want))
        st = ladder.stats()
        print("R = %d: proposed %s accepted %s walker %s" % (R, proposed, accepted, st["walker"]))
        np.testing.assert_array_equal(st["proposed"], proposed)                   # the counters add up
        np.testing.assert_array_equal(st["accepted"], accepted)
        np.testing.assert_array_equal(st["walker"], walker)
        assert proposed.sum() == sum(len(tr.proposed_pairs(R, t)) for t in range(tr.EXCHANGE_STEPS))
        floor = tr.EXCHANGE_FLOOR[R]
        assert floor == (10 if R in (2, 5) else 3)
        assert np.all(accepted >= floor) and np.all(proposed - accepted >= floor)  # (it cannot pass empty)
        for c in chains:                                                          # and the chains go on from whole states
            c.sweeps(2)
        for c in chains:
            _counts_belong_to_the_labels(X, K, _state(c))
    finally:
        _close(chains, ladder)


# ---------------------------------------------------------------- 4. the exchange itself
NEARLY_ONE = 1.0 - 2.0 ** -30  # d = 2^-30 (L' - L): acceptance all but certain


def _counts_belong_to_the_labels(X, K, state):
    Nk, S = _recount(X, np.frombuffer(state[0], dtype=np.int32), K)
    np.testing.assert_array_equal(np.frombuffer(state[1], dtype=np.int32), Nk)
    np.testing.assert_array_equal(np.frombuffer(state[2], dtype=np.int32).reshape(K, -1), S)


def _exchange_and_check(bmm, X, K, chains, ladder, before, expect=None, go_on=True):
    """One exchange point of a ladder of R rungs, the whole state of every rung held to it.  `before`: every rung's
    state ahead of the point (labels, Nk, S, alpha bytes; Nk and S None: counts unknown, labels and alpha only).  The
    recorded accepted pairs, applied as transpositions, say which state every rung must hold afterwards, byte for
    byte; the walker ids must have moved the same way; the counts must be a recount of X under the labels; and with
    `go_on` two more sweeps of every rung leave them so.  `expect`: the decisions, pair by pair, where the caller
    knows them.  Returns (the records, every rung's state after the point)."""
    R = len(chains)
    w0 = ladder.stats()["walker"]
    rec = ladder.exchange_step()
    assert len(rec) == R - 1 and len(before) == R
    if expect is not None:
        assert [e["accepted"] for e in rec] == list(expect), rec
    order = list(range(R))                                 # order[r]: the rung whose state sits at rung r now
    for r, e in enumerate(rec):
        assert e["proposed"] == (r in tr.proposed_pairs(R, e["point"])) and (e["proposed"] or not e["accepted"]), e
        if e["accepted"]:
            order[r], order[r + 1] = order[r + 1], order[r]
    after = [_state(c) for c in chains]
    w1 = ladder.stats()["walker"]
    for r in range(R):
        src = before[order[r]]
        assert after[r][0] == src[0], (r, order)           # the labels
        assert after[r][3] == src[3], (r, order)           # alpha
        if src[1] is not None:
            assert after[r][1:3] == src[1:3], (r, order)   # Nk, S
        _counts_belong_to_the_labels(X, K, after[r])
    np.testing.assert_array_equal(w1, w0[order])
    if go_on:
        for c in chains:                                   # and the chains go on from whole states
            c.sweeps(2)
        for c in chains:
            _counts_belong_to_the_labels(X, K, _state(c))
    return rec, after


@pytest.mark.parametrize("N,P,K", [(300, 8, 4), (70_000, 130, 4)])
def test_an_accepted_exchange_before_the_first_sweep_swaps_the_pending_deltas(bmm, N, P, K):
    """A finite chain before its first sweep: the counts of the initial allocation wait in the delta replicas."""
    X, _ = tfs._mixture(N, P, [0.2, 0.5, 0.8], 3)
    zs = [np.random.default_rng(s).integers(1, K + 1, N).astype(np.int32) for s in (1, 2)]
    chains, ladder = _ladder(bmm, X, K, (1.0, NEARLY_ONE), initials=zs)
    try:
        a = np.float64(ALPHA).tobytes()
        before = [(z.tobytes(), None, None, a) for z in zs]
        rec, _ = _exchange_and_check(bmm, X, K, chains, ladder, before, [True])
        assert rec[0]["proposed"]
    finally:
        _close(chains, ladder)


def test_accepted_and_rejected_exchanges_between_sweeps(bmm):
    N, P, K = 300, 8, 4
    X, comp = tfs._mixture(N, P, [0.05, 0.5, 0.95], 3)
    good = (comp + 1).astype(np.int32)                                  # the generating allocation: a far better log_lik
    poor = np.random.default_rng(2).integers(1, K + 1, N).astype(np.int32)
    # rung 1 holds the poor state at a power of 2^-10: d = (1 - 2^-10) (L_poor - L_good), hundreds below zero
    chains, ladder = _ladder(bmm, X, K, (1.0, 2.0 ** -10), initials=[good, poor])
    try:
        L = [c.logpost_state()["log_lik"] for c in chains]
        assert L[1] - L[0] < -100.0
        before = [_state(c) for c in chains]
        rec, _ = _exchange_and_check(bmm, X, K, chains, ladder, before, [False])
        assert rec[0]["proposed"]
    finally:
        _close(chains, ladder)
    chains, ladder = _ladder(bmm, X, K, (1.0, NEARLY_ONE), initials=[good, poor])
    try:
        for c in chains:
            c.sweeps(3)
        before = [_state(c) for c in chains]
        assert before[0] != before[1]
        rec, after = _exchange_and_check(bmm, X, K, chains, ladder, before, [True])
        assert rec[0]["proposed"]
        assert ladder.stats()["accepted"][0] == 1 and after[0] != after[1]
    finally:
        _close(chains, ladder)


def test_an_accepted_exchange_of_dp_chains_swaps_the_sampled_alpha(bmm):
    N, P, K = 300, 8, 12
    X, _ = tfs._mixture(N, P, [0.2, 0.5, 0.8], 3)
    chains, ladder = _ladder(bmm, X, K, (1.0, NEARLY_ONE), sampler="dp", alpha=None)
    try:
        with pytest.raises(bmm.BmmError) as e:       # rows without a label have no log_lik to compare
            ladder.exchange_step()
        assert e.value.code == E_STATE
        for c in chains:
            c.sweeps(4)
        before = [_state(c) for c in chains]
        assert before[0][3] != before[1][3]          # two concentrations
        rec, _ = _exchange_and_check(bmm, X, K, chains, ladder, before, [True])
        assert rec[0]["proposed"]
    finally:
        _close(chains, ladder)


# ---------------------------------------------------------------- 5. one rung is today's run
def _same(a, b, keys=("z", "theta", "alpha")):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_a_ladder_of_one_rung_is_the_run_without_it_and_a_ladder_is_reproducible(bmm):
    X, _ = tfs._mixture(2000, 37, [0.2, 0.5, 0.8], 2)
    for fn, kw in ((bmm.gibbs_collapsed, dict(K=4)), (bmm.gibbs_dp, dict(maxK=12))):
        a = fn(X, 8, burnin=0, seed=5, **kw)
        b = fn(X, 8, burnin=0, seed=5, temper=[1.0], **kw)
        _same(a, b)
        assert b["temper"]["proposed"].size == 0 and np.all(b["temper"]["walker_cold"] == 0)
        c = fn(X, 12, burnin=2, seed=5, temper=[1, 0.6, 0.3], **kw)
        d = fn(X, 12, burnin=2, seed=5, temper=[1, 0.6, 0.3], **kw)
        _same(c, d)
        for k in ("inv_temp", "proposed", "accepted", "rate", "walker_cold", "loglik"):
            assert np.array_equal(c["temper"][k], d["temper"][k], equal_nan=True), k
        np.testing.assert_array_equal(c["temper"]["proposed"], [6, 5])   # sweeps 1 .. 11: pair 0 at the even points 0, 2, .., 10
        assert np.all(np.isfinite(c["temper"]["loglik"]))
        e = fn(X, 12, burnin=2, seed=5, temper=3, temper_hottest=0.3, **kw)  # an integer: the geometric ladder
        np.testing.assert_allclose(e["temper"]["inv_temp"], [1.0, 0.3 ** 0.5, 0.3], rtol=1e-15)


# ---------------------------------------------------------------- 6. the cold chain against the exact posterior
@pytest.fixture(scope="module")
def exact_clusters():
    X = tfs.seven_by_four()
    parts = smr.partitions(len(X))
    assert len(parts) == 877
    pi, _ = tr.tempered_posterior(X, parts, ALPHA, BETA, GAMMA, 1.0)
    nclus = np.array(parts).max(axis=1) + 1
    return X, np.array([pi[nclus == k].sum() for k in range(1, 8)])


@pytest.mark.parametrize("swap_every", [1, 3])
def test_the_cold_chain_of_a_ladder_samples_the_exact_posterior(bmm, exact_clusters, swap_every):
    X, want = exact_clusters
    n_batches = 100
    out = bmm.gibbs_dp(np.asfortranarray(X), 20_001, alpha=ALPHA, beta=BETA, gamma=GAMMA, burnin=1, maxK=30, batch=1, seed=9,
                       temper=[1, 0.4], swap_every=swap_every)
    tp = out["temper"]
    print("swap_every %d: proposed %s accepted %s" % (swap_every, tp["proposed"], tp["accepted"]))
    assert tp["proposed"][0] == len(range(0, 20_000 // swap_every, 2)) and 0 < tp["accepted"][0] < tp["proposed"][0]
    assert set(np.unique(tp["walker_cold"])) == {0, 1}
    _clusters_in_use_within_four_standard_errors(out, want, n_batches)


def test_the_cold_chain_of_a_ladder_of_three_samples_the_exact_posterior(bmm, exact_clusters):
    """Both parities act on the cold chain's neighbours: pair 0 at the even points, pair 1 at the odd ones (with two
    rungs the odd points propose nothing).  tests/test_temper_ref.py holds the composition -- scan, even point, odd
    point -- to the invariance of pi_1 x pi_0.6 x pi_0.3 by enumeration; here the device's cold chain is held to pi_1."""
    X, want = exact_clusters
    out = bmm.gibbs_dp(np.asfortranarray(X), 20_001, alpha=ALPHA, beta=BETA, gamma=GAMMA, burnin=1, maxK=30, batch=1, seed=9,
                       temper=[1, 0.6, 0.3], swap_every=1)
    tp = out["temper"]
    print("three rungs: proposed %s accepted %s" % (tp["proposed"], tp["accepted"]))
    np.testing.assert_array_equal(tp["proposed"], [10_000, 10_000])      # points 0 .. 19 999: the even ones, the odd ones
    assert np.all(tp["accepted"] > 0) and np.all(tp["accepted"] < tp["proposed"])
    assert set(np.unique(tp["walker_cold"])) == {0, 1, 2}
    _clusters_in_use_within_four_standard_errors(out, want, 100)


def _clusters_in_use_within_four_standard_errors(out, want, n_batches):
    k_used = np.array([len(set(row)) for row in out["z"]])
    n = len(k_used) // n_batches * n_batches
    worst = 0.0
    for k in range(1, 8):
        s, p = (k_used[:n] == k).astype(np.float64), float(want[k - 1])
        bm = s.reshape(n_batches, -1).mean(axis=1)
        se = max(bm.std(ddof=1) / np.sqrt(n_batches), np.sqrt(max(p * (1.0 - p), 0.0) / n))
        zscore = abs(s.mean() - p) / se
        worst = max(worst, zscore)
        print("clusters=%d: sampled %.5f exact %.5f se %.5f z %.2f" % (k, s.mean(), p, se, zscore))
        assert zscore <= 4.0, k
    print("worst z-score %.2f" % worst)


# ---------------------------------------------------------------- 7. the route and the refusals
def test_logpost_rows_of_a_tempered_run_belong_to_the_states_in_the_trace(bmm):
    X, _ = tfs._mixture(300, 8, [0.2, 0.5, 0.8], 3)
    z0 = np.random.default_rng(1).integers(1, 5, 300).astype(np.int32)
    out = bmm.gibbs_collapsed(X, 40, K=4, initial_K=z0, burnin=3, seed=7, a=2.0, b=1.5, logpost=True, temper=[1, 0.9, 0.8])
    assert out["temper"]["accepted"].sum() > 0 and len(np.unique(out["temper"]["walker_cold"])) > 1
    got = bmm.log_joint(X, out["z"], "collapsed", 4, out["alpha"].ravel(), BETA, GAMMA, 2.0, 1.5, sample_alpha=True)
    for k in ("log_lik", "log_prior", "log_hyper", "log_joint"):
        np.testing.assert_array_equal(_bits(got[k]), _bits(out["logpost"][k]), err_msg=k)
    np.testing.assert_array_equal(_bits(out["temper"]["loglik"][:, 0]), _bits(out["logpost"]["log_lik"]))
    # theta is the trace's own state too: S / Nk of the returned labels
    Nk, S = _recount(X, out["z"][-1], 4)
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_array_equal(out["theta"][:, :, -1], S / Nk[:, None].astype(np.float64))
    out = bmm.gibbs_dp(X, 30, alpha=1.5, burnin=2, seed=7, maxK=12, logpost=True, temper=[1, 0.9, 0.8], swap_every=2)
    got = bmm.log_joint(X, out["z"], "dp", 12, out["alpha"].ravel())
    np.testing.assert_array_equal(_bits(got["log_lik"]), _bits(out["logpost"]["log_lik"]))
    np.testing.assert_array_equal(_bits(got["log_joint"]), _bits(out["logpost"]["log_joint"]))


def _refused(bmm, code, fn, *a, **kw):
    with pytest.raises(bmm.BmmError) as e:
        fn(*a, **kw)
    assert e.value.code == code, str(e.value)


def test_every_refusal_leaves_the_chain_or_the_call_usable(bmm):
    N, P, K = 300, 8, 4
    X, _ = tfs._mixture(N, P, [0.2, 0.5, 0.8], 3)
    z0 = np.random.default_rng(1).integers(1, K + 1, N).astype(np.int32)
    pi0, th0 = np.full(K, 1.0 / K), np.full((K, P), 0.5)
    for sampler in ("stickbreaking", "full"):
        with bmm.Chain(sampler, N, P, K, alpha=ALPHA, seed=1) as c:
            c.set_data(X)
            c.set_initial_params(pi0, th0)
            _refused(bmm, E_UNSUPPORTED, c.set_temper, 0.5)
            c.sweeps(1)
    with _chain(bmm, "collapsed", X, K, None, 1, initial=z0) as c:       # a feature mask
        c.set_features(np.ones(P, dtype=np.uint8))
        _refused(bmm, E_UNSUPPORTED, c.set_temper, 0.5)
        c.sweeps(1)
    with _chain(bmm, "collapsed", X, K, None, 1, initial=z0) as c:       # the allocation sampler
        c.set_alloc()
        _refused(bmm, E_UNSUPPORTED, c.set_temper, 0.5)
        c.sweeps(1)
    with _chain(bmm, "dp", X, 12, None, 1) as c:                         # split-merge moves
        c.set_split_merge(1)
        _refused(bmm, E_UNSUPPORTED, c.set_temper, 0.5)
        c.sweeps(2)
    with _chain(bmm, "dp", X, 12, None, 1) as c:                         # ... and an armed chain refuses them in turn
        _refused(bmm, E_ARG, c.set_temper, 0.0)
        _refused(bmm, E_ARG, c.set_temper, 1.5)
        c.set_temper(0.5)
        _refused(bmm, E_UNSUPPORTED, c.set_split_merge, 1)
        _refused(bmm, E_UNSUPPORTED, c.set_features, np.ones(P, dtype=np.uint8))
        c.sweeps(2)
        c.set_temper(on=False)
        assert c.temper() == (False, 1.0)
        c.set_split_merge(1)
        c.sweeps(1)
    # the ladder's own checks name the rung
    a = _chain(bmm, "collapsed", X, K, None, 1, initial=z0)
    b = _chain(bmm, "collapsed", X, K, None, 2, initial=z0, share=a)
    c = _chain(bmm, "collapsed", X, K, None, 3, initial=z0, share=a)
    own = _chain(bmm, "collapsed", X, K, None, 4, initial=z0)           # its own copy of the data
    try:
        with pytest.raises(bmm.BmmError) as e:
            bmm.Ladder([a, b])                                           # rung 1 unarmed
        assert e.value.code == E_STATE and "rung 1" in str(e.value)
        b.set_temper(0.5)
        c.set_temper(0.5)
        with pytest.raises(bmm.BmmError) as e:
            bmm.Ladder([a, b, c])                                        # not strictly decreasing
        assert e.value.code == E_ARG and "rung 2" in str(e.value)
        own.set_temper(0.25)
        with pytest.raises(bmm.BmmError) as e:
            bmm.Ladder([a, b, own])
        assert e.value.code == E_STATE and "rung 2" in str(e.value)
        with pytest.raises(bmm.BmmError) as e:
            bmm.Ladder([b, c])                                           # rung 0 below 1
        assert e.value.code == E_ARG and "rung 0" in str(e.value)
        c.set_temper(0.25)
        b.sweeps(1)
        with pytest.raises(bmm.BmmError) as e:
            bmm.Ladder([a, b, c])                                        # another sweep index
        assert e.value.code == E_STATE and "rung 1" in str(e.value)
        a.sweeps(1)
        c.sweeps(1)
        with bmm.Ladder([a, b, c], seed=3) as lad:                       # and the same chains make a ladder afterwards
            lad.sweeps(4)
            assert lad.stats()["proposed"].tolist() == [2, 2]
        if bmm._capi.device_count() > 1:                                 # rungs on different devices
            far = bmm.Chain("collapsed", N, P, K, alpha=ALPHA, seed=5, device=1)
            try:
                far.set_data(X)
                far.set_initial_labels(z0)
                far.sweeps(5)
                far.set_temper(0.1)
                with pytest.raises(bmm.BmmError) as e:
                    bmm.Ladder([a, b, c, far])
                assert e.value.code == E_UNSUPPORTED and "rung 3" in str(e.value)
            finally:
                far.close()
    finally:
        for ch in (own, c, b, a):
            ch.close()
    # the run's refusals, each before anything is touched, and the next call runs
    _refused(bmm, E_UNSUPPORTED, bmm.gibbs_collapsed, X, 6, K=K, seed=1, temper=2, chains=2)
    _refused(bmm, E_UNSUPPORTED, bmm.gibbs_dp, X, 6, seed=1, maxK=12, temper=2, split_merge=1)
    _refused(bmm, E_UNSUPPORTED, bmm.gibbs_dp, X, 6, seed=1, maxK=12, temper=2, select_features=True)
    _refused(bmm, E_UNSUPPORTED, bmm.gibbs_collapsed, X, 60, K=K, seed=1, burnin=10, temper=2, relabel=True, stephens="device")
    _refused(bmm, E_ARG, bmm.gibbs_collapsed, X, 6, K=K, seed=1, temper=[1.0, 0.5, 0.5])
    _refused(bmm, E_ARG, bmm.gibbs_collapsed, X, 6, K=K, seed=1, temper=[0.9, 0.5])
    _refused(bmm, E_ARG, bmm.gibbs_collapsed, X, 6, K=K, seed=1, temper=2, swap_every=0)
    plain = bmm.gibbs_collapsed(X, 6, K=K, seed=1, burnin=0)
    again = bmm.gibbs_collapsed(X, 6, K=K, seed=1, burnin=0)
    _same(plain, again)
    assert "temper" not in again
