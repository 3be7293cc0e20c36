"""The oracle's whole-matrix output (probs_sweep= of oracle.collapsed / dp / stickbreaking / full): the N x K matrix of
allocation probabilities of one sweep, filed by label as the reference stores it for Stephens' relabelling.  The GPU
tests hold every hand-off matrix of the device to it bit for bit; the tests here pin the matrix itself:

  - bit for bit, every row, to the per-row conditionals (collapsed_cond / dp_cond / sb_cond, spec=True), each under the
    state its batch saw -- earlier batches of the sweep redrawn, the rest as the previous sweep left them;
  - within 1e-11 of the softmax of loo_ref's leave-one-out category terms, taken in np.longdouble: a restatement
    that shares nothing with the oracle's table arithmetic;
  - for the DP, on a chain that reaches every branch of the rule for where the new-cluster mass is filed.

The DP's filing rule is applied here as tests/test_gpu_boundary.py applies it: the new cluster's probability goes under
the label a new cluster would take for that observation (collapsed_gibbs_dp.cpp:169-170, 193) -- the smallest label
without a member at batch start, or the observation's own label when it sat alone there and that label is smaller."""
import functools

import numpy as np
import pytest

import loo_ref
import predictive_ref as pref
from util import load_dataset, synth

ATOL = 1e-11          # the bound tests/test_gpu_predict.py holds responsibilities to
N, P = 300, 12
BATCHES = (N, 70)     # one batch; 70 does not divide 300 (four batches and a short one)


def batches_of(n, batch, dp_first_sweep=False):
    """[lo, hi) of every batch of a sweep; the DP seats its first sweep in batches of 1, 1, 2, 4, ... up to batch"""
    out, lo = [], 0
    while lo < n:
        length = min(batch, max(1, lo)) if dp_first_sweep else batch
        out.append((lo, min(n, lo + length)))
        lo = out[-1][1]
    return out


def states(z_before, z_after, n, batch, dp_first_sweep=False):
    """(lo, hi, state) per batch: the labels the batch saw"""
    return [(lo, hi, np.concatenate([z_after[:lo], z_before[lo:]])) for lo, hi in batches_of(n, batch, dp_first_sweep)]


def dp_file(norm, state, i, maxK):
    """the maxK + 1 normalised weights of row i as the row of the stored matrix; also the label the new-cluster mass
    went under (-1: nowhere) and whether the row sat alone"""
    size = np.bincount(state[state > 0] - 1, minlength=maxK)
    free = np.flatnonzero(size == 0)
    free = int(free[0]) if free.size else -1
    own = state[i] - 1
    alone = own >= 0 and size[own] == 1
    lbl = own if alone and (free < 0 or own < free) else free
    row = norm[:maxK].copy()
    if lbl >= 0:
        row[lbl] = norm[maxK]          # a label without members has weight exactly 0
    return row, lbl, alone, free


def softmax_ld(terms):
    t = np.asarray(terms, dtype=np.longdouble)
    w = np.exp(t - t.max(axis=1, keepdims=True))
    return w / w.sum(axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _data():
    X, _, _, _ = synth(N, P, 3, 21)
    rng = np.random.default_rng(4)
    return X, rng.integers(1, 5, N).astype(np.int32), rng.dirichlet(np.ones(5)), 0.05 + 0.9 * rng.random((5, P))


@functools.lru_cache(maxsize=None)
def _chain(sampler, batch):
    """four sweeps of the oracle chain with every sweep's matrix (sweep 0 of the trace is the initial state)"""
    from oracle import oracle
    oracle.build()
    X, z0, pi0, th0 = _data()
    sw = [1, 2, 3, 4]
    if sampler == "collapsed":
        return oracle.collapsed(X, z0, 5, 4, 1.3, 0.5, 0.5, 1, 1, 0, seed=6, batch=batch, probs_sweep=sw)
    if sampler == "dp":
        return oracle.dp(X, 5, 2.0, 0.5, 0.5, 1, 1, 0, 10, seed=6, batch=batch, probs_sweep=sw)
    fn = oracle.stickbreaking if sampler == "stickbreaking" else oracle.full
    return fn(X, pi0, th0, 5, 5, 1.5, 0.5, 0.5, 1, 1, 0, seed=6, probs_sweep=sw)


def test_existing_outputs_do_not_change_and_one_sweep_is_a_slice(oracle):
    X, z0, pi0, th0 = _data()
    plain = oracle.dp(X, 5, 2.0, 0.5, 0.5, 1, 1, 0, 10, seed=6, batch=70)
    assert "probs" not in plain
    both = _chain("dp", 70)
    for k in ("z", "theta", "alpha"):
        assert np.array_equal(plain[k], both[k], equal_nan=True)
    assert both["probs"].shape == (N, 10, 4)
    one = oracle.dp(X, 5, 2.0, 0.5, 0.5, 1, 1, 0, 10, seed=6, batch=70, probs_sweep=3)
    assert one["probs"].shape == (N, 10) and np.array_equal(one["probs"], both["probs"][:, :, 2])
    plain = oracle.full(X, pi0, th0, 5, 5, 1.5, 0.5, 0.5, 1, 1, 0, seed=6)
    both = _chain("full", N)
    for k in ("z", "theta", "alpha", "pi"):
        assert np.array_equal(plain[k], both[k])
    with pytest.raises(ValueError):
        oracle.collapsed(X, z0, 5, 4, 1.3, 0.5, 0.5, 1, 1, 0, seed=6, probs_sweep=5)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("sampler", ["collapsed", "dp"])
def test_counting_matrix_is_the_per_row_conditional_bit_for_bit(oracle, sampler, batch):
    X = _data()[0]
    got = _chain(sampler, batch)
    z = got["z"].copy()
    z[z < 0] = 0                                # the DP's rows before their first seat: no label
    for j in (1, 2, 3, 4):
        first = sampler == "dp" and j == 1      # the doubling schedule: 1, 1, 2, 4, ... (capped at the batch)
        m = got["probs"][:, :, j - 1]
        for lo, hi, state in states(z[j - 1], z[j], N, batch, first):
            for i in range(lo, hi):
                if sampler == "collapsed":
                    want = oracle.collapsed_cond(X, state, i, 4, 1.3, 0.5, 0.5, spec=True)[1]
                else:
                    want = dp_file(oracle.dp_cond(X, state, i, 10, 2.0, 0.5, 0.5, spec=True)[1], state, i, 10)[0]
                assert np.array_equal(m[i], want), (j, i)


@pytest.mark.parametrize("sampler", ["stickbreaking", "full"])
def test_explicit_matrix_is_the_per_row_conditional_bit_for_bit(oracle, sampler):
    X, _, pi0, th0 = _data()
    got = _chain(sampler, N)
    for j in (1, 2, 3, 4):                      # sweep j draws from the parameters sweep j - 1 left (slice 0: the initial ones)
        pi, th = got["pi"][j - 1], got["theta"][:, :, j - 1]
        for i in range(N):
            assert np.array_equal(got["probs"][i, :, j - 1], oracle.sb_cond(X, i, pi, th, spec=True)[1]), (j, i)


def _loo_softmax(sampler, X, state, K, alpha):
    Nk, S = pref.counts_from_labels(X, state, K)
    return softmax_ld(loo_ref.counting_terms(X, state, Nk, S, alpha, 0.5, 0.5, sampler))


@pytest.mark.parametrize("sampler,batch", [(s, b) for s in ("collapsed", "dp") for b in BATCHES]
                         + [("stickbreaking", N), ("full", N)])    # (the explicit samplers have no batches)
def test_matrix_against_the_leave_one_out_softmax_in_long_double(sampler, batch):
    """The Gibbs conditional of a fitted row is the softmax of its leave-one-out category terms.  Largest difference
    measured over these shapes (N = 300, P = 12, sweeps 2-4): 3.9e-15, 0.04 % of the bound."""
    explicit = sampler in ("stickbreaking", "full")
    X = _data()[0]
    got = _chain(sampler, batch)
    worst = 0.0
    for j in (2, 3, 4):                         # every row holds a label from sweep 1 on (loo_ref needs one)
        m = got["probs"][:, :, j - 1]
        if explicit:
            want = softmax_ld(pref.explicit_terms(X, got["pi"][j - 1], got["theta"][:, :, j - 1]))
        else:
            K, alpha = (4, 1.3) if sampler == "collapsed" else (10, 2.0)
            want = np.zeros((N, K), dtype=np.longdouble)
            for lo, hi, state in states(got["z"][j - 1], got["z"][j], N, batch):
                sm = _loo_softmax(sampler, X, state, K, alpha)
                for i in range(lo, hi):
                    want[i] = sm[i, :K] if sampler == "collapsed" else dp_file(sm[i], state, i, K)[0]
        worst = max(worst, float(np.abs(m - want).max()))
        np.testing.assert_allclose(m.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    print("largest difference %.3g = %.3g of the bound" % (worst, worst / ATOL))
    assert worst <= ATOL, worst


def test_dp_chain_that_reaches_every_filing_branch(oracle):
    """maxK = 10 and alpha = 1.5 on the 100 rows of the bundled K = 2 data: the chain moves between six and nine labels
    in use, so that rows sit alone below and above the smallest free label, and at maxK - 1 labels rows draw the new
    cluster while it cannot be opened.  Every row of every sweep against dp_cond and the rule."""
    X = load_dataset("K2_N100_P5")
    n, maxK, alpha, batch, seed, ns = 100, 10, 1.5, 7, 1, 31
    sweeps = list(range(1, ns))
    got = oracle.dp(X, ns, alpha, 0.5, 0.5, 1, 1, 0, maxK, seed=seed, batch=batch, probs_sweep=sweeps)
    z = got["z"].copy()
    z[z < 0] = 0
    below = above = full_state = truncated = 0
    for j in sweeps:
        for lo, hi, state in states(z[j - 1], z[j], n, batch, j == 1):
            size = np.bincount(state[state > 0] - 1, minlength=maxK)
            for i in range(lo, hi):
                norm = oracle.dp_cond(X, state, i, maxK, alpha, 0.5, 0.5, spec=True)[1]
                want, lbl, alone, free = dp_file(norm, state, i, maxK)
                assert np.array_equal(got["probs"][i, :, j - 1], want), (j, i)
                assert lbl >= 0 and want[lbl] == norm[maxK] > 0
                below += alone and lbl == state[i] - 1 and free >= 0      # alone under a label below the free one
                above += alone and lbl == free and free < state[i] - 1    # alone under a label above it
                if (size > 0).sum() == maxK - 1 and not alone:
                    # no room for another cluster (collapsed_gibbs_dp.cpp:213): the mass is still filed under the one
                    # free label, the draw of a row that lands in it goes to the smallest cluster
                    full_state += 1
                    assert lbl == free and (size == 0).sum() == 1
                    if oracle.z_uniform(seed, i, j) > 1.0 - norm[maxK] + 1e-9:     # the new cluster is the last category
                        rest = size - (np.arange(maxK) == state[i] - 1)
                        smallest = min((k for k in range(maxK) if rest[k] > 0), key=lambda k: (rest[k], k))
                        assert z[j, i] - 1 == smallest != free, (j, i)
                        truncated += 1
    print("alone below / above the free label: %d / %d; rows at maxK - 1 labels: %d, drawing the new cluster: %d"
          % (below, above, full_state, truncated))
    assert below >= 1, "no row alone under a label below the smallest free one: the test lost its case"
    assert above >= 1, "no row alone under a label above the smallest free one: the test lost its case"
    assert full_state >= 1, "no state with maxK - 1 labels in use: the test lost its case"
    assert truncated >= 1, "no draw of the new cluster at maxK - 1 labels in use: the test lost its case"
