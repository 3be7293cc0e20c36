"""The device's variates over the whole shape plane, and the chains that draw from them at small hyperparameters.

1. bmm_device_variates_ex against the oracle bit for bit, NaN placement included, over the grids of
   variates_cases.py (whose laws test_variates_law.py holds the oracle to): gamma, beta, update_alpha_.
2. The forms the kernels actually run: update_alpha_wave (four gammas side by side in one wave) against update_alpha_,
   and the Beta draw split over two threads as k_sb_theta_tables draws theta against rbeta_.
3. gibbs_stickbreaking and gibbs_full against the oracle at beta, gamma down to 0.003, where gamma variates flush to
   0, theta cells are exactly 0 or 1 and their table entries -inf, on every form of the resample kernel; one run
   through the hand-off entry point.
4. The imputation step's phi and the eject move's p_E at 0.003 against the host builds of the spec."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi
from util import assert_matrix_equal

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_cases  # noqa: E402
import alloc_checks  # noqa: E402
import na_ref  # noqa: E402
import variates_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu

GAMMA, BETA, ALPHA, ALPHA_WAVE, SPLIT_BETA = 0, 1, 2, 3, 4
STREAMS = 20_000


def _dev(kind, p, q, seed, sweep, a=1.0, b=1.0, N=1000.0):
    p = np.ascontiguousarray(p, dtype=np.float64)
    q = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
    out = np.full(p.size, -7.0)
    _capi.check(_capi.lib().bmm_device_variates_ex(0, kind, _capi.vp(p), None if q is None else _capi.vp(q), C.c_double(a),
                                                   C.c_double(b), C.c_double(N), C.c_uint64(seed), C.c_uint32(sweep),
                                                   _capi.vp(out), C.c_int64(p.size)))
    return out


def _same_bits(got, want, what):
    bad = np.flatnonzero(vc.bits(got) != vc.bits(want))
    assert bad.size == 0, "%s: %d of %d differ, the first at %d: got %r, want %r" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------- 1. the plane, device against oracle
def test_gamma_grid_bit_exact(oracle):
    shape = np.repeat(vc.GAMMA_SHAPES, STREAMS)
    got = _dev(GAMMA, shape, None, 77, 5)
    _same_bits(got, oracle.rgamma_array(shape, 77, 5), "gamma")
    assert (got[:STREAMS] == 0.0).any()  # shape 1e-3: the flushed draws are in the comparison


def test_beta_grid_bit_exact(oracle):
    p = np.repeat([pq[0] for pq in vc.BETA_PAIRS], STREAMS)
    q = np.repeat([pq[1] for pq in vc.BETA_PAIRS], STREAMS)
    got = _dev(BETA, p, q, 9, 2)
    _same_bits(got, oracle.rbeta_array(p, q, 9, 2), "beta")
    assert not np.isnan(got).any() and ((got >= 0.0) & (got <= 1.0)).all()
    first = got[:STREAMS]  # Beta(1e-3, 1e-3): values decided from the logarithms, not only 0 and 1
    assert ((first > 0.0) & (first < 1e-300)).any()


def test_shapes_swept_over_twelve_decades_bit_exact(oracle):
    """one launch, a shape per element: neighbouring lanes take different branches (boost or none) and different
    numbers of rejection rounds"""
    p = np.logspace(-4, 8, 4096)
    q = p[::-1].copy()
    _same_bits(_dev(GAMMA, p, None, 3, 1), oracle.rgamma_array(p, 3, 1), "gamma sweep")
    got = _dev(BETA, p, q, 3, 1)
    _same_bits(got, oracle.rbeta_array(p, q, 3, 1), "beta sweep")
    assert not np.isnan(got).any()
    _same_bits(_dev(SPLIT_BETA, p, q, 3, 1), got, "split beta sweep")


@pytest.mark.parametrize("a", vc.ALPHA_A)
def test_update_alpha_grid_bit_exact(oracle, a):
    triples, old, K = vc.alpha_grid()
    old, K = np.repeat(old, STREAMS), np.repeat(K, STREAMS)
    for t, (a_, b, N) in enumerate(triples):
        if a_ != a:
            continue
        got = _dev(ALPHA, old, K, 1000 + t, 8, a, b, N)
        _same_bits(got, oracle.update_alpha_array(old, K, a, b, N, 1000 + t, 8), "update_alpha a=%g b=%g N=%g" % (a, b, N))
        assert np.isfinite(got).all() and (got > 0.0).all()


# ---------------------------------------------------------------- 2. the forms the kernels run
def test_update_alpha_wave_equals_update_alpha(oracle):
    triples, old, K = vc.alpha_grid()
    old, K = np.repeat(old, 2000), np.repeat(K, 2000)  # a wave per element
    for t, (a, b, N) in enumerate(triples):
        wave = _dev(ALPHA_WAVE, old, K, 50 + t, 3, a, b, N)
        _same_bits(wave, _dev(ALPHA, old, K, 50 + t, 3, a, b, N), "update_alpha_wave a=%g b=%g N=%g" % (a, b, N))
        if t % 9 == 0:
            _same_bits(wave, oracle.update_alpha_array(old, K, a, b, N, 50 + t, 3), "update_alpha_wave against the oracle")


def test_split_thread_beta_equals_rbeta(oracle):
    p = np.repeat([pq[0] for pq in vc.BETA_PAIRS], STREAMS)[:-77]  # a last workgroup that is not full
    q = np.repeat([pq[1] for pq in vc.BETA_PAIRS], STREAMS)[:-77]
    got = _dev(SPLIT_BETA, p, q, 9, 2)
    _same_bits(got, _dev(BETA, p, q, 9, 2), "split-thread beta against rbeta_")
    _same_bits(got, oracle.rbeta_array(p, q, 9, 2), "split-thread beta against the oracle")


# ---------------------------------------------------------------- 3. chains at small hyperparameters
@pytest.fixture(scope="module")
def chain_x():
    return vc.chain_data()


def _form(sampler, maxK):
    with bm.Chain(sampler, vc.CHAIN_N, vc.CHAIN_P, maxK, seed=1) as ch:
        return ch.kernel_shape()


@pytest.mark.parametrize("form", list(vc.CHAIN_FORMS))
def test_the_cases_run_the_kernel_forms_they_name(form):
    for sampler in ("stickbreaking", "full"):
        ks = _form(sampler, vc.CHAIN_FORMS[form])
        print(sampler, form, ks)
        if form == "generic":
            assert ks["lds_bytes"] == 0
        else:
            assert ks["lds_bytes"] > 0
        if form == "one-lane":
            assert ks["lanes_per_observation"] == 1
        if form == "two-lanes":
            assert ks["lanes_per_observation"] == 2


@pytest.mark.parametrize("form", list(vc.CHAIN_FORMS))
@pytest.mark.parametrize("beta,gamma", vc.CHAIN_HYPER)
def test_explicit_chains_at_small_hyperparameters(oracle, chain_x, beta, gamma, form):
    maxK = vc.CHAIN_FORMS[form]
    pi0, th0 = vc.chain_start(maxK)
    for sampler, fn in (("stickbreaking", bm.gibbs_stickbreaking), ("full", bm.gibbs_full)):
        got = fn(chain_x, vc.CHAIN_SWEEPS, maxK, beta=beta, gamma=gamma, burnin=0, seed=17, initial_pi=pi0, initial_theta=th0)
        want = vc.oracle_chain(oracle, sampler, chain_x, maxK, beta, gamma)
        n0, n1 = int((got["theta"] == 0.0).sum()), int((got["theta"] == 1.0).sum())
        print("%s %s beta = gamma = (%g, %g): theta cells exactly 0: %d, exactly 1: %d" % (sampler, form, beta, gamma, n0, n1))
        assert not np.isnan(got["theta"]).any() and not np.isnan(got["pi"]).any()
        assert ((got["theta"] >= 0.0) & (got["theta"] <= 1.0)).all()
        for key in ("z", "theta", "pi", "alpha"):
            assert got[key].shape == want[key].shape, key
            assert np.array_equal(got[key], want[key]), (sampler, key)
        if (beta, gamma) == (0.01, 0.01):  # the case is here for the -inf table entries: it must keep reaching them
            assert n0 > 0 and n1 > 0


class _Recorder:
    """stand-in for the host's Stephens code: keeps the matrices it is handed, relabels nothing"""

    def __init__(self, K):
        self.K, self.cube, self.samples = K, None, {}

    def batch(self, p):
        self.cube = np.array(p)
        return self.cube.mean(axis=2)

    def online(self, Q, p, j):
        self.samples[j] = np.array(p)
        return np.arange(self.K), (j * Q + p) / (j + 1)


@pytest.mark.parametrize("sampler", ["stickbreaking", "full"])
def test_hand_off_matrices_at_small_hyperparameters(oracle, chain_x, sampler):
    """the emitting twins on tables with -inf entries: every matrix against the oracle's, whole"""
    maxK, beta, burnin, W = vc.CHAIN_FORMS["resident"], 0.01, 50, 2
    pi0, th0 = vc.chain_start(maxK)
    st = _Recorder(maxK)
    fn = bm.gibbs_stickbreaking if sampler == "stickbreaking" else bm.gibbs_full
    got = fn(chain_x, vc.CHAIN_SWEEPS, maxK, beta=beta, gamma=beta, burnin=burnin, relabel=True, burnrelabel=W, seed=17,
             initial_pi=pi0, initial_theta=th0, stephens=st)
    sweeps = list(range(burnin - W, vc.CHAIN_SWEEPS))
    pi0, th0 = vc.chain_start(maxK)
    ofn = oracle.stickbreaking if sampler == "stickbreaking" else oracle.full
    want = ofn(chain_x, pi0, th0, vc.CHAIN_SWEEPS, maxK, 0.0, beta, beta, 1, 1, burnin, seed=17, probs_sweep=sweeps)
    assert np.array_equal(got["z_original"], want["z"]) and np.array_equal(got["pi"], want["pi"])
    assert st.cube.shape == (vc.CHAIN_N, maxK, W) and sorted(st.samples) == list(range(burnin, vc.CHAIN_SWEEPS))
    zeros = 0
    for q, j in enumerate(sweeps):
        m = st.cube[:, :, q] if j < burnin else st.samples[j]
        assert not np.isnan(m).any()
        zeros += int((m == 0.0).sum())
        assert_matrix_equal(m, want["probs"][:, :, q], "%s sweep %d" % (sampler, j))
    assert zeros > 0  # categories a theta cell of exactly 0 or 1 rules out


# ---------------------------------------------------------------- 4. the imputation step and the eject move
def test_imputation_step_at_small_hyperparameters():
    """gibbs_collapsed's auxiliary phi ~ Beta(beta + s, gamma + n - s) at beta = gamma = 0.003.  Feature 1 is missing in
    every row, so no label has an observed cell of it and its phi is a draw from the prior, Beta(0.003, 0.003): before
    the fallback a quarter of those were NaN.  40 sweeps, the counts a recount after every one, then one step against
    the host build of na_phi."""
    N, P, K, beta, seed = 200, 8, 4, 0.003, 21
    rng = np.random.default_rng(3)
    comp = rng.integers(3, size=N)
    X = (rng.random((N, P)) < np.asarray([0.15, 0.5, 0.85])[comp][:, None]).astype(np.int32)
    mis = rng.random((N, P)) < 0.2
    mis[:, 1] = True
    rows, cols = np.nonzero(mis)
    with bm.Chain("collapsed", N, P, K, alpha=1.3, beta=beta, gamma=beta, batch=50, seed=seed) as c:
        c.set_data(np.asfortranarray(np.where(mis, 0, X).astype(np.int32)))
        c.set_initial_labels(rng.integers(1, K + 1, N).astype(np.int32))
        c.set_missing(mask=mis)
        for t in range(40):
            c.sweeps(1)
            Xc = np.where(mis, 0, X).astype(np.int32)
            Xc[np.nonzero(mis)] = c.missing_state()
            Nk, S = c.counts()
            rNk, rS = na_ref.recount(Xc, c.labels() - 1, K)
            np.testing.assert_array_equal(Nk, rNk)
            np.testing.assert_array_equal(S, rS)
        z = c.labels() - 1
        c.missing_reset()
        c.impute_step()
        h = na_ref.host_step(Xc, z, Nk, S, rows, cols, seed, 40, beta, beta)
        phis = []
        for k in np.flatnonzero(Nk > 0):
            m, o, s, n, a, b, ph = h["cnt"][int(k) * P + 1]
            assert (s, n, a, b) == (0, 0, beta, beta)  # the (label, feature) pair with no observed cell
            phis.append(ph)
        allphi = np.array([v[6] for v in h["cnt"].values()])
        assert np.isfinite(allphi).all() and ((allphi >= 0.0) & (allphi <= 1.0)).all()
        assert len(phis) > 0
        np.testing.assert_array_equal(c.missing_state(), h["bits"][0])
        summ = c.missing_summary()
        assert summ["n_folded"] == 1
        assert np.isfinite(summ["mean"]).all() and ((summ["mean"] >= 0.0) & (summ["mean"] <= 1.0)).all()
        np.testing.assert_array_equal(summ["mean"].view(np.uint64), h["sum"].view(np.uint64))  # phi of every cell, by bits
        np.testing.assert_array_equal(c.counts()[1], h["S"])


def test_eject_moves_at_a_small_eject_parameter(tmp_path):
    """p_E ~ Beta(e, e) at e = 0.003 over 200 moves: a number in [0, 1] whenever a move ejects, the host build's bits"""
    exe = alloc_checks.build_host(tmp_path)
    case = alloc_cases.BY_NAME["empties"]._replace(e=0.003)
    X, z1, lp = alloc_cases.start(case)
    ejects, inside = 0, 0
    with bm.Chain("collapsed", case.N, case.P, case.maxK, alpha=case.a, beta=alloc_cases.BETA, gamma=alloc_cases.GAMMA,
                   seed=case.seed) as c:
        c.set_data(X)
        c.set_initial_labels(z1)
        c.set_alloc(np.exp(lp), 0, case.e)
        c.set_k(case.K0)
        for step in range(200):
            K_before = c.k()
            d = c.alloc_step(sides=True)
            h = alloc_checks.host_draws(exe, tmp_path, case.seed, 1, step, K_before, case.maxK, case.e)
            assert d["pe_bits"] == h["pe_bits"]
            pe = float(np.array([d["pe_bits"]], dtype=np.uint64).view(np.float64)[0])
            if d["kind"] == "eject":
                ejects += 1
                assert not np.isnan(pe) and 0.0 <= pe <= 1.0, (step, pe)
                inside += 0.0 < pe < 1.0
    print("%d ejects of 200 moves, %d with p_E strictly inside (0, 1)" % (ejects, inside))
    assert ejects >= 50
