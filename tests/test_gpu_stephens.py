"""Stephens' relabelling on the device (relabel=True, stephens="device") against the NumPy restatement of
src/stephens.cpp as it executes (tests/stephens_ref.py): the device entry points on random and crafted inputs,
then whole runs of all four samplers against the hook path driven by the restatement."""
import numpy as np
import pytest

import bmm_mcmc_amd as bm
import stephens_ref as sr
from util import load_dataset, synth

pytestmark = pytest.mark.gpu


def _probs(rng, N, K, zero_cols=()):
    p = rng.dirichlet(np.full(K, 0.3), size=N)
    for l in zero_cols:
        p[:, l] = 0.0
    s = p.sum(axis=1, keepdims=True)
    return np.asfortranarray(np.where(s > 0, p / np.where(s > 0, s, 1), 0.0))


@pytest.mark.parametrize("K,N,zero_cols", [(1, 777, ()), (2, 1001, ()), (3, 4099, (1,)), (20, 5003, (4, 17)),
                                           (30, 2049, ()), (50, 1531, (0, 49)), (128, 613, (5,))])
def test_online_entry_matches_the_restatement(K, N, zero_cols):
    rng = np.random.default_rng(K * 1000 + N)
    p = _probs(rng, N, K, zero_cols)
    Q = np.asfortranarray(rng.random((N, K)) * 3 + 0.01)
    j = 17
    perm, Qn, C = bm.stephens_online(Q, p, j, with_cost=True)
    lq = np.log(Q)
    want_C = sr.cost(p, lq, False)
    scale = sr.cost_scale(p, lq, False)
    assert np.all(np.abs(C - want_C) <= 1e-12 * scale + 1e-300)
    for l in zero_cols:
        assert (C[:, l] == 0).all()
    # the assignment: exactly the restatement's Hungarian method on the device's own costs
    assert np.array_equal(perm, sr.hungarian(C))
    # the update, bit for bit
    assert np.array_equal(Qn, (float(j) * (Q + p[:, perm])) / float(j + 1))
    # reproducible
    perm2, Qn2, C2 = bm.stephens_online(Q, p, j, with_cost=True)
    assert np.array_equal(perm, perm2) and np.array_equal(Qn, Qn2) and np.array_equal(C, C2)


def test_online_entry_on_crafted_ties_and_a_cycle():
    # all-zero p: every cost is exactly 0, the tie rule gives the identity
    N, K = 300, 6
    perm, Qn, C = bm.stephens_online(np.ones((N, K)), np.zeros((N, K)), 3, with_cost=True)
    assert (C == 0).all() and list(perm) == list(range(K))
    # the K = 3 cycle of test_stephens_ref: perm [2, 0, 1], p reordered by it uninverted
    Q = np.ones((3, 3))
    Q[:, 0] = np.exp([0.0, 3.0, 0.0])
    Q[:, 1] = np.exp([0.0, 0.0, 3.0])
    Q[:, 2] = np.exp([3.0, 0.0, 0.0])
    p = np.eye(3)
    perm, Qn = bm.stephens_online(Q, p, 5)
    want_perm, want_Q, _ = sr.online(Q, p, 5)
    assert list(perm) == [2, 0, 1] == list(want_perm)
    assert np.array_equal(Qn, want_Q)


@pytest.mark.parametrize("K,N,M", [(1, 500, 2), (2, 1001, 3), (3, 2000, 4), (20, 3001, 3), (50, 777, 2)])
def test_batch_entry_matches_the_restatement(K, N, M):
    rng = np.random.default_rng(K + N + M)
    # slices of one labelling with the labels shuffled per slice (what label switching looks like), plus noise
    base = _probs(rng, N, K)
    cube = np.empty((N, K, M))
    for m in range(M):
        cube[:, :, m] = base[:, rng.permutation(K)] * 0.9 + _probs(rng, N, K) * 0.1
    cube[:7, :, 0] = 0.0                                          # exact zeros: replaced by 1e-6
    Q, perm = bm.stephens_batch(cube)
    want_Q, want_perm, t = sr.batch(cube)
    assert t == 100
    assert np.array_equal(perm, want_perm)
    pr = np.where(cube == 0, 1e-6, cube)
    scale = np.abs(pr).sum(axis=2) / M
    assert np.all(np.abs(Q - want_Q) <= 1e-12 * scale)
    Q2, perm2 = bm.stephens_batch(cube)
    assert np.array_equal(Q, Q2) and np.array_equal(perm, perm2)


def _compare(device, hook, st, with_pi):
    assert st.min_margin >= 1e-9, st.min_margin      # the restatement's choices are far from ties
    keys = ["alpha", "permutations", "z", "theta", "z_original", "theta_original"] + (["pi"] if with_pi else [])
    for k in keys:
        assert np.array_equal(device[k], hook[k], equal_nan=True), k


CASES = [("K3_N1000_P5", 3, 7), ("K2_N1000_P5", 2, 3)]


@pytest.mark.parametrize("name,K,seed", CASES)
def test_collapsed_and_dp_runs_match_the_hook_path(name, K, seed):
    X = load_dataset(name)
    N = X.shape[0]
    z0 = np.random.default_rng(seed).integers(1, K + 1, N).astype(np.int32)
    kw = dict(alpha=1.0, burnin=6, relabel=True, burnrelabel=3, seed=seed, initial_K=z0)
    st = sr.Stephens()
    dev = bm.gibbs_collapsed(X, 12, K, stephens="device", **kw)
    hook = bm.gibbs_collapsed(X, 12, K, stephens=st, **kw)
    _compare(dev, hook, st, False)
    plain = bm.gibbs_collapsed(X, 12, K, alpha=1.0, burnin=6, seed=seed, initial_K=z0)
    assert np.array_equal(dev["z_original"], plain["z"])
    for s in range(dev["z"].shape[0]):
        pm = dev["permutations"][s]
        assert np.array_equal(dev["z"][s], pm[dev["z_original"][s] - 1] + 1)
    # the DP sampler: unused labels are all-zero columns (tie rule), the new-cluster column is not
    st = sr.Stephens()
    kw = dict(alpha=1.0, burnin=6, relabel=True, burnrelabel=3, maxK=K + 2, seed=seed)
    dev = bm.gibbs_dp(X, 12, stephens="device", **kw)
    hook = bm.gibbs_dp(X, 12, stephens=st, **kw)
    _compare(dev, hook, st, False)


@pytest.mark.parametrize("name,K,seed", CASES)
def test_stickbreaking_and_full_runs_match_the_hook_path(name, K, seed):
    X = load_dataset(name)
    rng = np.random.default_rng(seed)
    pi0, th0 = rng.dirichlet(np.ones(K)), rng.random((K, X.shape[1]))
    for fn in (bm.gibbs_stickbreaking, bm.gibbs_full):
        kw = dict(alpha=1.0, burnin=5, relabel=True, burnrelabel=3, seed=seed, initial_pi=pi0, initial_theta=th0)
        st = sr.Stephens()
        dev = fn(X, 11, K, stephens="device", **kw)
        hook = fn(X, 11, K, stephens=st, **kw)
        _compare(dev, hook, st, True)
        plain = fn(X, 11, K, alpha=1.0, burnin=5, seed=seed, initial_pi=pi0, initial_theta=th0)
        assert np.array_equal(dev["z_original"], plain["z"]) and np.array_equal(dev["pi"], plain["pi"])


def test_north_star_shaped_runs_match_the_hook_path():
    N, P, K = 100_000, 50, 20
    X, _, _, _ = synth(N, P, K, 21)
    rng = np.random.default_rng(4)
    z0 = rng.integers(1, K + 1, N).astype(np.int32)
    st = sr.Stephens()
    kw = dict(alpha=1.0, burnin=4, relabel=True, burnrelabel=2, seed=5, initial_K=z0)
    _compare(bm.gibbs_collapsed(X, 7, K, stephens="device", **kw), bm.gibbs_collapsed(X, 7, K, stephens=st, **kw),
             st, False)
    st = sr.Stephens()
    kw = dict(alpha=1.0, burnin=4, relabel=True, burnrelabel=2, maxK=K, seed=5)   # every label in use: no ties
    _compare(bm.gibbs_dp(X, 7, stephens="device", **kw), bm.gibbs_dp(X, 7, stephens=st, **kw), st, False)
    pi0, th0 = rng.dirichlet(np.ones(K)), rng.random((K, P))
    for fn in (bm.gibbs_stickbreaking, bm.gibbs_full):
        st = sr.Stephens()
        kw = dict(alpha=1.0, burnin=4, relabel=True, burnrelabel=2, seed=5, initial_pi=pi0, initial_theta=th0)
        _compare(fn(X, 7, K, stephens="device", **kw), fn(X, 7, K, stephens=st, **kw), st, True)


def test_device_stephens_plugs_into_the_hook_path():
    X = load_dataset("K3_N1000_P5")
    z0 = np.random.default_rng(7).integers(1, 4, X.shape[0]).astype(np.int32)
    kw = dict(alpha=1.0, burnin=6, relabel=True, burnrelabel=3, seed=7, initial_K=z0)
    dev = bm.gibbs_collapsed(X, 12, 3, stephens="device", **kw)
    hook = bm.gibbs_collapsed(X, 12, 3, stephens=bm.DeviceStephens(0), **kw)
    for k in ("permutations", "z", "theta", "z_original", "theta_original"):
        assert np.array_equal(dev[k], hook[k], equal_nan=True), k


def test_errors_are_clean_and_the_library_stays_usable():
    X, _, _, _ = synth(2000, 10, 3, 2)
    with pytest.raises(bm.BmmError, match="128"):
        bm.gibbs_stickbreaking(X, 8, 129, burnin=4, relabel=True, burnrelabel=2, seed=1, stephens="device")
    with pytest.raises(ValueError, match="burnin >= 2"):
        bm.gibbs_collapsed(X, 8, 3, burnin=1, relabel=True, stephens="device")
    # a window that cannot fit: 2e6 x 128 doubles per sweep, 2000 sweeps (4 TB)
    Xb = np.zeros((2_000_000, 2), dtype=np.int32, order="F")
    with pytest.raises(bm.BmmError, match="bytes"):
        bm.gibbs_stickbreaking(Xb, 2002, 128, burnin=2001, relabel=True, burnrelabel=2000, seed=1, stephens="device")
    got = bm.gibbs_collapsed(X, 8, 3, burnin=4, relabel=True, burnrelabel=2, seed=1, stephens="device")
    assert got["z"].shape == (4, 2000) and sorted(got["permutations"][0]) == [0, 1, 2]
