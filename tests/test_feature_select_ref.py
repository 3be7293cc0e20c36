"""The restatement of the feature-selection sampler (tests/feature_select_ref.py) against brute force: its two
conditionals are the conditionals of the enumerated joint posterior over (partition, mask), and one restated sweep
leaves that joint invariant.  And the wrappers' refusals, which need no device."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feature_select_ref as fsr  # noqa: E402
import split_merge_ref as smr  # noqa: E402

ALPHA, BETA, GAMMA, RHO = 1.3, 0.5, 0.5, 0.3


@pytest.fixture(scope="module")
def five_rows():
    rng = np.random.default_rng(5)
    X = (rng.random((5, 3)) < [0.7, 0.4, 0.5]).astype(np.int64)
    parts, ms, W = fsr.joint_posterior(X, ALPHA, BETA, GAMMA, RHO)
    assert len(parts) == 52 and len(ms) == 8
    return X, parts, ms, W


def test_gamma_conditional_is_the_conditional_of_the_enumerated_joint(five_rows):
    X, parts, ms, W = five_rows
    mi = {tuple(m): k for k, m in enumerate(ms)}
    worst = 0.0
    for si, z in enumerate(parts):
        z = np.asarray(z)
        Nk, S = fsr.counts(X, z, z.max() + 1)
        p = fsr.gamma_prob(fsr.gamma_logit(Nk, S, BETA, GAMMA, RHO))
        for m in ms:
            for d in range(3):
                m1, m0 = m.copy(), m.copy()
                m1[d], m0[d] = 1, 0
                w1, w0 = W[si, mi[tuple(m1)]], W[si, mi[tuple(m0)]]
                worst = max(worst, abs(p[d] - w1 / (w1 + w0)))
    print("gamma conditional: worst deviation %.3e" % worst)
    assert worst <= 1e-12


def test_masked_dp_z_conditional_is_the_conditional_of_the_enumerated_joint(five_rows):
    X, parts, ms, W = five_rows
    index = {s: k for k, s in enumerate(parts)}
    K, worst = 6, 0.0
    for si, z in enumerate(parts):
        z = np.asarray(z)
        for mi, m in enumerate(ms):
            for i in range(5):
                cond = fsr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, m, "dp", rows=[i])[0]
                want = np.zeros(K)
                for k in np.flatnonzero(cond > 0):
                    z2 = z.copy()
                    z2[i] = k
                    want[k] = W[index[smr.canon(z2)], mi]
                assert len(np.flatnonzero(cond > 0)) == len(set(np.delete(z, i))) + 1  # every used label and one new
                worst = max(worst, np.abs(cond - want / want.sum()).max())
    print("dp z conditional: worst deviation %.3e" % worst)
    assert worst <= 1e-12


def test_masked_collapsed_z_conditional_is_the_conditional_of_the_finite_joint(five_rows):
    X, _, ms, _ = five_rows
    K, worst, seen = 2, 0.0, 0
    for zt in itertools.product(range(K), repeat=5):
        z = np.array(zt)
        if len(set(zt)) < K:
            continue  # (the sampler gives an empty label probability 0 for ever: not the model's conditional)
        for m in ms:
            for i in range(5):
                if np.sum(z == z[i]) == 1:
                    continue  # (nor a row that sits alone: its label is empty once it is out)
                cond = fsr.z_conditional(X, z, K, ALPHA, BETA, GAMMA, m, "collapsed", rows=[i])[0]
                lw = []
                for k in range(K):
                    z2 = z.copy()
                    z2[i] = k
                    lw.append(fsr.log_joint_finite(X, z2, m, K, ALPHA, BETA, GAMMA, RHO))
                w = np.exp(np.array(lw) - max(lw))
                worst = max(worst, np.abs(cond - w / w.sum()).max())
                seen += 1
    print("collapsed z conditional: %d cases, worst deviation %.3e" % (seen, worst))
    assert seen > 0 and worst <= 1e-12


def test_one_restated_sweep_leaves_the_enumerated_joint_invariant(five_rows):
    X, parts, ms, W = five_rows
    T = fsr.sweep_matrix(X, parts, ms, ALPHA, BETA, GAMMA, RHO, K=6)
    np.testing.assert_allclose(T.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    pi = W.reshape(-1)
    dev = np.abs(pi @ T - pi).max()
    print("invariance: worst deviation %.3e" % dev)
    assert dev <= 1e-12


def test_the_uniform_is_a_stream_of_its_own():
    # stream id 9, counter (d, 0, sweep): differs from the split-merge stream's block of the same counter
    u = fsr.fs_uniform(17, 3, 4)
    r = smr.philox4x32_10((3, 0, 4, 8), (17, 0))
    assert 0.0 <= u < 1.0 and u != smr.u01(r[0], r[1])
    assert u == fsr.fs_uniform(17, 3, 4) and u != fsr.fs_uniform(17, 4, 4) and u != fsr.fs_uniform(17, 3, 5)


def test_wrapper_refusals_need_no_device():
    import importlib
    bmm = importlib.import_module("bmm-mcmc_amd")
    X = (np.random.default_rng(1).random((40, 6)) < 0.5).astype(np.int32)
    new = X[:3]
    for kw in (dict(rho=0.0), dict(rho=1.0), dict(rho=-0.1), dict(chains=2), dict(newdata=new), dict(loo=True)):
        with pytest.raises(ValueError):
            bmm.gibbs_collapsed(X, 10, 3, select_features=True, **kw)
        with pytest.raises(ValueError):
            bmm.gibbs_dp(X, 10, maxK=5, select_features=True, **kw)
    with pytest.raises(ValueError):
        bmm.gibbs_dp(X, 10, maxK=5, select_features=True, split_merge=1)
    with pytest.raises(ValueError):
        bmm.gibbs_dp(X, 10, maxK=5, select_features=True, beta=0.5, gamma=0.7)
