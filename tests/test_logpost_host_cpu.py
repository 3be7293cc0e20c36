"""The host statement of the log joint (bmm_spec.h log_joint_spec, built as tests/logpost/logpost_host.cpp) against the
SciPy restatement (tests/logpost_ref.py), within eps (LGAMMA_ULPS + 2 + depth) sum max(1, |v_i|) over every lgamma_ /
log_ value entering (tests/logpost_host.py: bound).  The device is held to this program bit for bit on the GPU
(tests/test_gpu_logpost.py), so the two together hold the device to the restatement.  Without the log joint in
bmm_spec.h the program does not build."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_ref  # noqa: E402
import logpost_host as host  # noqa: E402
import logpost_ref as ref  # noqa: E402


def _state(N, P, K, used, seed):
    """N rows of P features on `used` of K labels (the others empty), labels scattered over 0 .. K-1"""
    rng = np.random.default_rng(seed)
    labels = rng.choice(K, size=used, replace=False)
    z = labels[rng.integers(used, size=N)]
    theta = rng.random((K, P))
    X = (rng.random((N, P)) < theta[z]).astype(np.int64)
    return X, z


# (model, N, P, K, labels in use): cell counts below, at and above one pass of the 256 lanes, P past one pass, empty labels
CASES = [
    ("collapsed", 40, 5, 3, 3), ("collapsed", 300, 32, 32, 32), ("collapsed", 200, 41, 25, 20), ("collapsed", 40, 7, 20, 6),
    ("full", 65, 130, 4, 4), ("dp", 90, 12, 30, 3), ("dp", 1, 3, 4, 1), ("stickbreaking", 64, 9, 6, 4),
    ("stickbreaking", 63, 300, 3, 3), ("collapsed", 500, 1024, 13, 13), ("collapsed", 400, 6, 70, 50),
]


@pytest.mark.parametrize("model,N,P,K,used", CASES)
@pytest.mark.parametrize("sample_alpha", [False, True])
def test_the_host_statement_is_the_restatement_within_the_bound(model, N, P, K, used, sample_alpha):
    X, z = _state(N, P, K, used, seed=N + P)
    Nk, S = ref.counts(X, z, K)
    kw = dict(sample_alpha=sample_alpha, a=2.0, b=0.5)
    beta, gamma = (0.5, 0.5) if model == "dp" else (0.7, 1.9)
    bits, vals = host.run(model, Nk, S, N, 1.3, beta, gamma, **kw)
    host.check(model, vals, Nk, S, N, 1.3, beta, gamma, **kw)
    assert vals[3] == (vals[0] + vals[1]) + vals[2]
    bits2, _ = host.run(model, Nk, S, N, 1.3, beta, gamma, **kw)
    assert np.array_equal(bits, bits2)


@pytest.mark.parametrize("P,n_out", [(5, 2), (41, 17), (300, 299), (64, 0), (33, 33)])
def test_a_feature_mask_pools_the_excluded_features(P, n_out):
    N, K = 80, 6
    X, z = _state(N, P, K, 4, seed=P)
    Nk, S = ref.counts(X, z, K)
    mask = np.ones(P, dtype=np.uint8)
    mask[np.random.default_rng(P).choice(P, size=n_out, replace=False)] = 0
    kw = dict(mask=mask, rho=0.3, sample_alpha=True, a=1.0, b=1.0)
    _, vals = host.run("collapsed", Nk, S, N, 0.8, 0.5, 1.5, **kw)
    host.check("collapsed", vals, Nk, S, N, 0.8, 0.5, 1.5, **kw)
    if n_out == 0:  # every feature included: the likelihood and the prior of the chain without a mask, bit for bit
        bits, _ = host.run("collapsed", Nk, S, N, 0.8, 0.5, 1.5, **kw)
        plain, _ = host.run("collapsed", Nk, S, N, 0.8, 0.5, 1.5, sample_alpha=True, a=1.0, b=1.0)
        assert np.array_equal(bits[:2], plain[:2])


@pytest.mark.parametrize("k_open", [1, 3, 5])
def test_the_allocation_model_reads_the_open_labels(k_open):
    N, P, maxK = 50, 9, 5
    X, z = _state(N, P, k_open, max(1, k_open - 1), seed=k_open)
    Nk, S = ref.counts(X, z, maxK)
    lpk = alloc_ref.poisson_prior(maxK)
    kw = dict(k_open=k_open, log_prior_k=lpk)
    _, vals = host.run("allocation", Nk, S, N, 0.9, 0.5, 0.8, **kw)
    host.check("allocation", vals, Nk, S, N, 0.9, 0.5, 0.8, **kw)
    want = alloc_ref.log_target(k_open, z, X, 0.9, 0.5, 0.8, lpk)
    assert abs((vals[0] + vals[1]) - want) <= host.bound("allocation", Nk, S, N, 0.9, 0.5, 0.8, **kw)
