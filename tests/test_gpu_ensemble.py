"""An ensemble of exact chains (include/bmm_mcmc.h "ensemble of exact chains"): every chain of
bm.gibbs_ensemble against the oracle's batch = 1 chain under seed + c, as raw bytes (so NaN cells count), on shapes chosen
where k_ens_sweep can go wrong; against the device path that exists; the whole bundled set once; and no state shared
between the chains of a launch."""
import numpy as np
import pytest

import bmm_mcmc_amd as bm
from util import load_dataset, synth

pytestmark = pytest.mark.gpu

PRIOR = (0.5, 0.5, 1, 1)  # beta, gamma, a, b


def _same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes(), what


def _starts(seed, chains, K, N):
    return [np.ascontiguousarray(np.random.default_rng(seed + c).integers(1, K + 1, N), dtype=np.int32) for c in range(chains)]


def _check_chain(oracle, got, sampler, X, z0, nsamples, K, alpha, burnin, seed, what):
    """one chain of the ensemble against the oracle's chain at batch = 1 under `seed`"""
    be, ga, a, b = PRIOR
    if sampler == "collapsed":
        tr = oracle.collapsed(X, z0, nsamples, K, alpha, be, ga, a, b, burnin, seed=seed, batch=1)
    else:
        tr = oracle.dp(X, nsamples, alpha, be, ga, a, b, burnin, K, seed=seed, batch=1)
    su = oracle.counts_summary(sampler, X, z0, nsamples, K, alpha, be, ga, a, b, burnin, seed=seed, batch=1)
    if got["z"] is not None:
        _same_bytes(got["z"], tr["z"], what + " z")
    _same_bytes(got["theta"], tr["theta"], what + " theta")
    _same_bytes(got["alpha"], tr["alpha"], what + " alpha")
    _same_bytes(got["theta"], su["theta"], what + " theta (summary)")
    _same_bytes(got["sizes"], su["nk"], what + " sizes")
    _same_bytes(got["z_last"], su["z_last"], what + " z_last")


def _run_and_check(oracle, sampler, X, K, nsamples, chains, alpha, burnin, keep_trace, seed, initial_K=None):
    N = X.shape[0]
    z0s = None
    if sampler == "collapsed":
        z0s = initial_K if initial_K is not None else _starts(seed, chains, K, N)
    outs = bm.gibbs_ensemble(X, nsamples, K, sampler=sampler, chains=chains, alpha=alpha, burnin=burnin, seed=seed,
                             initial_K=initial_K, keep_trace=keep_trace)
    assert len(outs) == chains
    for c, got in enumerate(outs):
        assert (got["z"] is None) == (not keep_trace)
        _check_chain(oracle, got, sampler, X, None if z0s is None else z0s[c], nsamples, K, 0.0 if alpha is None else alpha, burnin,
                     seed + c, "%s chain %d" % (sampler, c))
    return outs


def _three_label_starts(seed, chains, N):
    """starts that use labels 1, 2 and 4 of 5 only: labels 3 and 5 stay empty for ever"""
    return [np.ascontiguousarray(np.array([1, 2, 4], dtype=np.int32)[np.random.default_rng(seed + c).integers(0, 3, N)]) for c in range(chains)]


def _planted(N, P, comps, seed):
    """well separated components: theta 0.05 or 0.95 per (component, feature)"""
    rng = np.random.default_rng(seed)
    th = np.where(rng.random((comps, P)) < 0.5, 0.05, 0.95)
    lab = rng.integers(0, comps, N)
    return np.asfortranarray((rng.random((N, P)) < th[lab]).astype(np.int32))


# (name, sampler, data, K or maxK, sweeps)
SHAPES = {
    "K2_P5_N130": ("collapsed", lambda: synth(130, 5, 2, 1)[0], 2, 30),                # N no multiple of 64; one full group
    "K3_P7": ("collapsed", lambda: synth(200, 7, 3, 2)[0], 3, 24),                     # a partial group of 5; own groups 3 + 3 + 1
    "K5_P33_three_labels": ("collapsed", lambda: synth(257, 33, 3, 3)[0], 5, 16),      # second plane word; empty labels
    "K20_P112": ("collapsed", lambda: synth(150, 112, 6, 4)[0], 20, 12),               # group width 4
    "K64_P9": ("collapsed", lambda: synth(400, 9, 8, 5)[0], 64, 12),                   # every lane a category
    "DP63_P12": ("dp", lambda: synth(200, 12, 5, 6)[0], 63, 14),                       # Kc = 64
    "DP4_four_components": ("dp", lambda: _planted(300, 10, 4, 7), 4, 20),             # the truncation branch
    "DP20_three_components": ("dp", lambda: _planted(256, 8, 3, 8), 20, 20),           # the free-label rule
}
# every value of every axis meets every shape: the concentration sampled and fixed, burn-in 0 and > 0, the label trace
# kept and not, one chain and five (five is no multiple of the chains per workgroup wherever that is above one)
VARIANTS = {
    "sampled_burn0_trace_5chains": dict(alpha=None, burnin=0, keep_trace=True, chains=5),
    "fixed_burn3_notrace_1chain": dict(alpha=1.7, burnin=3, keep_trace=False, chains=1),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_chain_is_the_oracle_chain(oracle, shape, variant):
    sampler, data, K, sweeps = SHAPES[shape]
    v = VARIANTS[variant]
    X = data()
    N, P = X.shape
    seed = 1000 + 17 * sorted(SHAPES).index(shape)
    initial_K = _three_label_starts(seed, v["chains"], N) if shape == "K5_P33_three_labels" else None
    outs = _run_and_check(oracle, sampler, X, K, sweeps + 1, v["chains"], v["alpha"], v["burnin"], v["keep_trace"], seed, initial_K)
    plan = bm.ensemble_plan(sampler, N, P, K, v["chains"])
    if shape == "K20_P112":
        assert plan["group_width"] == 4 and plan["launches_per_sweep"] == 2  # 128 rows a launch at P = 112
    elif v["chains"] == 5:
        assert plan["chains_per_workgroup"] == 4 and plan["workgroups"] == 2  # the second workgroup holds one chain
    if shape == "K5_P33_three_labels":
        for o in outs:
            assert (o["sizes"][:, [2, 4]] == 0).all() and np.isnan(o["theta"][[2, 4]]).all()
    if shape == "DP4_four_components":  # truncated: a draw of "new" with maxK - 1 clusters in use goes to the smallest one
        for o in outs:
            assert (o["sizes"][:, :K - 1] > 0).all(axis=1).any(), "the first maxK - 1 labels were never all in use"
    if shape == "DP20_three_components":  # clusters open and empty again: labels are freed and taken anew
        used = np.stack([(o["sizes"] > 0).sum(axis=1) for o in outs])
        assert used.max() > used.min()


def test_a_sweep_over_several_launches(oracle):
    """N above the rows of one launch: the state crosses launches in global memory, the terms are rebuilt from it"""
    X = synth(2100, 5, 2, 9)[0]
    assert bm.ensemble_plan("collapsed", 2100, 5, 2, 2)["launches_per_sweep"] == 2
    _run_and_check(oracle, "collapsed", X, 2, 5, 2, None, 1, True, 77)
    _run_and_check(oracle, "dp", X, 6, 5, 1, None, 0, True, 78)


def test_three_hundred_chains_every_one_compared(oracle):
    X = synth(130, 5, 2, 1)[0]
    _run_and_check(oracle, "collapsed", X, 2, 7, 300, None, 1, True, 5000)  # 6 sweeps


@pytest.fixture(scope="module")
def k2n100():
    return load_dataset("K2_N100_P5")


def test_equal_to_the_device_path_that_exists_collapsed(k2n100):
    old = bm.gibbs_collapsed(k2n100, 21, 2, burnin=2, seed=31, batch=1, chains=3)
    new = bm.gibbs_ensemble(k2n100, 21, 2, sampler="collapsed", chains=3, burnin=2, seed=31)
    for c in range(3):
        for key in ("z", "theta", "alpha"):
            _same_bytes(new[c][key], old[c][key], "chain %d %s" % (c, key))


def test_equal_to_the_device_path_that_exists_dp(k2n100):
    for c in range(2):
        old = bm.gibbs_dp(k2n100, 21, burnin=2, maxK=10, seed=41 + c, batch=1)
        new = bm.gibbs_ensemble(k2n100, 21, 10, sampler="dp", chains=2, burnin=2, seed=41)[c]
        for key in ("z", "theta", "alpha"):
            _same_bytes(new[key], old[key], "chain %d %s" % (c, key))


def test_the_whole_bundled_set_once(oracle):
    X = load_dataset("K3_N1000_P5")
    outs = _run_and_check(oracle, "collapsed", X, 3, 41, 8, None, 4, True, 2024)  # 40 sweeps
    # ... and straight into the stand-alone tools
    r = bm.rhat([o["alpha"][:, 0] for o in outs])
    assert np.isfinite(r)


def test_no_state_is_shared_between_chains():
    X = synth(200, 7, 3, 2)[0]
    seed = 900
    z0s = _starts(seed, 5, 3, 200)
    five = bm.gibbs_ensemble(X, 15, 3, chains=5, burnin=0, seed=seed)
    for c in range(5):
        alone = bm.gibbs_ensemble(X, 15, 3, chains=1, burnin=0, seed=seed + c, initial_K=[z0s[c]])[0]
        for key in ("z", "theta", "alpha", "sizes", "z_last"):
            _same_bytes(five[c][key], alone[key], "chain %d %s" % (c, key))
    dp5 = bm.gibbs_ensemble(X, 15, 8, sampler="dp", chains=5, burnin=0, seed=seed)
    for c in range(5):
        alone = bm.gibbs_ensemble(X, 15, 8, sampler="dp", chains=1, burnin=0, seed=seed + c)[0]
        for key in ("z", "theta", "alpha", "sizes", "z_last"):
            _same_bytes(dp5[c][key], alone[key], "dp chain %d %s" % (c, key))
