"""The VI branch of the greedy search on the device (k_ps_phi, k_ps_score<VI>, k_ps_total<VI>, the host's keep-best;
DESIGN.md section 27) held to a restatement decision by decision.  On partition_search_ref.VI_CASES the reference
(search_vi_margins, np.longdouble) decides every row and every keep-best comparison by a gap of at least 2^10 x 2
derived error bounds (tests/test_partition_search_ref.py asserts that, and that the cases reach every path of the VI
kernels), so no correct binary64 implementation can decide otherwise: the result and the whole course of the search
equal the reference with ==, the totals lie within the project's bound for a VI total.  The first pass alone, one
batch over all rows, is compared choice by choice, so that a wrong cell names its row and slot.  Through a run: the
armed search against the reference on the returned trace."""
import functools

import numpy as np
import pytest

import bmm_mcmc_amd as bm
import partition_ref as pr
import partition_search_ref as ref
from util import synth

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(case):
    z, start, res = ref.vi_reference(case)
    z.setflags(write=False)
    start.setflags(write=False)
    return z, start, res


def _condition(res, Kc, Ka, N, S):
    return (res["score_margin"], 2 ** 10 * 2 * ref.score_error_bound(N, S),
            res["total_margin"], 2 ** 10 * 2 * pr.vi_bound(max(Kc, Ka), N) * S * N)


def _equals_the_reference(got, want, z, Kc, Ka, name):
    """the device's result dict against search_vi_margins': everything that is a decision or an integer with ==,
    every VI total within vi_bound(max(Kc, Ka), N) S N"""
    S, N = z.shape
    bound = pr.vi_bound(max(Kc, Ka), N) * S * N
    pairs = list(zip(got["total"], want["pass_total"])) + [(got["loss"] * S * N, want["total"]), (got["start_loss"] * S * N, want["start_total"])]
    worst = max(abs(a - b) for a, b in pairs)
    sm, sneed, tm, tneed = _condition(want, Kc, Ka, N, S)
    print("vi %s: score_margin %.3g (needs %.3g), total_margin %.3g (needs %.3g), %d structural ties; largest |total - reference| %.3g (bound %.3g); "
          "%d passes, batches %s, moved %s, %s, %d clusters"
          % (name, sm, sneed, tm, tneed, want["structural_ties"], worst, bound, got["passes"], got["batch"], got["moved"],
             want["stopped"], got["n_clusters"]))
    assert got["moved"] == want["moved"] and got["batch"] == want["batch"] and got["passes"] == want["passes"]
    assert got["converged"] == want["converged"] and got["n_clusters"] == want["n_clusters"]
    assert got["z"].dtype == np.int32 and np.array_equal(got["z"], want["z"])
    assert got["binder2"] == ref.State(z, got["z"], Kc, Ka).binder2() == want["binder2"]
    assert got["start_binder2"] == want["start_binder2"]
    assert len(got["total"]) == len(want["pass_total"])
    for a, b in pairs:
        assert abs(a - b) <= bound, (a, b)


@pytest.mark.parametrize("case", ref.VI_CASES, ids=ref.vi_case_id)
def test_vi_equals_the_restatement(case):
    Kc, N, S, batch, min_batch, _, Ka, _, _ = case
    z, start, want = _reference(case)
    assert ref.margins_hold(want, Kc, Ka, N, S)
    got = bm.partition_search(z, "vi", start=start, batch=batch, min_batch=min_batch, max_clusters=Ka, Kc=Kc,
                              max_passes=ref.VI_MAX_PASSES.get(case, 50))
    assert want["start_binder2"] == ref.State(z, start, Kc, Ka).binder2()
    _equals_the_reference(got, want, z, Kc, Ka, ref.vi_case_id(case))


@pytest.mark.parametrize("case", ref.VI_FIRST_PASS, ids=ref.vi_case_id)
def test_first_pass_choices(case):
    """one pass over one batch of all N rows: the pass lowers the total (in the reference, by more than 2^11 bounds),
    so the result is the choice of every row against the start state"""
    Kc, N, S, _, _, _, Ka, _, _ = case
    z, start, _ = _reference(case)
    want = ref.search_vi_margins(z, Kc, start, N, N, max_passes=1, Ka=Ka, keep_scores=True)
    assert want["moved"][0] > 0 and want["pass_total"][0] < want["start_total"] and ref.margins_hold(want, Kc, Ka, N, S)
    assert np.array_equal(want["z"], want["first_choice"])
    got = bm.partition_search(z, "vi", start=start, batch=N, min_batch=N, max_passes=1, max_clusters=Ka, Kc=Kc)
    bad = np.flatnonzero(got["z"] != want["first_choice"])
    if len(bad):
        i = int(bad[0])
        G = want["first_scores"][i]
        d, r = int(got["z"][i]), int(want["first_choice"][i])
        raise AssertionError(
            "%d of %d rows choose another slot than the reference; the first is row %d, in slot %d (1-based): the device "
            "chooses slot %d, the reference slot %d, which the reference scores %.6g lower (g = %s)"
            % (len(bad), N, i, int(start[i]), d, r, float(G[d - 1] - G[r - 1]), np.array2string(np.asarray(G, dtype=float), precision=4)))
    assert got["moved"] == want["moved"] and got["passes"] == 1 and got["batch"] == [N]
    assert abs(got["total"][0] - want["pass_total"][0]) <= pr.vi_bound(max(Kc, Ka), N) * S * N


def test_a_given_start_inside_fewer_slots():
    """Ka < Kc: the rows stay inside 1 .. Ka, and the course is the reference's"""
    cases = [c for c in ref.VI_CASES if c[6] < c[0]]
    assert cases
    for case in cases:
        Kc, N, S, batch, min_batch, _, Ka, _, _ = case
        z, start, want = _reference(case)
        assert start.max() <= Ka and sum(want["moved"]) > 0
        got = bm.partition_search(z, "vi", start=start, batch=batch, min_batch=min_batch, max_clusters=Ka, Kc=Kc)
        assert got["z"].min() >= 1 and got["z"].max() <= Ka and got["n_clusters"] <= Ka
        _equals_the_reference(got, want, z, Kc, Ka, ref.vi_case_id(case))


RUN_SEED = 4  # chosen on the device: the trace of this run meets the margin condition (asserted below)
RUN_SEARCH = {"batch": 200, "min_batch": 5, "max_passes": 20}


def test_through_a_run():
    """gibbs_collapsed(partition="vi", partition_search=...): the armed search against the reference on the returned
    trace, from the returned estimate.  The trace comes from the device, so the margin condition is asserted on it
    here before anything is compared."""
    X = synth(600, 8, 3, 21)[0]
    out = bm.gibbs_collapsed(X, 14, 3, burnin=4, seed=RUN_SEED, partition="vi", partition_search=dict(RUN_SEARCH))
    z, s = out["z"], out["partition"]["search"]
    S, N = z.shape
    want = ref.search_vi_margins(z, 3, out["partition"]["z"], RUN_SEARCH["batch"], RUN_SEARCH["min_batch"],
                                 RUN_SEARCH["max_passes"], Ka=3)
    sm, sneed, tm, tneed = _condition(want, 3, 3, N, S)
    assert sm >= sneed and tm >= tneed, \
        "the trace of seed %d does not meet the margin condition (score %.3g < %.3g or total %.3g < %.3g): choose another RUN_SEED" \
        % (RUN_SEED, sm, sneed, tm, tneed)
    assert sum(want["moved"]) > 0
    _equals_the_reference(s, want, z, 3, 3, "through a run, seed %d" % RUN_SEED)
