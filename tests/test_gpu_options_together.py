"""What the options of a gibbs_* call compute when several are armed in one call (the table: tests/options_together.py).
For every case and burn-in, with `all` the run of the case's keywords, `plain` the run of its chain keywords alone and
`alone[g]` the run of the chain keywords with one observer group:

  (a) the observers change nothing: every key of `plain` -- the traces and the results of the chain options -- is in
      `all` with the same bytes (under a relabelling the traces as sampled, z_original / theta_original);
  (b) each observer keeps its own result: what group g owns in `all` has the bytes it has in `alone[g]`;
  (c) the result belongs to the trace that came back: every observer of `all` recomputed from (X, z, theta, pi, alpha) of
      `all` -- through the stand-alone calls with == on bits, as the option's own test file compares a run with them, and
      through the NumPy restatements (predictive_ref, loo_ref, predictive_na_ref, summary_ref) at their files' tolerances.

(c) is left out where the trace does not hold what the observer read: with missing= the completed matrix of a kept
sweep is not returned (the parts that read labels alone stay: partition, search, the summary's memberships), under
keep_trace=False there is no label trace, and the predictive rows of a tempered run are those before the exchange
(DESIGN.md section 21).  Every case also asserts that what it arms did something: the equalities say nothing of a
constraint that never reverted a draw or a search that moved no row.

Tolerances, none new: rtol 1e-12 on log densities and ell, atol 1e-11 on responsibilities and cell means (test_gpu_predict.py,
test_gpu_loo.py, test_gpu_predict_na.py).  A fold that is compared with the fold of the restated trace (there is no
device trace to fold) gets what the two allow together: 1e-12, the files' bound on a fold of the device's own trace, and
rtol 1e-12 of the largest |log density| that went into it."""
import functools

import numpy as np
import pytest

import bmm_mcmc_amd as bm
import loo_ref as lref
import options_together as OT
import predictive_na_ref as nref
import predictive_ref as pref
import summary_ref as sref
from test_gpu_loo import _check_fold
from test_gpu_predict import RTOL, _check_fold_lppd

pytestmark = pytest.mark.gpu

ATOL_RESP = 1e-11   # test_gpu_predict.py, test_gpu_predict_na.py: responsibilities, cell means
ATOL_FOLD = 1e-12   # test_gpu_predict.py, test_gpu_loo.py: lppd / log_cpo against the fold of the trace
SAMPLER = {"gibbs_collapsed": "collapsed", "gibbs_dp": "dp", "gibbs_stickbreaking": "stickbreaking", "gibbs_full": "full",
           "gibbs_allocation": "allocation"}
RUNNABLE = [(n, b) for n, b in OT.PARAMS if b not in OT.CASES[n].refusals]
REFUSED = [(n, b) for n, b in OT.PARAMS if b in OT.CASES[n].refusals]
# (c) is about the trace: not with missing= (the partition, the search and the summary's memberships stay), nor without one
LABELS_ONLY = [n for n, c in OT.CASES.items() if "missing" in c.kwargs]
NO_TRACE = [n for n, c in OT.CASES.items() if c.kwargs.get("keep_trace") is False]
# the cases whose summary must have relabelled a sweep: a pivot, free labels, and a chain that has not settled (fourteen
# sweeps, or the random starting labels as the pivot)
RELABELLED = (("free_collapsed", 0), ("strides_collapsed", 0), ("strides_collapsed", 3), ("strides_full", 0), ("strides_full", 3))


class Runs:
    """the runs of one case and burn-in, made once and shared by (a), (b) and (c); nothing here is written to later"""

    def __init__(self, name, burnin):
        self.case, self.burnin = OT.CASES[name], burnin
        self.base, self.groups = OT.split(self.case.kwargs)
        self.all = OT.call(self.case, burnin)
        self.plain = OT.call(self.case, burnin, self.base)
        self._alone = {}

    def alone(self, i):
        if i not in self._alone:
            self._alone[i] = OT.call(self.case, burnin=self.burnin, kwargs={**self.base, **self.groups[i]})
        return self._alone[i]


@functools.lru_cache(maxsize=None)
def runs(name, burnin):
    return Runs(name, burnin)


def chains_of(out):
    return out if isinstance(out, list) else [out]


def test_the_table_holds_the_layout_cases_keyword_for_keyword():
    """(the values, which tests/test_options_together_cpu.py cannot see without importing a module that makes a device
    object: the names are held there)"""
    import test_gpu_run_driver as D
    assert list(D.CASES) == list(OT.DRIVER_CASES) and (D.N, D.P, D.K, D.M, D.NS, D.SEED) == (OT.N, OT.P, OT.K, OT.M, OT.NS, OT.SEED)
    assert D.X.tobytes() == OT.X.tobytes() and D.XNEW.tobytes() == OT.XNEW.tobytes() and D.BURNINS == OT.BURNINS
    for name, fn in D.CASES.items():
        cell = dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__)))
        case, kw = OT.CASES[name], dict(cell["kw"])
        assert cell["fn"] == case.wrapper and kw.pop("maxK", OT.K) == OT.K and cell["args"] == (() if "dp" in case.wrapper else (OT.K,))
        assert list(kw) == list(case.kwargs), name
        for k, v in kw.items():
            w = case.kwargs[k]
            w = w.make() if isinstance(w, OT.Factory) else w
            assert type(v) is type(w) and (OT.diff_leaves(v, w) == [] if not isinstance(v, bm.DeviceStephens) else True), (name, k)


@pytest.mark.parametrize("name,burnin", REFUSED)
def test_a_documented_refusal_is_raised_by_the_group_that_asks_for_it(name, burnin):
    case = OT.CASES[name]
    want = case.refusals[burnin]
    base, groups = OT.split(case.kwargs)
    OT.call(case, burnin, base)  # the chain alone runs
    asked = [g for g in groups if "relabel" in g]
    for kw in [case.kwargs] + [{**base, **g} for g in asked]:
        with pytest.raises(Exception) as e:
            OT.call(case, burnin, kw)
        assert type(e.value).__name__ == want.exception and getattr(e.value, "code", None) == want.code and want.words in str(e.value)
    for g in groups:
        if g not in asked:
            OT.call(case, burnin, {**base, **g})


# ---------------------------------------------------------------- (a)
def _did_something(r, a, p):
    """each armed option of the case, chain option or observer, has done what makes the equalities mean something"""
    kw, S = r.case.kwargs, r.case.nsamples - r.burnin
    if "known" in kw:
        assert a["constraints"]["reverted"] > 0 and a["constraints"]["n_known"] == 6
    if "missing" in kw:
        assert a["missing"]["n_cells"] > 0
        unarmed = OT.call(r.case, r.burnin, {k: v for k, v in r.base.items() if k != "missing"})
        assert unarmed["z"].tobytes() != p["z"].tobytes()
    if OT._on(kw.get("partition_search")):
        assert sum(a["partition"]["search"]["moved"]) > 0
    if OT._on(kw.get("credible_ball")):
        ball = a["partition"]["credible_ball"]
        assert ball["n_in"] >= 1 and ball["sim"].any()
    if OT._on(kw.get("summary")):
        rows = sref.folded_rows(S, kw.get("summary_stride", 1), 0 if r.burnin else 1)
        assert a["summary"]["n_folded"] == len(rows) >= 2
    if OT._on(kw.get("pair_check")):
        rows = sref.folded_rows(S, kw.get("pair_check_stride", 1), 0 if r.burnin else 1)
        assert a["pair_check"]["n_folded"] == len(rows) >= 2 and (a["pair_check"]["n_z"] > 0).any()
    if OT._on(kw.get("partition")):
        assert a["partition"]["loss"].size >= 2 and a["partition"]["n_used"] >= S - 1
    if OT._on(kw.get("newdata")):
        assert np.isfinite(a["predictive"]["lppd"]).all()
        if "newdata_missing" in kw:
            assert a["predictive"]["cells"]["n_cells"] == int((OT.XNEW > 0).sum()) > 0
    if OT._on(kw.get("loo")):
        assert a["loo"]["n_folded"] == S - (0 if r.burnin else 1)
    if OT._on(kw.get("logpost")) or kw.get("ecr_pivot") == "map":
        scored = int((p["z"].min(axis=1) >= 1).sum()) if int(kw.get("chains", 1)) > 1 else S - (0 if r.burnin else 1)
        assert a["logpost"]["n_used"] == scored >= S - 1  # (several chains are scored afterwards: every row that is a partition)
    if kw.get("relabel") == "ecr":
        assert a["ecr"]["n_used"] >= (S - 1) * int(kw.get("chains", 1))
    if kw.get("split_merge"):
        assert sum(v for k, v in a["split_merge"].items() if "proposed" in k) > 0
    if "temper" in kw:
        assert a["temper"]["proposed"].sum() > 0
    if OT._on(kw.get("select_features")):
        assert a["features"]["n_folded"] == S - (0 if r.burnin else 1)


@pytest.mark.parametrize("name,burnin", RUNNABLE)
def test_a_the_observers_change_nothing(name, burnin):
    r = runs(name, burnin)
    A, Pl = chains_of(r.all), chains_of(r.plain)
    assert len(A) == len(Pl) == int(r.case.kwargs.get("chains", 1))
    for c, (a, p) in enumerate(zip(A, Pl)):
        relabelled = "z_original" in a
        assert relabelled == OT._on(r.case.kwargs.get("relabel"))
        for k, v in p.items():
            if k == "permutations" and relabelled:
                continue  # (the relabelling's own)
            if k == "z" and a["z"] is None:
                assert r.case.kwargs["keep_trace"] is False
                continue
            got = a[{"z": "z_original", "theta": "theta_original"}.get(k, k) if relabelled else k]
            if k == "init":  # (device_ms is a clock)
                got, v = ({f: w for f, w in d.items() if f != "device_ms"} for d in (got, v))
            assert OT.diff_leaves(got, v) == [], (c, k)
        assert not set(p) & {"predictive", "loo", "partition", "logpost", "pair_check", "summary", "ecr", "z_original"}
        _did_something(r, a, p)
    if name == "temper_observed":
        print("temper: proposed", A[0]["temper"]["proposed"], "accepted", A[0]["temper"]["accepted"])
        assert A[0]["temper"]["accepted"][0] > 0  # the cold rung took another rung's state
    if (name, burnin) in RELABELLED:
        su = A[0]["summary"]
        assert (su["permutations"] != np.arange(OT.K)).any() and su["pivot"] is not None


# ---------------------------------------------------------------- (b)
@pytest.mark.parametrize("name,burnin", RUNNABLE)
def test_b_each_observer_keeps_its_own_result(name, burnin):
    r = runs(name, burnin)
    seen = set()
    for i, g in enumerate(r.groups):
        keys = OT.group_keys(g)
        A, B = chains_of(r.all), chains_of(r.alone(i))
        pooled = [k for k in keys if k in OT.POOLED_KEYS] if len(A) > 1 else []
        for c, (a, b) in enumerate(zip(A, B)):
            own = [k for k in keys if k not in pooled]
            assert set(own) <= set(a), (own, list(a))
            assert OT.diff_leaves(OT.pick(a, own), OT.pick(b, own)) == [], (c, sorted(g))
        for k in pooled:
            assert all(o[k] is A[0][k] for o in A)
            assert OT.diff_leaves(A[0][k], B[0][k]) == [], (k, sorted(g))
        seen |= set(keys)
    # nothing in `all` is outside (a) and (b): a key is the chain's or some group's
    for a, p in zip(chains_of(r.all), chains_of(r.plain)):
        assert set(a) <= set(p) | seen, sorted(set(a) - set(p) - seen)


# ---------------------------------------------------------------- (c)
def _same(got, want, what):
    d = OT.diff_leaves(got, want)
    assert d == [], (what, d)


def _first_assigned(z):
    use = [s for s in range(z.shape[0]) if z[s].min() >= 1]
    assert use == list(range(use[0], z.shape[0]))  # only the starting row of a run without burn-in is unassigned
    return use[0]


def _c_partition(pt, z, kw, K):
    """the point estimate, the similarity, the search and the ball from the (stacked) trace z of assigned rows"""
    q = bm.partition_distances(z, pt["criterion"], kw.get("partition_stride", 1), Kc=K)
    want = {"criterion": q["criterion"], "loss": q["loss"], "binder2": q["binder2"], "z": q["z"], "n_used": q["n_used"]}
    _same({k: pt[k] for k in want}, want, "partition")
    if "similarity_of" in kw:
        _same(pt["similarity"], bm.posterior_similarity(z, kw["similarity_of"]), "similarity")
    centre = pt["z"]
    if OT._on(kw.get("partition_search")):
        _same(pt["search"], bm.partition_search(z, pt["criterion"], start=pt["z"], Kc=K), "search")
        centre = pt["search"]["z"]
    else:
        assert "search" not in pt
    return q["best"], centre


def _c_ball(ball, z, centre, pt, kw, K, first):
    opts = kw["credible_ball"]
    alone = bm.credible_ball(z, centre, pt["criterion"], membership=opts["membership"], Kc=K, max_clusters=K)
    assert ball["centre"] == ("search" if "search" in pt else "visited")
    alone["centre"] = ball["centre"]
    for q in ("horizontal", "upper", "lower"):  # the bounds name rows of the run's trace
        alone[q]["sweep"] += first
    _same(ball, alone, "credible ball")


def _c_ecr(o, z, theta, kw, K, first, pivot):
    """the relabelling of the trace as sampled, rows first.. ; pivot: the labels the run was to agree with, None: voted"""
    alone = bm.ecr_relabel(z[first:], K, pivot, kw.get("ecr_max_iter", 50), theta=theta[:, :, first:])
    ecr = o["ecr"]
    _same(np.ascontiguousarray(o["permutations"][first:]), np.ascontiguousarray(alone["permutations"]), "permutations")
    _same(np.ascontiguousarray(o["z"][first:]), np.ascontiguousarray(alone["z"]), "relabelled z")
    _same(np.ascontiguousarray(o["theta"][:, :, first:]), np.ascontiguousarray(alone["theta"]), "relabelled theta")
    _same(ecr["agree"][first:], alone["agree"], "agree")
    _same(ecr["pivot"], alone["pivot"], "pivot")
    assert (ecr["iterations"], ecr["converged"]) == (alone["iterations"], alone["converged"])
    if first:  # the starting row: as sampled
        assert np.array_equal(o["permutations"][0], np.arange(K)) and ecr["agree"][0] == 0 and np.array_equal(o["z"][0], z[0])


def _c_logpost(lp, X, z, o, case, first):
    sampler, S = SAMPLER[case.wrapper], z.shape[0]
    if sampler == "allocation":
        rows = bm.log_joint(X, z[first:], sampler, OT.K, 1.0, k_open=o["K"][first:], prior_k="poisson")
    else:  # (the cases leave alpha to be sampled)
        rows = bm.log_joint(X, z[first:], sampler, OT.K, o["alpha"].ravel()[first:], sample_alpha=True)
    for k in ("log_lik", "log_prior", "log_hyper", "log_joint"):
        assert np.isnan(lp[k][:first]).all()
        _same(lp[k][first:], rows[k], k)
    lj = lp["log_joint"]
    best = first + int(np.argmax(lj[first:]))  # the first maximum
    assert lp["best"] == best and (lj[first:best] < lj[best]).all() and lp["n_used"] == S - first
    _same(lp["z_map"], np.ascontiguousarray(z[best]), "z_map")
    _same(lp["ess"], bm.ess(lj[first:]), "ess")


def _c_pair_check(pc, X, z, kw, first):
    S = z.shape[0]
    rows = sref.folded_rows(S, kw.get("pair_check_stride", 1), first)
    alone = bm.pair_check(X, z[rows], OT.K, features=kw["pair_check"])
    zr, x2 = alone.pop("z"), alone.pop("x2")
    if kw.get("pair_check_trace"):
        for name, want in (("z", zr), ("x2", x2)):
            full = np.full((S, want.shape[1]), np.nan)
            full[rows] = want
            alone[name] = full
    _same(pc, alone, "pair check")


def _c_summary(su, z, theta, alpha, kw, K, first, labels_only):
    """as _check of tests/test_gpu_summary.py: the permutations are those of the pinned relabelling of the folded rows,
    everything else the restatement's"""
    S = z.shape[0]
    stride, pivot = kw.get("summary_stride", 1), kw.get("summary_pivot", "first")
    z0 = np.where(z >= 1, z - 1, -1).astype(np.int32)
    rows = sref.folded_rows(S, stride, first)
    rest = [s for s in range(S) if s not in rows]
    assert su["n_folded"] == len(rows)
    assert np.array_equal(su["agree"][rest], [-1] * len(rest)) and np.array_equal(su["permutations"][rest], np.tile(np.arange(K), (len(rest), 1)))
    if pivot is None:
        assert su["pivot"] is None and not su["agree"][rows].any() and np.array_equal(su["permutations"][rows], np.tile(np.arange(K), (len(rows), 1)))
        relabelled, given = z[rows], None
    else:
        assert isinstance(pivot, str) and np.array_equal(su["pivot"], z[sref.first_assigned(z0)])
        e = bm.ecr_relabel(z[rows], K, pivot=su["pivot"])
        assert np.array_equal(e["permutations"], su["permutations"][rows]) and np.array_equal(e["agree"], su["agree"][rows])
        relabelled, given = e["z"], su["pivot"] - 1
    ref = sref.summarise(z0, K, theta, alpha, pivot=given, stride=stride, first_fold=first,
                         permutations=None if pivot is None else su["permutations"])
    assert ref["folded"] == rows
    if pivot is not None:
        assert np.array_equal(ref["agree"], su["agree"])
    if "counts" in su:
        assert np.array_equal(su["counts"], np.stack([(relabelled == k + 1).sum(axis=0) for k in range(K)], axis=1))
        assert su["counts"].dtype == np.uint32 and np.array_equal(su["counts"], ref["counts"])
    assert np.array_equal(su["z_hat"], ref["z_hat"] + 1) and np.array_equal(su["n_max"], ref["n_max"])
    assert su["size_sum"].dtype == np.int64 and np.array_equal(su["size_sum"], ref["size_sum"])
    if labels_only:
        return
    assert su["theta_sum"].tobytes() == np.asfortranarray(ref["theta_sum"]).tobytes()
    assert su["theta_sq"].tobytes() == np.asfortranarray(ref["theta_sq"]).tobytes()
    assert np.array_equal(su["theta_n"], ref["theta_n"]) and su["alpha_sum"].tobytes() == ref["alpha_sum"].tobytes()


def _states(o, X, z, theta, sampler, first):
    """per kept sweep from `first`: what the restatements take -- the counts recounted from the labels and the traced
    alpha (the counting samplers), or the traced pi and theta"""
    for s in range(first, z.shape[0]):
        if sampler in ("stickbreaking", "full"):
            yield s, (o["pi"][s], theta[:, :, s])
        else:
            Nk, Sx = pref.counts_from_labels(X, z[s], OT.K)
            yield s, (Nk, Sx, float(o["alpha"].ravel()[s]), X.shape[0], 0.5, 0.5)


def _fold_bound(trace):
    return ATOL_FOLD + RTOL * np.max(np.abs(trace), axis=0)


def _c_predictive(pr, o, X, Xnew, z, theta, kw, sampler, first):
    S, explicit = z.shape[0], sampler in ("stickbreaking", "full")
    miss = kw.get("newdata_missing")
    if miss is not None:
        rows, cols = nref.cells_of(miss)
        parts_of = nref.explicit_parts if explicit else nref.collapsed_parts if sampler == "collapsed" else nref.dp_parts
        st = [nref.state(Xnew, miss, parts_of(*args)) for _, args in _states(o, X, z, theta, sampler, first)]
        ld, rp, lj = (np.stack([t[q] for t in st]) for q in range(3))
    else:
        terms_of = pref.explicit_terms if explicit else pref.collapsed_terms if sampler == "collapsed" else pref.dp_terms
        terms = [terms_of(Xnew, *args) for _, args in _states(o, X, z, theta, sampler, first)]
        ld, rp = np.stack([pref.logdens(t) for t in terms]), np.stack([pref.resp(t) for t in terms])
    n = S - first
    if "logdens" in pr:
        assert pr["logdens"].shape == (S, Xnew.shape[0]) and np.isnan(pr["logdens"][:first]).all()
        got = pr["logdens"][first:]
        zero = ld == 0.0  # (a row with every cell missing)
        np.testing.assert_allclose(got[~zero], ld[~zero], rtol=RTOL, atol=0)
        np.testing.assert_allclose(got[zero], ld[zero], rtol=0, atol=ATOL_FOLD)
        _check_fold_lppd(sampler, got, pr["lppd"], n, Xnew.shape[0])
    print(sampler, "lppd: largest difference from the fold of the restated trace", np.max(np.abs(pr["lppd"] - pref.lppd(ld))))
    assert np.all(np.abs(pr["lppd"] - pref.lppd(ld)) <= _fold_bound(ld))
    if "resp" in pr:
        np.testing.assert_allclose(pr["resp"], rp.mean(axis=0), rtol=0, atol=ATOL_RESP)
    if miss is not None:
        cells = pr["cells"]
        assert np.array_equal(cells["rows"], rows) and np.array_equal(cells["cols"], cols) and cells["n_folded"] == n
        np.testing.assert_allclose(cells["mean"], nref.fold(ld, lj, rows)[1], rtol=0, atol=ATOL_RESP)


def _c_loo(lo, o, X, z, theta, sampler, first):
    S, explicit = z.shape[0], sampler in ("stickbreaking", "full")
    if explicit:
        ell = np.stack([lref.explicit_ell(X, *args) for _, args in _states(o, X, z, theta, sampler, first)])
    else:
        ell = np.stack([lref.counting_ell(X, z[s], a[0], a[1], a[2], 0.5, 0.5, sampler) for s, a in _states(o, X, z, theta, sampler, first)])
    n = S - first
    assert lo["n_folded"] == n and ("p_waic" in lo) == explicit
    if "ell" in lo:
        assert np.isnan(lo["ell"][:first]).all()
        np.testing.assert_allclose(lo["ell"][first:], ell, rtol=RTOL)
        _check_fold(sampler, lo["ell"][first:], lo, n, X.shape[0])
    want = lref.summary(ell, waic=explicit)
    for key in ("log_cpo", "lppd"):
        print(sampler, key, "largest difference from the fold of the restated trace", np.max(np.abs(lo[key] - want[key])))
        assert np.all(np.abs(lo[key] - want[key]) <= _fold_bound(ell)), key


@pytest.mark.parametrize("name,burnin", [p for p in RUNNABLE if p[0] not in NO_TRACE])
def test_c_the_result_belongs_to_the_trace_that_came_back(name, burnin):
    r = runs(name, burnin)
    case, kw = r.case, r.case.kwargs
    X, Xnew = OT.DATA[case.data]
    sampler, labels_only = SAMPLER[case.wrapper], name in LABELS_ONLY
    A = chains_of(r.all)
    first = 0 if burnin else 1  # row 0 of a run without burn-in is the starting state: NaN, and not folded
    sampled = [(o.get("z_original", o["z"]), o.get("theta_original", o["theta"])) for o in A]
    checked = set()
    # ---- what reads the label trace after the last sweep: over the stacked traces of the chains
    fa = [_first_assigned(z) for z, _ in sampled]
    if OT._on(kw.get("partition")):
        pt = A[0]["partition"]
        zz = np.asfortranarray(np.concatenate([z[f:] for (z, _), f in zip(sampled, fa)], axis=0))
        best, centre = _c_partition(pt, zz, kw, OT.K)
        src = [(c, s) for c, ((z, _), f) in enumerate(zip(sampled, fa)) for s in range(f, z.shape[0])]
        if len(A) > 1:
            assert (pt["chain"], pt["best"]) == src[best]
        else:
            assert pt["best"] == src[best][1]
        assert np.array_equal(pt["z"], sampled[src[best][0]][0][src[best][1]])
        if OT._on(kw.get("credible_ball")):
            _c_ball(pt["credible_ball"], zz, centre, pt, kw, OT.K, fa[0])
            checked.add("credible_ball")
        checked.add("partition")
    for c, (o, (z, theta)) in enumerate(zip(A, sampled)):
        S = z.shape[0]
        assert S == case.nsamples - burnin
        if (OT._on(kw.get("logpost")) or kw.get("ecr_pivot") == "map") and not labels_only:
            if len(A) == 1:
                _c_logpost(o["logpost"], X, z, o, case, first)
            else:  # scored after the run: the rows that are a partition
                lp = o["logpost"]
                rows = bm.log_joint(X, z[fa[c]:], sampler, OT.K, o["alpha"].ravel()[fa[c]:], sample_alpha=True)
                for k in ("log_lik", "log_prior", "log_hyper", "log_joint"):
                    _same(lp[k][fa[c]:], rows[k], k)
                best = fa[c] + int(np.argmax(lp["log_joint"][fa[c]:]))
                assert lp["best"] == best and np.array_equal(lp["z_map"], z[best])
            checked.add("logpost")
        if kw.get("relabel") == "ecr" and len(A) == 1:
            pivot = {"iterative": None, "partition": o["partition"]["z"] if "partition" in o else None,
                     "map": o["logpost"]["z_map"] if "logpost" in o else None}[kw.get("ecr_pivot", "iterative")]
            assert (pivot is None) == (kw.get("ecr_pivot", "iterative") == "iterative")
            _c_ecr(o, z, theta, kw, OT.K, fa[c], pivot)
            checked.add("relabel")
        if OT._on(kw.get("pair_check")) and not labels_only:
            _c_pair_check(o["pair_check"], X, z, kw, first)
            checked.add("pair_check")
        if OT._on(kw.get("summary")):
            _c_summary(o["summary"], z, theta, o["alpha"], kw, OT.K, first, labels_only)
            checked.add("summary")
        if OT._on(kw.get("newdata")) and not labels_only and "temper" not in kw:
            _c_predictive(o["predictive"], o, X, Xnew, z, theta, kw, sampler, first)
            checked.add("newdata")
        if OT._on(kw.get("loo")):
            _c_loo(o["loo"], o, X, z, theta, sampler, first)
            checked.add("loo")
    if kw.get("relabel") == "ecr" and len(A) > 1:  # one relabelling of the stacked traces to one pivot
        top = A[0]["logpost"]["chain"] if kw.get("ecr_pivot") == "map" else None
        pivot = {"iterative": None, "partition": A[0].get("partition", {}).get("z"),
                 "map": None if top is None else A[top]["logpost"]["z_map"]}[kw.get("ecr_pivot", "iterative")]
        alone = bm.ecr_relabel(np.concatenate([z[f:] for (z, _), f in zip(sampled, fa)], axis=0), OT.K, pivot, kw.get("ecr_max_iter", 50))
        at = 0
        for o, (z, theta), f in zip(A, sampled, fa):
            n = z.shape[0] - f
            assert np.array_equal(o["permutations"][f:], alone["permutations"][at:at + n]) and np.array_equal(o["z"][f:], alone["z"][at:at + n])
            assert np.array_equal(o["ecr"]["agree"][f:], alone["agree"][at:at + n]) and np.array_equal(o["ecr"]["pivot"], alone["pivot"])
            assert o["theta"].tobytes() == bm._permute_theta(theta, o["permutations"]).tobytes()
            at += n
        checked.add("relabel")
    # every observer the case arms was recomputed, but those the module's docstring leaves out
    armed = {k for k in kw if OT.KINDS[k] == "observer" and OT._on(kw[k])}
    left_out = set()
    if labels_only:
        left_out = {"newdata", "logpost", "pair_check"}
    if "temper" in kw:
        left_out = {"newdata"}
    if kw.get("relabel") is True:
        left_out = {"relabel"}  # (Stephens' relabelling reads the probabilities of every sweep, which no trace holds)
    assert armed - left_out <= checked, sorted(armed - left_out - checked)
