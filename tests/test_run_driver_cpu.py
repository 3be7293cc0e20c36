"""What the gibbs_* wrappers hand to the library, and what they refuse before they call it, without a device.

`_capi.lib` is replaced by a stub whose every function records its arguments and returns 0; a run entry point
(bmm_*_run*, bmm_multi_run, bmm_alloc_run) records itself and raises, so no result code ever reads an unfilled buffer.
A transcript holds, call by call, the function name, every plain scalar's value, for a pointer only whether it is null,
for a struct passed by reference the same per field -- no addresses.  tests/golden/run_calls.json holds the transcripts
of every case below as recorded at the commit before the four wrappers were folded into one driver; the signatures and
docstring digests of tests/golden/run_api.json were recorded there too.  `python tests/test_run_driver_cpu.py --record`
rewrites both files from the package as it is: only to be run at a commit whose wrappers are known to be right."""
import ctypes as C
import hashlib
import inspect
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bmm_mcmc_amd as bm
from bmm_mcmc_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
API = ("gibbs_collapsed", "gibbs_dp", "gibbs_stickbreaking", "gibbs_full", "gibbs_allocation")
_RUN_ENDINGS = ("_run", "_run_probs", "_run_relabel", "_run_predict")


# ---------------------------------------------------------------- the stub
class _Reached(Exception):
    """a run entry point was called"""


def _field(ftype, v):
    if ftype is C.c_void_p:
        return "null" if v is None else "ptr"
    if issubclass(ftype, (C._Pointer, C._CFuncPtr)):
        return "ptr" if v else "null"
    if issubclass(ftype, C.Array):
        return [type(v).__name__, len(v)]
    return v


def _arg(a):
    if a is None:
        return "null"
    if isinstance(a, (bool, int, float, str)):
        return a
    if isinstance(a, C.c_void_p):
        return "null" if a.value is None else "ptr"
    if isinstance(a, C._SimpleCData):
        return [type(a).__name__, a.value]
    if isinstance(a, C._CFuncPtr):
        return "fn" if a else "null"
    if isinstance(a, C.Array):
        if a._type_ is C.c_void_p:
            return ["table", len(a), ["null" if v is None else "ptr" for v in a]]
        if a._type_ is C.c_int:
            return ["ints", list(a)]
        return "ptr"
    if isinstance(a, C._Pointer):
        return "ptr" if a else "null"
    obj = getattr(a, "_obj", None)  # ctypes.byref(...)
    if isinstance(obj, C.Structure):
        return {type(obj).__name__: {name: _field(ftype, getattr(obj, name)) for name, ftype in obj._fields_}}
    if obj is not None:
        return ["byref", type(obj).__name__]
    raise TypeError("the stub cannot describe %r" % (a,))


class _Stub:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append([name] + [_arg(a) for a in args])
            if name.startswith("bmm_") and name.endswith(_RUN_ENDINGS):
                raise _Reached(name)
            return 0
        return fn


def _transcript(call):
    """the calls a case makes and how it ends: ["reached", entry point], ["raised", type, message] or ["returned"]"""
    stub = _Stub()
    saved = _capi.lib
    _capi.lib = lambda: stub
    try:
        try:
            call()
            end = ["returned"]
        except _Reached as e:
            end = ["reached", str(e)]
        except Exception as e:
            end = ["raised", type(e).__name__, str(e)]
    finally:
        _capi.lib = saved
    return {"calls": stub.calls, "end": end}


# ---------------------------------------------------------------- the cases
N, P, K, M, NS = 10, 3, 3, 4, 6


def _data():
    rng = np.random.default_rng(3)
    X = np.asfortranarray((rng.random((N, P)) < 0.5).astype(np.int32))
    Xn = np.asfortranarray((rng.random((M, P)) < 0.5).astype(np.int32))
    return X, Xn


X, XNEW = _data()
XNA = X.astype(np.float64)
XNA[1, 2] = XNA[7, 0] = np.nan
MISS = np.zeros((N, P), dtype=bool)
MISS[2, 1] = MISS[9, 2] = True
NMISS = np.zeros((M, P), dtype=bool)
NMISS[0, 0] = NMISS[3, 2] = True
KNOWN = np.zeros(N, dtype=np.int64)
KNOWN[0], KNOWN[4] = 1, 2
ALLOWED = np.ones((N, K), dtype=bool)
ALLOWED[3, 0] = False
ALLOWED[6, 1:] = False
Z0 = np.random.default_rng(4).integers(1, K + 1, N).astype(np.int32)
PIVOT = np.random.default_rng(5).integers(1, K + 1, N).astype(np.int32)
PI0 = np.ones(K) / K
TH0 = np.asfortranarray(0.1 + 0.8 * np.random.default_rng(6).random((K, P)))


class _HostStephens:
    """a stand-in for host code on the hook path: never called, the run entry point raises first"""

    def batch(self, p):
        raise AssertionError("not reached")

    def online(self, Q, p, j):
        raise AssertionError("not reached")


SAMPLERS = ("collapsed", "dp", "stickbreaking", "full")
TOGETHER = dict(newdata=XNEW, partition="binder", partition_search=True, logpost=True, pair_check=True, missing=MISS,
                known=KNOWN, summary=True)

# offered by all four samplers: one option at a time, then the documented combination
COMMON = {
    "plain": {},
    "alpha": dict(alpha=1.5, beta=0.4, gamma=0.6, a=2, b=3),
    "burnin_default": dict(burnin=None),
    "burnin_0": dict(burnin=0),
    "device_1": dict(device=1),
    "debug": dict(debug=True),
    "newdata": dict(newdata=XNEW),
    "newdata_trace_resp": dict(newdata=XNEW, predictive_trace=True, responsibilities=True),
    "newdata_missing": dict(newdata=XNEW, newdata_missing=NMISS),
    "newdata_missing_none_set": dict(newdata=XNEW, newdata_missing=np.zeros((M, P), dtype=bool)),
    "partition_binder": dict(partition="binder"),
    "partition_vi_similarity": dict(partition="vi", partition_stride=2, similarity_of=[0, 3, 5]),
    "partition_search": dict(partition="binder", partition_search=True),
    "partition_search_opts": dict(partition="vi", partition_search=dict(batch=4, min_batch=2, max_passes=7, max_clusters=5)),
    "loo": dict(loo=True),
    "loo_trace": dict(loo="trace"),
    "logpost": dict(logpost=True),
    "pair_check": dict(pair_check=True),
    "pair_check_list": dict(pair_check=[2, 0], pair_check_stride=2, pair_check_trace=True),
    "missing_mask": dict(missing=MISS),
    "known": dict(known=KNOWN),
    "summary": dict(summary=True),
    "summary_counts": dict(summary="counts", summary_stride=2),
    "summary_no_pivot": dict(summary=True, summary_pivot=None),
    "summary_given_pivot": dict(summary=True, summary_pivot=PIVOT),
    "keep_trace_false": dict(summary=True, keep_trace=False),
    "relabel_host": dict(relabel=True, burnrelabel=2, stephens=_HostStephens()),
    "relabel_host_newdata": dict(relabel=True, burnrelabel=2, stephens=_HostStephens(), newdata=XNEW),
    "stephens_device": dict(relabel=True, burnrelabel=2, stephens="device"),
    "stephens_device_newdata_partition": dict(relabel=True, burnrelabel=2, stephens="device", newdata=XNEW, partition="binder",
                                              loo=True, logpost=True),
    "stephens_device_unused": dict(stephens="device"),
    "burnrelabel_clamped": dict(relabel=True, burnin=4, burnrelabel=50, stephens=_HostStephens()),
    "ecr_iterative": dict(relabel="ecr", ecr_pivot="iterative", ecr_max_iter=9),
    "ecr_partition": dict(relabel="ecr", ecr_pivot="partition", partition="binder"),
    "ecr_map": dict(relabel="ecr", ecr_pivot="map"),
    "ecr_given": dict(relabel="ecr", ecr_pivot=PIVOT),
    "together": TOGETHER,  # (armed and called; the library then refuses the pair check beside missing cells)
    "together_pair_check": dict(TOGETHER, missing=None),
    "together_missing": dict(TOGETHER, pair_check=None, newdata_missing=NMISS),
    "together_ecr": dict(TOGETHER, summary=None, relabel="ecr", ecr_pivot="partition"),
    "chains_2": dict(chains=2),
    "chains_2_devices": dict(chains=2, devices=[0, 1]),
    "chains_2_missing": dict(chains=2, missing=MISS),
    "chains_2_known": dict(chains=2, known=KNOWN),
    "chains_2_pooled": dict(chains=2, partition="binder", partition_search=True, logpost=True, relabel="ecr", ecr_pivot="map"),
    # pairs the docstrings rule out but the library, not the wrapper, refuses: the wrapper arms both and calls
    "missing_with_loo": dict(missing=MISS, loo=True),
    "known_with_loo": dict(known=KNOWN, loo=True),
    "missing_with_relabel": dict(missing=MISS, relabel=True, burnrelabel=2, stephens="device"),
}
OWN = {
    "collapsed": {
        "missing_na": dict(data_=XNA, missing="na"),
        "initial_K": dict(initial_K=Z0),
        "batch": dict(batch=4),
        "allowed": dict(allowed=ALLOWED),
        "known_allowed": dict(known=KNOWN, allowed=ALLOWED),
        "select_features": dict(select_features=True, rho=0.3),
        "temper_rungs": dict(temper=2, swap_every=2, temper_hottest=0.2),
        "temper_ladder": dict(temper=[1.0, 0.5, 0.25]),
        "kmodes": dict(init="kmodes", init_iters=4),
        "kmodes_with_the_rest": dict(TOGETHER, missing=None, known=None, init="kmodes", loo=True, select_features=False),
        "features_known_partition": dict(select_features=True, known=KNOWN, partition="vi"),
        "chains_2_kmodes": dict(chains=2, init="kmodes"),
        "chains_2_initial_K": dict(chains=2, initial_K=[Z0, Z0[::-1]]),
        "temper_with_relabel": dict(temper=2, relabel=True, burnrelabel=2, stephens="device"),
        "temper_with_features": dict(temper=2, select_features=True),
        "temper_with_summary": dict(temper=2, summary=True),
        "missing_with_kmodes": dict(missing=MISS, init="kmodes"),
    },
    "dp": {
        "batch": dict(batch=4),
        "select_features": dict(select_features=True, rho=0.3),
        "split_merge": dict(split_merge=2),
        "split_merge_scans": dict(split_merge=1, split_merge_scans=3),
        "temper_rungs": dict(temper=3),
        "split_merge_with_the_rest": dict(TOGETHER, missing=None, known=None, split_merge=1, loo="trace"),
        "split_merge_with_known": dict(split_merge=1, known=KNOWN),
        "temper_with_split_merge": dict(temper=2, split_merge=1),
    },
    "stickbreaking": {
        "initial_params": dict(initial_pi=PI0, initial_theta=TH0),
        "chains_2_initial_params": dict(chains=2, initial_pi=[PI0, PI0], initial_theta=[TH0, TH0]),
        "burnrelabel_not_clamped": dict(relabel=True, burnrelabel=50, stephens=_HostStephens()),
    },
    "full": {
        "initial_params": dict(initial_pi=PI0, initial_theta=TH0),
        "allowed": dict(allowed=ALLOWED),
        "known_allowed": dict(known=KNOWN, allowed=ALLOWED),
        "chains_2_initial_params": dict(chains=2, initial_pi=[PI0, PI0], initial_theta=[TH0, TH0]),
    },
}

ALLOCATION = {
    "plain": {},
    "start": dict(K0=3, initial_K=Z0, moves=2, eject_a=2.0, a=0.5, prior_k="uniform", batch=4, device=1),
    "partition": dict(partition="binder", partition_stride=2, similarity_of=[1, 2]),
    "logpost": dict(logpost=True),
    "split_merge": dict(split_merge=2, split_merge_scans=3),
    "ecr": dict(relabel="ecr"),
    "ecr_partition": dict(relabel="ecr", ecr_pivot="partition", partition="vi"),
    "everything": dict(partition="vi", logpost=True, split_merge=1),
}

# refused in Python: the first refusal a caller sees, and the calls made before it
REFUSED = {
    "features_with_newdata": dict(select_features=True, newdata=XNEW),
    "features_with_loo": dict(select_features=True, loo=True),
    "features_with_loo_chains_2": dict(select_features=True, loo=True, chains=2),
    "features_with_bad_loo": dict(select_features=True, loo="all"),
    "features_bad_rho": dict(select_features=True, rho=1.0),
    "summary_with_relabel": dict(summary=True, relabel=True, stephens="device"),
    "summary_with_ecr": dict(summary=True, relabel="ecr"),
    "summary_bad": dict(summary="all"),
    "summary_pivot_bad": dict(summary=True, summary_pivot="last"),
    "summary_pivot_shape": dict(summary=True, summary_pivot=PIVOT[:-1]),
    "keep_trace_without_summary": dict(keep_trace=False),
    "keep_trace_false_with_partition": dict(summary=True, keep_trace=False, partition="binder"),
    "ecr_with_stephens": dict(relabel="ecr", stephens="device"),
    "ecr_partition_without_partition": dict(relabel="ecr", ecr_pivot="partition"),
    "ecr_bad_pivot": dict(relabel="ecr", ecr_pivot="first"),
    "ecr_pivot_shape": dict(relabel="ecr", ecr_pivot=PIVOT[:-1]),
    "search_without_partition": dict(partition_search=True),
    "search_unknown_option": dict(partition="binder", partition_search=dict(passes=3)),
    "search_few_clusters": dict(partition="binder", partition_search=dict(max_clusters=2)),
    "similarity_without_partition": dict(similarity_of=[0, 1]),
    "partition_bad": dict(partition="rand"),
    "partition_bad_stride": dict(partition="binder", partition_stride=0),
    "similarity_out_of_range": dict(partition="binder", similarity_of=[0, N]),
    "loo_bad": dict(loo="all"),
    "kmodes_with_initial_K": dict(init="kmodes", initial_K=Z0),
    "kmodes": dict(init="kmodes"),
    "init_bad": dict(init="kmeans"),
    "init_bad_with_missing_bad": dict(init="kmeans", missing="nan"),
    "init_iters_bad": dict(init="kmodes", init_iters=-1),
    "allowed": dict(allowed=ALLOWED),
    "allowed_shape": dict(allowed=ALLOWED[:, :2]),
    "known_shape": dict(known=KNOWN[:-1]),
    "known_above_K": dict(known=np.where(KNOWN > 0, K + 1, 0)),
    "missing_bad": dict(missing="nan"),
    "missing_shape": dict(missing=MISS[:-1]),
    "data_with_na": dict(data_=XNA),
    "burnin_all": dict(burnin=NS),
    "burnin_negative": dict(burnin=-1),
    "initial_K_shape": dict(initial_K=Z0[:-1]),
    "initial_pi_shape": dict(initial_pi=PI0[:-1]),
    "initial_theta_shape": dict(initial_theta=TH0[:, :-1]),
    "initial_pi_shape_chains_2": dict(chains=2, initial_pi=[PI0, PI0[:-1]], missing=MISS),
    "newdata_columns": dict(newdata=XNEW[:, :-1]),
    "newdata_missing_bad": dict(newdata=XNEW, newdata_missing="nan"),
    "newdata_missing_shape": dict(newdata=XNEW, newdata_missing=NMISS[:-1]),
    "pair_check_one_feature": dict(pair_check=[1]),
    "pair_check_bad_stride": dict(pair_check=True, pair_check_stride=0),
    "temper_too_many": dict(temper=9),
    "split_merge_negative": dict(split_merge=-1),
    "split_merge_with_features": dict(split_merge=1, select_features=True),
    "features_beta_gamma": dict(select_features=True, beta=0.4),
    "loo_chains_2": dict(loo=True, chains=2),
    "newdata_chains_2": dict(newdata=XNEW, chains=2),
    "summary_chains_2": dict(summary=True, chains=2),
    "pair_check_chains_2": dict(pair_check=True, chains=2),
    "features_chains_2": dict(select_features=True, chains=2),
    "split_merge_chains_2": dict(split_merge=1, chains=2),
    "temper_chains_2": dict(temper=2, chains=2),
    "relabel_chains_2": dict(relabel=True, chains=2),
    "relabel_chains_2_armed": dict(relabel=True, chains=2, missing=MISS, known=KNOWN),
    "devices_chains_2_armed": dict(chains=2, devices=[0], missing=MISS),
    "relabel_without_stephens": dict(relabel=True),
    "relabel_without_stephens_newdata": dict(relabel=True, newdata=XNEW, missing=MISS),
    "stephens_bad": dict(stephens="host"),
    "stephens_device_short_burnin": dict(relabel=True, stephens="device", burnin=1, burnrelabel=1),
    "stephens_device_no_batch": dict(relabel=True, stephens="device", burnrelabel=0),
    "stephens_device_before_initial_K": dict(relabel=True, stephens="device", burnrelabel=0, initial_K=Z0[:-1]),
    "stephens_device_before_initial_pi": dict(relabel=True, stephens="device", burnrelabel=0, initial_pi=PI0[:-1]),
}
# (a case that only some of the samplers offering its keywords refuse)
REFUSED_BY = {"features_beta_gamma": ("dp",), "kmodes": ("dp", "stickbreaking", "full"), "allowed": ("dp", "stickbreaking")}

ALLOCATION_REFUSED = {
    "K0_above_maxK": dict(K0=5),
    "relabel_true": dict(relabel=True),
    "ecr_partition_without_partition": dict(relabel="ecr", ecr_pivot="partition"),
    "split_merge_negative": dict(split_merge=-1),
    "split_merge_scans_negative_with_na": dict(split_merge_scans=-1, data_=XNA),
    "initial_K_shape": dict(initial_K=Z0[:-1]),
    "prior_k_bad": dict(prior_k="geometric"),
    "burnin_all": dict(burnin=NS),
    "similarity_without_partition": dict(similarity_of=[0]),
}


def _offered(fn, kw):
    """a case is a case of a sampler only if its public signature has every keyword"""
    names = inspect.signature(fn).parameters
    return all(k in names or k == "data_" for k in kw)


def _call(sampler, kw):
    kw = dict(kw)
    data = kw.pop("data_", X)
    if sampler == "allocation":
        return lambda: bm.gibbs_allocation(data, NS, 4, **{"burnin": 2, "seed": 7, **kw})
    fn = getattr(bm, "gibbs_" + sampler)
    if sampler == "dp":
        return lambda: fn(data, NS, **{"burnin": 2, "seed": 7, "maxK": K, **kw})
    return lambda: fn(data, NS, K, **{"burnin": 2, "seed": 7, **kw})


def _cases(common, own, alloc, only={}):
    out = {}
    for s in SAMPLERS:
        for name, kw in {**common, **own.get(s, {})}.items():
            if _offered(getattr(bm, "gibbs_" + s), kw) and s in only.get(name, SAMPLERS):
                out["%s/%s" % (s, name)] = _call(s, kw)
    for name, kw in alloc.items():
        out["allocation/%s" % name] = _call("allocation", kw)
    return out


MATRIX = _cases(COMMON, OWN, ALLOCATION)
REFUSALS = _cases(REFUSED, {}, ALLOCATION_REFUSED, REFUSED_BY)


def _api():
    return {f: {"signature": str(inspect.signature(getattr(bm, f))),
                "doc_sha256": hashlib.sha256(getattr(bm, f).__doc__.encode()).hexdigest()} for f in API}


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _plain(t):
    return json.loads(json.dumps(t))  # tuples to lists, as the golden file holds them


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("fn", API)
def test_signature_and_docstring_are_the_recorded_ones(fn):
    assert _api()[fn] == _golden("run_api.json")[fn]


def test_every_case_has_a_recorded_counterpart():
    rec = _golden("run_calls.json")
    assert sorted(rec["matrix"]) == sorted(MATRIX)
    assert sorted(rec["refusals"]) == sorted(REFUSALS)


@pytest.mark.parametrize("case", sorted(MATRIX))
def test_the_run_reaches_the_library_as_recorded(case):
    want = _golden("run_calls.json")["matrix"][case]  # (a case without a record fails here: KeyError)
    got = _plain(_transcript(MATRIX[case]))
    assert got["end"][0] == "reached", got["end"]
    assert got == want


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_refusal_is_the_recorded_one(case):
    want = _golden("run_calls.json")["refusals"][case]
    got = _plain(_transcript(REFUSALS[case]))
    assert got["end"][0] == "raised", got["end"]
    assert got == want


def test_the_stub_sees_a_struct_field_by_field():
    """(the recorder itself: a changed scalar, a pointer gone null and another entry point all show)"""
    a = _plain(_transcript(_call("collapsed", dict(partition="binder", partition_stride=2))))
    b = _plain(_transcript(_call("collapsed", dict(partition="vi", partition_stride=3, similarity_of=[1]))))
    (pa,), (pb,) = ([c for c in t["calls"] if c[0] == "bmm_set_partition_summary"] for t in (a, b))
    sa, sb = pa[1]["_PartitionOut"], pb[1]["_PartitionOut"]
    assert (sa["criterion"], sa["stride"], sa["psm_idx"], sa["psm_M"]) == (0, 2, "null", 0)
    assert (sb["criterion"], sb["stride"], sb["psm_idx"], sb["psm_M"]) == (1, 3, "ptr", 1)
    assert a["end"] == ["reached", "bmm_collapsed_run_probs"]
    assert _transcript(_call("dp", dict(newdata=XNEW)))["end"] == ["reached", "bmm_dp_run_predict"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_run_driver_cpu.py --record")
    with open(os.path.join(GOLDEN, "run_api.json"), "w") as f:
        json.dump(_api(), f, indent=1, sort_keys=True)
        f.write("\n")
    rec = {"matrix": {k: _transcript(c) for k, c in sorted(MATRIX.items())},
           "refusals": {k: _transcript(c) for k, c in sorted(REFUSALS.items())}}
    for group, end in (("matrix", "reached"), ("refusals", "raised")):
        for k, t in rec[group].items():
            assert t["end"][0] == end, (group, k, t["end"])
    with open(os.path.join(GOLDEN, "run_calls.json"), "w") as f:
        json.dump(rec, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("recorded %d runs and %d refusals" % (len(rec["matrix"]), len(rec["refusals"])))
