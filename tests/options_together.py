"""The options of the gibbs_* wrappers armed together: the table of what each keyword is, the split of a call's keywords
into the chain and its observers, a byte-exact comparison of results, and the cases tests/test_gpu_options_together.py
runs.  Nothing here touches a device at import: an object that needs one (bm.DeviceStephens) is a Factory, made when
the case runs.

A keyword is one of four kinds:
  chain     changes what is sampled (known=, missing=, split_merge=, temper=, the priors and the starts, ...);
  observer  reads state only: its result may depend on the chain and on the observers in its own group, on nothing else;
  modifier  a setting of one observer (its `owner`), which travels with it;
  shape     where and how loudly the run happens (device, devices, debug).
An observer that reads another observer's result is in one group with it: credible_ball and ecr_pivot="partition" with
partition=, ecr_pivot="map" with logpost= (which it implies)."""
import inspect
from collections import namedtuple

import numpy as np

import bmm_mcmc_amd as bm

WRAPPERS = ("gibbs_collapsed", "gibbs_dp", "gibbs_stickbreaking", "gibbs_full", "gibbs_allocation")

CHAIN = ("data", "nsamples", "K", "maxK", "alpha", "beta", "gamma", "a", "b", "burnin", "seed", "batch", "initial_K",
         "initial_pi", "initial_theta", "K0", "prior_k", "moves", "eject_a", "chains", "known", "allowed", "missing",
         "split_merge", "split_merge_scans", "select_features", "rho", "init", "init_iters", "temper", "swap_every",
         "temper_hottest")
OBSERVERS = ("newdata", "loo", "partition", "logpost", "pair_check", "summary", "relabel", "credible_ball")
MODIFIERS = {"predictive_trace": "newdata", "responsibilities": "newdata", "newdata_missing": "newdata",
             "partition_stride": "partition", "similarity_of": "partition", "partition_search": "partition",
             "ecr_pivot": "relabel", "ecr_max_iter": "relabel", "burnrelabel": "relabel", "stephens": "relabel",
             "pair_check_stride": "pair_check", "pair_check_trace": "pair_check",
             "summary_pivot": "summary", "summary_stride": "summary", "keep_trace": "summary"}
SHAPE = ("device", "devices", "debug")

KINDS = {**{k: "chain" for k in CHAIN}, **{k: "observer" for k in OBSERVERS}, **{k: "modifier" for k in MODIFIERS},
         **{k: "shape" for k in SHAPE}}

# the top-level keys of a result that an observer owns (a relabelling also rewrites z and theta: the trace as sampled
# is then z_original / theta_original)
RESULT_KEYS = {"newdata": ("predictive",), "loo": ("loo",), "partition": ("partition",), "logpost": ("logpost",),
               "pair_check": ("pair_check",), "summary": ("summary",), "credible_ball": ("partition",),
               "relabel": ("permutations", "z", "theta", "z_original", "theta_original", "ecr")}
POOLED_KEYS = ("partition",)  # with chains > 1: one dict over the stacked traces, shared by every chain object


def signature_names():
    """every parameter name of the five wrappers, and every name the run_options block takes"""
    names = set(bm._RUN_OPTIONS)
    for w in WRAPPERS:
        names |= set(inspect.signature(getattr(bm, w)).parameters)
    return names


def wrapper_takes(wrapper, name):
    return name in inspect.signature(getattr(bm, wrapper)).parameters or (
        name in bm._RUN_OPTIONS and "partition" in inspect.signature(getattr(bm, wrapper)).parameters)


def _on(v):
    return not (v is None or v is False)


def split(kwargs):
    """(base, groups): the chain and shape keywords (and observers that are switched off, modifiers without their
    observer: they arm nothing), and the list of observer groups, each a dict of an observer, its modifiers and the
    observers that read its result.  {**base, **g1, **g2, ...} has the items of kwargs."""
    unknown = sorted(set(kwargs) - set(KINDS))
    if unknown:
        raise KeyError("not classified: %s" % ", ".join(unknown))
    armed = [k for k in kwargs if KINDS[k] == "observer" and _on(kwargs[k])]
    leader = {k: k for k in armed}
    pivot = kwargs.get("ecr_pivot", "iterative")
    needs = []
    if "credible_ball" in leader:
        needs.append(("credible_ball", "partition"))
    if "relabel" in leader and isinstance(pivot, str) and kwargs["relabel"] == "ecr":
        if pivot == "partition":
            needs.append(("relabel", "partition"))
        if pivot == "map" and "logpost" in leader:
            needs.append(("relabel", "logpost"))
    for reader, read in needs:
        if read not in leader:
            raise ValueError("%s reads %s=, which is not armed" % (reader, read))
        old, new = leader[reader], leader[read]
        for k in leader:
            if leader[k] == old:
                leader[k] = new
    base, groups = {}, {}
    for k, v in kwargs.items():
        owner = k if KINDS[k] == "observer" else MODIFIERS.get(k)
        if owner in leader:
            groups.setdefault(leader[owner], {})[k] = v
        else:
            base[k] = v
    return base, [groups[k] for k in armed if k in groups]


def group_keys(group):
    """the top-level result keys a group owns"""
    keys = []
    for k in group:
        for r in RESULT_KEYS.get(k, ()):
            if r not in keys:
                keys.append(r)
    if group.get("relabel") == "ecr" and group.get("ecr_pivot") == "map" and "logpost" not in keys:
        keys.append("logpost")  # (implied)
    if group.get("relabel") is True and "ecr" in keys:
        keys.remove("ecr")
    return keys


# ---------------------------------------------------------------- results compared leaf by leaf, on bytes
def _leaf(obj):
    """what two leaves must share: (type, dtype, shape, bytes)"""
    if isinstance(obj, np.ndarray):
        if obj.dtype == object:
            return ("ndarray", "object", obj.shape, tuple(obj.ravel().tolist()))
        return ("ndarray", str(obj.dtype), obj.shape, np.ascontiguousarray(obj).tobytes())
    if isinstance(obj, np.generic):
        return (type(obj).__name__, str(obj.dtype), (), obj.tobytes())
    if isinstance(obj, float):
        return ("float", None, None, np.float64(obj).tobytes())
    return (type(obj).__name__, None, None, obj)


def diff_leaves(got, want, path=""):
    """The paths at which two results differ, by the walk of schema() in tests/test_gpu_run_driver.py: dicts key by key in
    order, lists and tuples item by item, and leaves by type, dtype, shape and raw bytes (a NaN equals only a NaN of the
    same payload, 0.0 is not -0.0).  A container whose keys or length differ is named itself, with the keys both hold
    still walked."""
    if isinstance(got, dict) and isinstance(want, dict):
        out = [] if list(got) == list(want) else [path + "{keys}"]
        for k in got:
            if k in want:
                out += diff_leaves(got[k], want[k], "%s/%s" % (path, k))
        return out
    if isinstance(got, (list, tuple)) and type(got) is type(want):
        out = [] if len(got) == len(want) else [path + "[len]"]
        for i, (g, w) in enumerate(zip(got, want)):
            out += diff_leaves(g, w, "%s[%d]" % (path, i))
        return out
    if isinstance(got, (dict, list, tuple)) or isinstance(want, (dict, list, tuple)):
        return [path]
    a, b = _leaf(got), _leaf(want)
    return [] if a[:3] == b[:3] and a[3] == b[3] else [path]


def pick(result, keys):
    """the sub-dict of the named top-level keys that the result has, in the order of the result"""
    return {k: v for k, v in result.items() if k in keys}


# ---------------------------------------------------------------- the data: that of tests/test_gpu_run_driver.py
N, K, M, NS, SEED = 257, 6, 5, 6, 11
BURNINS = (0, 2)


def _data(P):
    rng = np.random.default_rng(5)
    theta = 0.1 + 0.8 * rng.random((3, P))
    rows = (rng.random((N + M, P)) < theta[rng.integers(0, 3, N + M)]).astype(np.int32)
    return np.asfortranarray(rows[:N]), np.asfortranarray(rows[N:])


P = 33            # two plane words, one live bit in the second
P_GENERIC = 130   # past the 128 features of the table kernels: the generic resample kernel, without a debug switch
X, XNEW = _data(P)
XG, XGNEW = _data(P_GENERIC)
DATA = {"layout": (X, XNEW), "generic": (XG, XGNEW)}
MISS = np.zeros((N, P), dtype=bool)
MISS[np.random.default_rng(6).integers(0, N, 20), np.random.default_rng(7).integers(0, P, 20)] = True
KNOWN = np.zeros(N, dtype=np.int64)
KNOWN[:6] = [1, 1, 2, 2, 3, 3]


class Factory:
    """a keyword value made when the case runs: what it makes may touch a device"""

    def __init__(self, make):
        self.make = make


Refusal = namedtuple("Refusal", "exception code words")  # code: BmmError.code, or None for a refusal of the wrapper
Case = namedtuple("Case", "wrapper data nsamples kwargs burnins refusals seed")

TOGETHER = dict(newdata=XNEW, partition="binder", partition_search=True, logpost=True, pair_check=[0, 5, 32], known=KNOWN,
                summary=True)
TOGETHER_NA = dict(TOGETHER, pair_check=None, missing=MISS, newdata_missing=XNEW > 0)
FREE = dict(newdata=XNEW, predictive_trace=True, responsibilities=True, loo="trace", partition="vi", partition_search=True,
            credible_ball={"membership": True}, logpost=True, pair_check=[0, 5, 32], summary="counts")
STRIDES = dict(partition="binder", partition_stride=2, pair_check=[0, 5, 32], pair_check_stride=3, pair_check_trace=True,
               summary=True, summary_stride=2, newdata=XNEW, predictive_trace=True)
GENERIC = dict(TOGETHER, newdata=XGNEW, pair_check=[0, 5, 129])
# DESIGN.md "relabel = TRUE": Stephens' relabelling has no Q without the batch step at sweep burnin - 1
NO_BATCH_STEP = Refusal("ValueError", None, "relabel on the device needs the batch step")
NO_Q = Refusal("ValueError", None, "Q and p must both be N x K")  # the hook path: online() is handed the Q that never was


# The seed is that of the layout test but for two cases, where an armed option has to have done something for the
# equalities to mean anything: at seed 11 the search of generic_dp starts from an estimate no single row improves (P = 130
# separates the clusters within six sweeps), and the cold rung of temper_observed accepts no exchange (about one seed in a
# hundred does at N = 257: the rungs' log likelihoods are a hundred nats apart once the chains have settled).
def _case(wrapper, _data="layout", _nsamples=NS, _burnins=BURNINS, _refusals=None, _seed=SEED, **kw):
    return Case(wrapper, _data, _nsamples, kw, _burnins, _refusals or {}, _seed)


CASES = {
    # ---- the cases of tests/test_gpu_run_driver.py, keyword for keyword
    "collapsed_together": _case("gibbs_collapsed", **TOGETHER),
    "dp_together": _case("gibbs_dp", **TOGETHER),
    "stickbreaking_together": _case("gibbs_stickbreaking", **TOGETHER),
    "full_together": _case("gibbs_full", **TOGETHER),
    "collapsed_together_missing": _case("gibbs_collapsed", **TOGETHER_NA),
    "dp_together_missing": _case("gibbs_dp", **TOGETHER_NA),
    "stickbreaking_together_missing": _case("gibbs_stickbreaking", **TOGETHER_NA),
    "full_together_missing": _case("gibbs_full", **TOGETHER_NA),
    "collapsed_stephens_device": _case("gibbs_collapsed", relabel=True, burnrelabel=2, stephens="device", newdata=XNEW,
                                       predictive_trace=True, responsibilities=True, loo=True, _refusals={0: NO_BATCH_STEP}),
    "full_stephens_device": _case("gibbs_full", relabel=True, burnrelabel=2, stephens="device", partition="vi",
                                  _refusals={0: NO_BATCH_STEP}),
    "dp_stephens_hook": _case("gibbs_dp", relabel=True, burnrelabel=2, stephens=Factory(lambda: bm.DeviceStephens(0)),
                              logpost=True, _refusals={0: NO_Q}),
    "dp_ecr_iterative": _case("gibbs_dp", relabel="ecr", loo="trace"),
    "full_ecr_partition": _case("gibbs_full", relabel="ecr", ecr_pivot="partition", partition="binder", similarity_of=[0, 1, 256]),
    "stickbreaking_ecr_map": _case("gibbs_stickbreaking", relabel="ecr", ecr_pivot="map", loo=True),
    "collapsed_temper": _case("gibbs_collapsed", temper=2, logpost=True),
    "collapsed_kmodes_features": _case("gibbs_collapsed", init="kmodes", select_features=True, loo=False),
    "dp_features": _case("gibbs_dp", select_features=True, rho=0.4),
    "dp_split_merge": _case("gibbs_dp", split_merge=1, newdata=XNEW, newdata_missing=XNEW > 0, responsibilities=True),
    "full_keep_trace_false": _case("gibbs_full", summary="counts", summary_pivot=None, keep_trace=False, known=KNOWN),
    "collapsed_chains_2": _case("gibbs_collapsed", chains=2, init="kmodes", partition="binder", partition_search=True, logpost=True,
                                relabel="ecr", ecr_pivot="partition"),
    "stickbreaking_chains_2": _case("gibbs_stickbreaking", chains=2, relabel="ecr", ecr_pivot="map"),
    "allocation": _case("gibbs_allocation", partition="vi", logpost=True, split_merge=1),
    # ---- nothing held: everything that reads, together
    "free_collapsed": _case("gibbs_collapsed", **FREE),
    "free_dp": _case("gibbs_dp", **FREE),
    "free_stickbreaking": _case("gibbs_stickbreaking", **FREE),
    "free_full": _case("gibbs_full", **FREE),
    # ---- three recorders with three bases and strides in one run
    "strides_collapsed": _case("gibbs_collapsed", _nsamples=14, _burnins=(0, 3), **STRIDES),
    "strides_full": _case("gibbs_full", _nsamples=14, _burnins=(0, 3), **STRIDES),
    # ---- the generic resample kernel beside the predictive and the folds that share its scratch
    "generic_collapsed": _case("gibbs_collapsed", _data="generic", **GENERIC),
    "generic_dp": _case("gibbs_dp", _data="generic", _seed=16, **GENERIC),
    # ---- folds split around the exchange point of a ladder
    "temper_observed": _case("gibbs_collapsed", _nsamples=14, _seed=79, temper=[1, 0.6, 0.3], swap_every=2, logpost=True,
                             pair_check=[0, 5, 32], newdata=XNEW, predictive_trace=True, partition="binder"),
}
DRIVER_CASES = tuple(list(CASES)[:22])
PARAMS = [(name, b) for name in CASES for b in CASES[name].burnins]


def call(case, burnin, kwargs=None):
    """one run of the case's wrapper with `kwargs` (default: all of the case's): Factories made, credible_ball handed
    through bm.run_options"""
    kw = dict(case.kwargs if kwargs is None else kwargs)
    for k, v in kw.items():
        if isinstance(v, Factory):
            kw[k] = v.make()
    ball = kw.pop("credible_ball", None)
    Xd = DATA[case.data][0]
    fn = getattr(bm, case.wrapper)
    args = (Xd, case.nsamples) if case.wrapper == "gibbs_dp" else (Xd, case.nsamples, K)
    if case.wrapper == "gibbs_dp":
        kw["maxK"] = K
    with bm.run_options(**({"credible_ball": ball} if ball is not None else {})):
        return fn(*args, burnin=burnin, seed=case.seed, **kw)
