"""bmm_mcmc_amd -- MI355X-native cluster-allocation path of the bmm-mcmc Gibbs samplers.

Host-side mirror of the reference's R wrappers (R/utils.R:23-47, 95-107): the same
function names, argument meaning, defaults and returned objects, over the C ABI in
include/bmm_mcmc.h.  (R is not installed in the build image; the R wrappers and the
.Call shim a maintainer would use are in bmm-mcmc_amd/R and bmm-mcmc_amd/r-shim, see
INTEGRATION.md.)  Returned arrays are laid out like the R objects: `z` is S x N with
1-based labels, `theta` is K x P x S, `alpha` is S x 1, `pi` is S x maxK.

There is no CPU fallback: without the built HIP library and a gfx950 device every
sampler call raises.
"""
import ctypes as _C
import threading as _threading
from collections import namedtuple as _namedtuple

import numpy as _np

from . import _capi
from ._capi import BmmError, NA_INTEGER
from .rdata import read_rdata_matrix  # the package's bundled data sets (data/*.RData) without R

__all__ = ["gibbs_collapsed", "gibbs_dp", "gibbs_stickbreaking", "gibbs_full", "Chain", "BmmError", "NA_INTEGER", "set_progress",
           "default_batch", "sweep_chains", "broadcast_planes", "read_rdata_matrix", "chain_summary", "TOL_PROPORTIONS", "TOL_THETA",
           "stephens_batch", "stephens_online", "stephens_plan", "DeviceStephens", "STEPHENS_MAX_K",
           "partition_distances", "posterior_similarity", "partition_plan", "partition_search", "partition_search_plan", "credible_ball", "credible_ball_plan", "run_options", "PARTITION_MAX_K", "gibbs_allocation", "log_prior_k",
           "ecr_relabel", "ecr_plan", "ECR_MAX_K", "log_joint", "ess", "rhat", "pair_check", "pair_check_plan", "pair_check_pairs", "PAIR_CHECK_MAX_M", "run_bytes", "summary_plan", "Ladder", "temper_ladder", "TEMPER_MAX_RUNGS",
           "categorical", "Categorical", "categorical_plan", "gibbs_ensemble", "ensemble_plan", "ensemble_fold_plan", "ensemble_pool"]

# include/bmm_mcmc.h: the stated tolerance of a batch > 1 against the reference's sequential scan
TOL_PROPORTIONS = 0.015
TOL_THETA = 0.05


def _seed(seed):
    # R draws through the session RNG, so set.seed() fixes the chain; here the global
    # NumPy RNG plays that part when no seed is given.
    if seed is None:
        return int(_np.random.randint(0, 2 ** 31 - 1))
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _burnin(burnin, nsamples):
    if burnin is None:
        burnin = int(round(0.1 * nsamples))  # R/utils.R:25,40,97 (round half even, as R)
    burnin = int(burnin)
    if not 0 <= burnin < nsamples:
        raise ValueError("burnin must be in [0, nsamples)")
    return burnin


def _na_perm(S, K):
    return _np.full((S, K), NA_INTEGER, dtype=_np.int32, order="F")  # uninitialised in the reference


def default_batch(sampler, N):
    return int(_capi.lib().bmm_default_batch(_capi.SAMPLER_CODE[sampler], N))


# ---------------------------------------------------------------- relabel = TRUE
_PROBS_FN = _C.CFUNCTYPE(_C.c_int, _C.c_void_p, _C.c_int, _C.POINTER(_C.c_double))


class _Hooks(_C.Structure):  # bmm_relabel_hooks
    _fields_ = [("burnrelabel", _C.c_int), ("probs_batch", _C.c_void_p), ("batch_done", _PROBS_FN),
                ("on_sample", _PROBS_FN), ("user", _C.c_void_p)]


class _Relabel:
    """The reference's relabel = TRUE bookkeeping (src/collapsed_gibbs.cpp:187-201, 215-217, 232-243) around
    host code that stays what it is: `stephens` supplies the two functions of src/stephens.h,
        stephens.batch(p)          p: (N, K, burnrelabel) cube      -> Q (N, K)       my_stephens_batch
        stephens.online(Q, p, j)   p: (N, K) of sweep j             -> (perm, Q_new)  my_stephens_online
    (perm 0-based, as arma::Row<int>).  The per-sweep probability matrices come from the device."""

    def __init__(self, stephens, N, K, nsamples, burnin, burnrelabel):
        if stephens is None:
            raise NotImplementedError(
                "relabel=TRUE needs Stephens' relabelling (src/stephens.cpp, src/my_lpsolve.cpp): pass "
                "stephens=\"device\" to run it on the device, or stephens=<object with batch(p) and "
                "online(Q, p, j)> to run host code of your own on the probability matrices this build supplies")
        self.st, self.N, self.K, self.burnin = stephens, N, K, burnin
        self.S = nsamples - burnin
        self.W = max(0, int(burnrelabel))
        self.cube = _np.zeros((N, K, max(self.W, 1)), order="F")
        self.Q = None
        self.perms = _np.full((self.S, K), NA_INTEGER, dtype=_np.int32, order="F")
        self.error = None
        self._batch_cb = _PROBS_FN(self._batch_done)
        self._sample_cb = _PROBS_FN(self._on_sample)
        self.hooks = _Hooks(self.W, self.cube.ctypes.data_as(_C.c_void_p), self._batch_cb, self._sample_cb, None)

    def _batch_done(self, user, j, probs):
        try:
            self.Q = _np.asarray(self.st.batch(self.cube[:, :, :self.W]), dtype=_np.float64)
            return 0
        except Exception as e:  # an exception must not unwind through the C frames
            self.error = e
            return 1

    def _on_sample(self, user, j, probs):
        try:
            p = _np.ctypeslib.as_array(probs, shape=(self.K, self.N)).T  # N x K column-major, no copy
            perm, self.Q = self.st.online(self.Q, p, j)
            self.perms[j - self.burnin] = _np.asarray(perm, dtype=_np.int32)
            return 0
        except Exception as e:
            self.error = e
            return 1

    def ref(self):
        return _C.byref(self.hooks)

    def finish(self, rc, out):
        if self.error is not None:
            raise self.error
        _capi.check(rc)
        z, theta = out["z"], out["theta"]
        zr = _np.empty_like(z)
        thr = _np.empty_like(theta)
        for s in range(self.S):
            pm = self.perms[s]
            zr[s] = pm[z[s] - 1] + 1          # z_out_relabelled(j,i) = perm(z_out(j,i)-1) + 1   (:198)
            thr[pm, :, s] = theta[:, :, s]    # thetas_relab(perm(k), d, j) = theta(k, d, j)     (:216)
        out.update(permutations=self.perms, z=zr, theta=thr, z_original=z, theta_original=theta)
        return out


# ---------------------------------------------------------------- relabel = TRUE, Stephens on the device
STEPHENS_MAX_K = 128  # include/bmm_mcmc.h BMM_STEPHENS_MAX_K


class _RelabelOut(_C.Structure):  # bmm_relabel_out
    _fields_ = [("burnrelabel", _C.c_int), ("permutations", _C.c_void_p), ("z_original", _C.c_void_p),
                ("theta_original", _C.c_void_p)]


def _device_relabel(stephens, relabel, burnin, burnrelabel):
    """stephens="device" with relabel=True: checked before any device is touched.  The reference has no Q
    unless the batch step runs at sweep burnin - 1 over at least one sweep (collapsed_gibbs.cpp:187-190)."""
    if isinstance(stephens, str):
        if stephens != "device":
            raise ValueError('stephens must be "device", None or an object with batch() and online()')
        if not relabel:
            return False
        if burnin < 2 or burnrelabel < 1:
            raise ValueError("relabel on the device needs the batch step: burnin >= 2 and burnrelabel >= 1 "
                             "(burnin = %d, burnrelabel = %d)" % (burnin, burnrelabel))
        return True
    return False


class _DeviceRelabelRun:
    """Outputs of a bmm_*_run_relabel call, laid out as the reference's list (collapsed_gibbs.cpp:232-243)."""

    def __init__(self, N, K, P, S, W):
        self.perms = _np.empty((S, K), dtype=_np.int32, order="F")
        self.z_orig = _np.empty((S, N), dtype=_np.int32, order="F")
        self.th_orig = _np.zeros((K, P, S), order="F")
        self.s = _RelabelOut(int(W), self.perms.ctypes.data, self.z_orig.ctypes.data, self.th_orig.ctypes.data)

    def ref(self):
        return _C.byref(self.s)

    def finish(self, rc, out):
        _capi.check(rc)
        out.update(permutations=self.perms, z=out["z"], theta=out["theta"], z_original=self.z_orig,
                   theta_original=self.th_orig)
        return out


# ---------------------------------------------------------------- what every option of a run is
class _Option:
    """What a run carries for one of its options: arm() hands it to the library just ahead of the call, into(out)
    adds what the run left in it to the result -- under `key`, unless the option says otherwise."""
    key = None

    def into(self, out):
        out[self.key] = self.result()
        return out


_RUN_OPTIONS = ("credible_ball",)
_run_options = _threading.local()


class run_options:
    """Options of the gibbs_* calls made inside the block by this thread, beside their own keywords:

        with bm.run_options(credible_ball={"level": 0.9, "membership_of": rows}):
            out = bm.gibbs_dp(X, 1000, partition="vi", partition_search=True)
        out["partition"]["credible_ball"]

    `credible_ball=True` (level 0.95; needs partition= on the call), a level in (0, 1], or a dict of `level`,
    `membership`, `membership_of`: how sure the clustering estimate is (credible_ball(); include/bmm_mcmc.h "credible
    ball").  After the summary and the search the device measures every kept sweep's distance to
    the estimate -- the searched partition with partition_search=, else the visited sweep -- and `partition` gains
    `credible_ball = {"level", "criterion", "centre" ("search" or "visited"), "radius", "n_in", "n_used", "distance",
    "binder2", "n_clusters", and "horizontal", "upper", "lower": {"sweep" (row of z), "ties", "n_clusters", "distance",
    "z"}}`; with `membership=True` (all rows) or `membership_of=` (rows 0 .. N-1) also "sim", "membership", "sizes",
    "rows": the similarity of rows to the clusters of the estimate, a soft membership that needs no relabelling.
    Everything else is that of the run without it.  Taken by every wrapper that takes partition= (the four gibbs_*
    samplers and gibbs_allocation); at most 64 categories; not with keep_trace=False.  With `chains > 1` it is computed
    once over the pooled traces.  An unknown option is refused by name.  Blocks nest: the inner one wins, and the outer
    options are back when it ends."""

    def __init__(self, **options):
        bad = sorted(set(options) - set(_RUN_OPTIONS))
        if bad:
            raise ValueError("run_options: unknown option %s (known: %s)" % (bad[0], ", ".join(_RUN_OPTIONS)))
        self.options = options

    def __enter__(self):
        self.saved = getattr(_run_options, "now", {})
        _run_options.now = {**self.saved, **self.options}
        return self

    def __exit__(self, *exc):
        _run_options.now = self.saved
        return False


def _run_option(name):
    return getattr(_run_options, "now", {}).get(name)


def _arm(options):
    for o in options:
        if o is not None:
            o.arm()


def _collect(out, options):
    for o in options:
        if o is not None:
            out = o.into(out)
    return out


# ---------------------------------------------------------------- newdata=: the posterior predictive
class _PredictOut(_C.Structure):  # bmm_predict_out
    _fields_ = [("lppd", _C.c_void_p), ("logdens", _C.c_void_p), ("resp", _C.c_void_p), ("relabel", _C.c_void_p),
                ("hooks", _C.c_void_p)]


class _Predict(_Option):
    """Inputs and outputs of a bmm_*_run_predict call: the new rows, lppd (M,), optionally the (S, M) trace of
    log p(x_m | state s) and the (M, Kc) mean responsibilities (include/bmm_mcmc.h)."""
    key = "predictive"

    def __init__(self, newdata, P, S, Kc, trace, responsibilities, chains, newdata_missing=None, burnin=0):
        if int(chains) > 1:
            raise NotImplementedError("newdata= is offered per chain (chains=1)")
        self.cells = None
        self.n_folded = S if int(burnin) > 0 else max(S - 1, 0)  # (row 0 of a run without burn-in is the start, not a sweep)
        if newdata_missing is not None:  # incomplete new rows: the cells, and the matrix without them
            try:
                rows, cols, newdata = _capi.missing_cells(newdata, newdata_missing)
            except ValueError as e:
                raise ValueError(str(e).replace("missing must", "newdata_missing must").replace("N x P", "M x P")) from None
            if rows.size:  # (a set without missing cells takes the complete-row kernels: byte-equal results)
                self.cells = (rows, cols)
                self.cell_mean = _np.full(rows.size, _np.nan)
        self.X = _capi.as_x(newdata)
        if self.X.shape[1] != P:
            raise ValueError("newdata must have the %d columns of data" % P)
        self.M = self.X.shape[0]
        self.lppd = _np.full(self.M, _np.nan)
        self.logdens = _np.full((S, self.M), _np.nan, order="F") if trace else None
        self.resp = _np.full((self.M, Kc), _np.nan, order="F") if responsibilities else None
        self.s = _PredictOut(self.lppd.ctypes.data, self.logdens.ctypes.data if trace else None,
                             self.resp.ctypes.data if responsibilities else None, None, None)

    def arm(self):
        if self.cells is not None:
            rows, cols = self.cells
            _capi.check(_capi.lib().bmm_set_newdata_missing(_capi.vp(rows), _capi.vp(cols), _C.c_int64(rows.size), _capi.vp(self.cell_mean)))

    def result(self):
        out = {"lppd": self.lppd}
        if self.logdens is not None:
            out["logdens"] = self.logdens
        if self.resp is not None:
            out["resp"] = self.resp
        if self.cells is not None:
            rows, cols = self.cells
            out["cells"] = {"rows": rows, "cols": cols, "n_cells": int(rows.size), "mean": self.cell_mean, "n_folded": self.n_folded}
        return out


class _PredictNaPlanOut(_C.Structure):  # bmm_predict_na_plan_out
    _fields_ = [("form", _C.c_int), ("threads", _C.c_int), ("lds_bytes", _C.c_int64), ("table_bytes", _C.c_int64)]


def predict_na_plan(sampler, K, P):
    """Which form of the masked scorer of incomplete new rows a shape takes, without a device (bmm_predict_na_plan,
    DESIGN.md section 28): {"form": "lds" | "global", "lds_bytes", "threads", "table_bytes"}.  K: the labels (maxK for
    gibbs_dp and gibbs_stickbreaking)."""
    o = _PredictNaPlanOut()
    _capi.check(_capi.lib().bmm_predict_na_plan(_C.c_int(_capi.SAMPLER_CODE[sampler]), _C.c_int(int(K)), _C.c_int(int(P)), _C.byref(o)))
    return {"form": "lds" if o.form == 0 else "global", "lds_bytes": int(o.lds_bytes), "threads": int(o.threads),
            "table_bytes": int(o.table_bytes)}


# ---------------------------------------------------------------- loo=: leave-one-out predictive, LPML, WAIC
class _LooOut(_C.Structure):  # bmm_loo_out
    _fields_ = [("log_cpo", _C.c_void_p), ("ess", _C.c_void_p), ("lppd", _C.c_void_p), ("mean", _C.c_void_p),
                ("var", _C.c_void_p), ("lpml", _C.c_void_p), ("min_ess", _C.c_void_p), ("p_waic", _C.c_void_p),
                ("elpd_waic", _C.c_void_p), ("n_folded", _C.c_void_p), ("ell", _C.c_void_p)]


class _Loo(_Option):
    """Outputs of the leave-one-out summary (include/bmm_mcmc.h): per fitted row log_cpo, ess,
    lppd, mean and var of ell over the folded states; lpml, min_ess, n_folded; p_waic and elpd_waic for the samplers
    that carry explicit parameters; optionally the (S, N) trace ell."""
    key = "loo"

    def __init__(self, N, S=0, trace=False, waic=False):
        self.waic = waic
        self.rows = {k: _np.full(N, _np.nan) for k in ("log_cpo", "ess", "lppd", "mean", "var")}
        self.scal = (_C.c_double * 4)(*([float("nan")] * 4))
        self.n = _C.c_int(0)
        self.ell = _np.full((S, N), _np.nan, order="F") if trace else None
        a = _C.addressof(self.scal)
        self.s = _LooOut(*[self.rows[k].ctypes.data for k in ("log_cpo", "ess", "lppd", "mean", "var")],
                         a, a + 8, a + 16, a + 24, _C.addressof(self.n), self.ell.ctypes.data if trace else None)

    def arm(self):
        _capi.check(_capi.lib().bmm_set_loo_summary(_C.byref(self.s)))

    def result(self):
        out = dict(self.rows)
        out.update(lpml=self.scal[0], min_ess=self.scal[1], n_folded=self.n.value)
        if self.waic:
            out.update(p_waic=self.scal[2], elpd_waic=self.scal[3])
        if self.ell is not None:
            out["ell"] = self.ell
        return out


def _make_loo(loo, N, S, chains, waic):
    """loo= of a wrapper, checked before any device is touched"""
    if loo is None or loo is False:
        return None
    if loo is not True and loo != "trace":
        raise ValueError('loo must be True, "trace" or False')
    if int(chains) > 1:
        raise ValueError("loo= is offered per chain (chains=1): pooling the leave-one-out summary over chains is not offered")
    return _Loo(N, S, loo == "trace", waic)


# ---------------------------------------------------------------- partition=: point estimate and similarity
PARTITION_MAX_K = 1024  # include/bmm_mcmc.h BMM_PARTITION_MAX_K
_CRITERION = {"binder": 0, "vi": 1}


class _PartitionOut(_C.Structure):  # bmm_partition_out
    _fields_ = [("criterion", _C.c_int), ("stride", _C.c_int), ("loss", _C.c_void_p), ("binder2", _C.c_void_p),
                ("best", _C.c_void_p), ("z_best", _C.c_void_p), ("n_used", _C.c_void_p), ("dist", _C.c_void_p),
                ("psm_idx", _C.c_void_p), ("psm_M", _C.c_int64), ("psm_cnt", _C.c_void_p)]


def _criterion(criterion):
    if criterion not in _CRITERION:
        raise ValueError('partition criterion must be "binder" or "vi"')
    return _CRITERION[criterion]


def _stride(stride):
    stride = int(stride)
    if stride < 1:
        raise ValueError("partition stride must be >= 1")
    return stride


def _indices(idx, N):
    idx = _np.ascontiguousarray(idx, dtype=_np.int64).ravel()
    if idx.size < 1 or idx.min() < 0 or idx.max() >= N:
        raise ValueError("similarity indices must be observations 0 .. N-1, at least one")
    return idx


class _Partition(_Option):
    """Outputs of an armed bmm_set_partition_summary: the run fills them after its last sweep (include/bmm_mcmc.h,
    DESIGN.md section 13).  With several chains nothing is armed: the traces are pooled afterwards."""
    key = "partition"

    def __init__(self, criterion, stride, similarity_of, N, S):
        self.criterion, self.stride = criterion, _stride(stride)
        code = _criterion(criterion)
        C = -(-S // self.stride)
        self.loss = _np.full(C, _np.nan)
        self.binder2 = _np.zeros(C, dtype=_np.uint64)
        self.best = _C.c_int(-1)
        self.n_used = _C.c_int(0)
        self.z = _np.zeros(N, dtype=_np.int32)
        self.idx = None if similarity_of is None else _indices(similarity_of, N)
        self.cnt = None if self.idx is None else _np.zeros((self.idx.size, self.idx.size), dtype=_np.uint32)
        self.s = _PartitionOut(code, self.stride, self.loss.ctypes.data, self.binder2.ctypes.data,
                               _C.addressof(self.best), self.z.ctypes.data, _C.addressof(self.n_used),
                               None,
                               None if self.idx is None else self.idx.ctypes.data,
                               0 if self.idx is None else self.idx.size,
                               None if self.cnt is None else self.cnt.ctypes.data)

    def arm(self):
        _capi.check(_capi.lib().bmm_set_partition_summary(_C.byref(self.s)))

    def result(self):
        nu = self.n_used.value
        C = -(-nu // self.stride)
        out = {"criterion": self.criterion, "loss": self.loss[:C], "binder2": self.binder2[:C],
               "best": self.best.value, "z": self.z, "n_used": nu}
        if self.cnt is not None:
            out["similarity"] = self.cnt
        return out


def _make_partition(partition, stride, similarity_of, N, S, chains):
    """partition=, partition_stride=, similarity_of= of a wrapper, checked before any device is touched.  One chain:
    the outputs to arm for the run; several: None (the traces are pooled afterwards, _pooled)."""
    if partition is None:
        if similarity_of is not None:
            raise ValueError('similarity_of= needs partition="binder" or "vi"')
        return None
    if int(chains) > 1:
        _criterion(partition), _stride(stride)
        if similarity_of is not None:
            _indices(similarity_of, N)
        return None
    return _Partition(partition, stride, similarity_of, N, S)


def _pooled(chains_out, partition, stride, similarity_of, device):
    """chains > 1: the chains' traces stacked (rows that are no partition -- the unassigned starting state of a run
    without burn-in -- left out), one stand-alone call, the pooled summary attached to every chain object."""
    if partition is None:
        return chains_out
    rows, src = [], []
    for ci, o in enumerate(chains_out):
        z = o["z"]
        keep = [s for s in range(z.shape[0]) if z[s].min() >= 1]
        rows.append(z[keep])
        src += [(ci, s) for s in keep]
    zz = _np.asfortranarray(_np.concatenate(rows, axis=0))
    res = partition_distances(zz, partition, stride, device=device)
    res["chain"], res["best"] = src[res["best"]]
    if similarity_of is not None:
        res["similarity"] = posterior_similarity(zz, similarity_of, device=device)
    for o in chains_out:
        o["partition"] = res
    return chains_out


def _as_trace(z):
    z = _np.asfortranarray(z, dtype=_np.int32)
    if z.ndim != 2 or z.shape[0] < 1 or z.shape[1] < 1:
        raise ValueError("z must be an S x N matrix of labels (rows: kept sweeps), S, N >= 1")
    return z


def partition_distances(z, criterion="binder", stride=1, distances=False, device=0, Kc=None):
    """Point estimate of the clustering from a label trace, on the device (include/bmm_mcmc.h).
    z: S x N labels, 1-based, as a run returns them -- or the traces of several chains stacked.  Candidates are rows
    0, stride, ...; the draws are all rows.  Returns {"criterion", "loss" (C,), "binder2" (C,) uint64 exact totals
    sum_t 2 B(c, z_t), "best" (row of z, 0-based, smallest expected loss, lowest index on ties), "z" (that row),
    "n_used" (S)} and, with distances=True, "distances" (C, S): Binder (exact integers held in doubles) or VI in nats.
    Kc: number of categories (default: the largest label)."""
    z = _as_trace(z)
    S, N = z.shape
    code, stride = _criterion(criterion), _stride(stride)
    Kc = max(1, int(z.max())) if Kc is None else int(Kc)
    C = -(-S // stride)
    loss = _np.zeros(C)
    b2 = _np.zeros(C, dtype=_np.uint64)
    best = _C.c_int(-1)
    dist = _np.zeros((C, S), order="F") if distances else None
    _capi.check(_capi.lib().bmm_device_partition_distances(
        _C.c_int(device), _capi.vp(z), _C.c_int(S), _C.c_int64(N), _C.c_int(Kc), _C.c_int(code), _C.c_int(stride),
        _capi.vp(loss), _capi.vp(b2), _C.byref(best), _capi.vp(dist) if distances else None))
    out = {"criterion": criterion, "loss": loss, "binder2": b2, "best": best.value, "z": z[best.value].copy(), "n_used": S}
    if distances:
        out["distances"] = dist
    return out


def posterior_similarity(z, idx, device=0):
    """cnt[u, v] = number of rows of z (S x N, labels >= 1) in which observations idx[u] and idx[v] (0-based, any
    order, repeats allowed) share a cluster: (M, M) uint32, symmetric, diagonal S.  Computed on the device."""
    z = _as_trace(z)
    S, N = z.shape
    idx = _indices(idx, N)
    cnt = _np.zeros((idx.size, idx.size), dtype=_np.uint32)
    _capi.check(_capi.lib().bmm_device_psm(_C.c_int(device), _capi.vp(z), _C.c_int(S), _C.c_int64(N), _capi.vp(idx),
                                           _C.c_int64(idx.size), _capi.vp(cnt)))
    return cnt


_PT_PLAN_FIELDS = ("label_bytes", "lds", "draws_per_workgroup", "replicas", "draw_blocks", "workgroups", "threads",
                   "lds_bytes", "triangular", "vi", "generic_bytes", "pitch")


def partition_plan(S, N, Kc, candidates=None, criterion="binder"):
    """Which form of the partition kernels a shape runs (S rows, N observations, Kc categories, `candidates` of the
    rows -- default all), read from the library's launch arithmetic without touching a device
    (bmm_device_partition_plan): a dict of the fields include/bmm_mcmc.h lists."""
    out = (_C.c_int64 * 12)()
    C = int(S) if candidates is None else int(candidates)
    _capi.check(_capi.lib().bmm_device_partition_plan(_C.c_int(int(S)), _C.c_int64(int(N)), _C.c_int(int(Kc)),
                                                      _C.c_int(C), _C.c_int(_criterion(criterion)), out))
    return dict(zip(_PT_PLAN_FIELDS, (int(v) for v in out)))


# ---------------------------------------------------------------- partition_search=: greedy search for the estimate
PARTITION_SEARCH_MAX_K = 64  # include/bmm_mcmc.h BMM_PARTITION_SEARCH_MAX_K
_PS_KEYS = ("batch", "min_batch", "max_passes", "max_clusters")


class _SearchOpts(_C.Structure):  # bmm_partition_search_opts
    _fields_ = [("batch", _C.c_int64), ("min_batch", _C.c_int64), ("max_passes", _C.c_int), ("max_clusters", _C.c_int)]


class _SearchOut(_C.Structure):  # bmm_partition_search_out
    _fields_ = [(k, _C.c_void_p) for k in ("z_hat", "binder2", "loss", "start_loss", "start_binder2", "passes", "pass_batch",
                                           "pass_moved", "pass_binder2", "pass_total", "converged", "n_clusters")]


def _search_opts(N, Kc, batch=None, min_batch=None, max_passes=50, max_clusters=None):
    """the options of a search with the defaults filled in: batch ceil(N / 8), min_batch ceil(N / 256), Ka = Kc"""
    batch = -(-N // 8) if batch is None else int(batch)
    min_batch = -(-N // 256) if min_batch is None else int(min_batch)
    max_passes = int(max_passes)
    Ka = int(Kc) if max_clusters is None else int(max_clusters)
    if batch < 1 or min_batch < 1:
        raise ValueError("partition_search: batch and min_batch must be >= 1")
    if max_passes < 1:
        raise ValueError("partition_search: max_passes must be >= 1")
    if Ka < 1 or Ka > PARTITION_SEARCH_MAX_K:
        raise ValueError("partition_search: max_clusters must be in 1 .. %d" % PARTITION_SEARCH_MAX_K)
    return _SearchOpts(batch, min_batch, max_passes, Ka)


class _Search(_Option):
    """Outputs of a greedy search (bmm_device_partition_search, or armed with bmm_set_partition_search for a run)."""

    def __init__(self, criterion, N, opts):
        self.criterion, self.opts = criterion, opts
        P = opts.max_passes
        self.z = _np.zeros(N, dtype=_np.int32)
        self.u64 = _np.zeros(2, dtype=_np.uint64)   # binder2, start_binder2
        self.f64 = _np.full(2, _np.nan)             # loss, start_loss
        self.i32 = _np.full(3, -1, dtype=_np.int32)  # passes, converged, n_clusters
        self.pb = _np.zeros(P, dtype=_np.int64)
        self.pm = _np.zeros(P, dtype=_np.int64)
        self.p2 = _np.zeros(P, dtype=_np.uint64)
        self.ptot = _np.full(P, _np.nan)
        self.s = _SearchOut(self.z.ctypes.data, self.u64.ctypes.data, self.f64.ctypes.data, self.f64.ctypes.data + 8,
                            self.u64.ctypes.data + 8, self.i32.ctypes.data, self.pb.ctypes.data, self.pm.ctypes.data,
                            self.p2.ctypes.data, self.ptot.ctypes.data, self.i32.ctypes.data + 4, self.i32.ctypes.data + 8)

    def arm(self):
        _capi.check(_capi.lib().bmm_set_partition_search(_C.byref(self.opts), _C.byref(self.s)))

    def result(self):
        n = int(self.i32[0])
        if n < 0:  # the run had no usable row: nothing was searched
            return None
        total = [int(v) for v in self.p2[:n]] if self.criterion == "binder" else [float(v) for v in self.ptot[:n]]
        return {"z": self.z, "loss": float(self.f64[0]), "binder2": int(self.u64[0]), "start_loss": float(self.f64[1]),
                "start_binder2": int(self.u64[1]), "passes": n, "batch": [int(v) for v in self.pb[:n]],
                "moved": [int(v) for v in self.pm[:n]], "total": total, "converged": bool(self.i32[1]),
                "n_clusters": int(self.i32[2])}

    def into(self, out):
        """the search of a single-chain run beside the summary it started from"""
        res = self.result() if "partition" in out else None
        if res is not None:
            out["partition"]["search"] = res
        return out


def partition_search(z, criterion="binder", start=None, batch=None, min_batch=None, max_passes=50, max_clusters=None,
                     device=0, Kc=None):
    """Greedy search for the clustering point estimate, on the device (include/bmm_mcmc.h "greedy search", DESIGN.md
    section 27).  z: S x N labels, 1-based, as partition_distances takes them.  From `start` (N labels in
    1 .. max_clusters; default: the row of z that partition_distances would choose) single rows are moved to whichever
    cluster lowers the posterior expected Binder or VI loss most, in passes of batches of `batch` rows scored against
    one state of the tables (default ceil(N / 8), halved down to `min_batch`, default ceil(N / 256), whenever a pass
    does not improve), until no row wants to move or `max_passes` passes have run.  `max_clusters`: the slots a row may
    move to, empty ones included (default Kc, at most 64).  Returns {"z" (N,) the searched partition, "loss" its expected
    loss, "binder2" its exact total sum_t 2 B(z, z_t), "start_loss", "start_binder2", "passes", and per pass "batch",
    "moved", "total" (binder2 as Python integers, or the VI total S N x expected VI), "converged" (no single-row move
    lowers the loss), "n_clusters"}.  The result is never worse than the start.  Kc: number of categories of z (default:
    the largest label), at most 64."""
    z = _as_trace(z)
    S, N = z.shape
    code = _criterion(criterion)
    Kc = max(1, int(z.max())) if Kc is None else int(Kc)
    opts = _search_opts(N, Kc, batch, min_batch, max_passes, max_clusters)
    st = None
    if start is not None:
        st = _np.ascontiguousarray(start, dtype=_np.int32)
        if st.shape != (N,):
            raise ValueError("start must have one label per observation")
    so = _Search(criterion, N, opts)
    _capi.check(_capi.lib().bmm_device_partition_search(
        _C.c_int(device), _capi.vp(z), _C.c_int(S), _C.c_int64(N), _C.c_int(Kc), _C.c_int(code),
        _capi.vp(st) if st is not None else None, _C.byref(opts), _C.byref(so.s)))
    return so.result()


_PS_PLAN_FIELDS = ("label_bytes", "slot_stride", "threads_per_row", "rows_per_workgroup", "draws_per_block", "draw_blocks",
                   "block_bound", "lds_bytes", "workgroups", "batches", "vi", "table_bytes")


def partition_search_plan(S, N, Kc, max_clusters=None, criterion="binder", batch=None):
    """Which form of the search kernels a shape runs, read from the library's launch arithmetic without touching a
    device (bmm_partition_search_plan): a dict of the fields include/bmm_mcmc.h lists; "block_bound" is 0 when a block
    of draws holds all S, 1 when the LDS budget bounds it, 2 when the 32-bit sums of a block do."""
    out = (_C.c_int64 * 12)()
    N = int(N)
    Ka = int(Kc) if max_clusters is None else int(max_clusters)
    batch = -(-N // 8) if batch is None else int(batch)
    L = _capi.lib()
    L.bmm_partition_search_plan.argtypes = [_C.c_int, _C.c_int64, _C.c_int, _C.c_int, _C.c_int, _C.c_int64, _C.c_void_p]
    _capi.check(L.bmm_partition_search_plan(int(S), N, int(Kc), Ka, _criterion(criterion), batch, out))
    return dict(zip(_PS_PLAN_FIELDS, (int(v) for v in out)))


def _make_search(partition_search, partition, N, K, chains):
    """partition_search= of a wrapper, checked before any device is touched: True or a dict of batch, min_batch,
    max_passes, max_clusters.  One chain: the outputs to arm; several: the options (searched after pooling)."""
    if partition_search is None or partition_search is False:
        return None
    if partition is None:
        raise ValueError('partition_search= needs partition="binder" or "vi"')
    kw = {} if partition_search is True else dict(partition_search)
    bad = sorted(set(kw) - set(_PS_KEYS))
    if bad:
        raise ValueError("partition_search: unknown option %s (known: %s)" % (bad[0], ", ".join(_PS_KEYS)))
    if K > PARTITION_SEARCH_MAX_K:
        raise ValueError("partition_search= takes at most %d categories (got %d)" % (PARTITION_SEARCH_MAX_K, K))
    opts = _search_opts(N, K, **kw)
    if opts.max_clusters < K:
        raise ValueError("partition_search: max_clusters must be at least the %d labels of the run" % K)
    return kw if int(chains) > 1 else _Search(partition, N, opts)


def _pooled_search(chains_out, kw, partition, K, device):
    """chains > 1: the search over the stacked traces _pooled used, from the pooled estimate, through the stand-alone call"""
    if kw is None:
        return chains_out
    rows = []
    for o in chains_out:
        z = o["z"]
        rows.append(z[[s for s in range(z.shape[0]) if z[s].min() >= 1]])
    zz = _np.asfortranarray(_np.concatenate(rows, axis=0))
    res = partition_search(zz, partition, start=chains_out[0]["partition"]["z"], device=device, Kc=K, **kw)
    chains_out[0]["partition"]["search"] = res  # (one dict shared by every chain object)
    return chains_out


# ---------------------------------------------------------------- credible_ball=: how sure the point estimate is
_CB_KEYS = ("level", "membership", "membership_of")
_CB_BOUNDS = ("horizontal", "upper", "lower")


class _BallBound(_C.Structure):  # bmm_credible_bound
    _fields_ = [(k, _C.c_void_p) for k in ("sweep", "ties", "n_clusters", "dist", "d2", "z")]


class _BallOut(_C.Structure):  # bmm_credible_ball_out
    _fields_ = [("d2", _C.c_void_p), ("dist", _C.c_void_p), ("n_clusters", _C.c_void_p), ("radius", _C.c_void_p),
                ("radius2", _C.c_void_p), ("n_in", _C.c_void_p), ("horizontal", _BallBound), ("upper", _BallBound),
                ("lower", _BallBound), ("sim", _C.c_void_p), ("member_idx", _C.c_void_p), ("member_M", _C.c_int64),
                ("sizes", _C.c_void_p)]


def _ball_opts(credible_ball, N):
    """credible_ball= as (level, membership, membership_of): True, a level, or a dict of the three"""
    if credible_ball is True:
        kw = {}
    elif isinstance(credible_ball, dict):
        kw = dict(credible_ball)
    else:
        kw = {"level": credible_ball}
    bad = sorted(set(kw) - set(_CB_KEYS))
    if bad:
        raise ValueError("credible_ball: unknown option %s (known: %s)" % (bad[0], ", ".join(_CB_KEYS)))
    return _ball_level(kw.get("level", 0.95)), bool(kw.get("membership", False)), _ball_rows(kw.get("membership_of"), N)


def _ball_level(level):
    level = float(level)
    if not 0.0 < level <= 1.0:
        raise ValueError("credible_ball: level must be in (0, 1]")
    return level


def _ball_rows(membership_of, N):
    if membership_of is None:
        return None
    idx = _np.ascontiguousarray(membership_of, dtype=_np.int64).ravel()
    if idx.size < 1 or idx.min() < 0 or idx.max() >= N:
        raise ValueError("credible_ball: membership_of must be observations 0 .. N-1, at least one")
    return idx


class _Ball(_Option):
    """Outputs of a credible ball (bmm_device_credible_ball, or armed with bmm_set_credible_ball for a run): S draws
    at most, N observations, Ka slots of the centre."""

    def __init__(self, criterion, level, S, N, Ka, membership=False, rows=None, centre="visited"):
        self.criterion, self.level, self.centre, self.S = criterion, level, centre, S
        self.d2 = _np.zeros(S, dtype=_np.uint64)
        self.dist = _np.full(S, _np.nan)
        self.k = _np.zeros(S, dtype=_np.int32)
        self.f64 = _np.full(4, _np.nan)               # radius, and the distance of the three bounds
        self.u64 = _np.zeros(4, dtype=_np.uint64)     # radius2, and d2 of the three bounds
        self.i32 = _np.full(10, -1, dtype=_np.int32)  # n_in, then sweep, ties, n_clusters of each bound
        self.zb = _np.zeros((3, N), dtype=_np.int32)
        self.sizes = _np.zeros(Ka, dtype=_np.int64)
        self.rows = rows
        self.sim = None
        if membership or rows is not None:
            self.sim = _np.zeros((N if rows is None else rows.size, Ka), dtype=_np.uint64)
        bounds = [_BallBound(self.i32.ctypes.data + 4 * (1 + 3 * q), self.i32.ctypes.data + 4 * (2 + 3 * q),
                             self.i32.ctypes.data + 4 * (3 + 3 * q), self.f64.ctypes.data + 8 * (1 + q),
                             self.u64.ctypes.data + 8 * (1 + q), self.zb[q].ctypes.data) for q in range(3)]
        self.s = _BallOut(self.d2.ctypes.data, self.dist.ctypes.data, self.k.ctypes.data, self.f64.ctypes.data,
                          self.u64.ctypes.data, self.i32.ctypes.data, bounds[0], bounds[1], bounds[2],
                          None if self.sim is None else self.sim.ctypes.data,
                          None if rows is None else rows.ctypes.data, 0 if rows is None else rows.size,
                          self.sizes.ctypes.data)

    def arm(self):
        _capi.check(_capi.lib().bmm_set_credible_ball(_C.c_double(self.level), _C.byref(self.s)))

    def result(self, n_used=None):
        if int(self.i32[0]) < 0:  # the run had no usable row: there is no ball
            return None
        nu = self.S if n_used is None else int(n_used)
        out = {"level": self.level, "criterion": self.criterion, "centre": self.centre, "radius": float(self.f64[0]),
               "n_in": int(self.i32[0]), "n_used": nu, "distance": self.dist[:nu],
               "binder2": _np.array([int(v) for v in self.d2[:nu]], dtype=object), "n_clusters": self.k[:nu]}
        for q, name in enumerate(_CB_BOUNDS):
            out[name] = {"sweep": int(self.i32[1 + 3 * q]), "ties": int(self.i32[2 + 3 * q]),
                         "n_clusters": int(self.i32[3 + 3 * q]), "distance": float(self.f64[1 + q]), "z": self.zb[q]}
        if self.sim is not None:
            out.update(_membership(self.sim, self.sizes, self.rows, nu, self._centre_labels))
        return out

    _centre_labels = None

    def into(self, out):
        """the ball of a single-chain run beside the summary, around the searched partition where there is one"""
        pt = out.get("partition")
        if pt is None:
            return out
        self._centre_labels = pt["search"]["z"] if "search" in pt else pt["z"]
        res = self.result(pt["n_used"])
        if res is not None:
            pt["credible_ball"] = res
        return out


def _membership(sim, sizes, rows, S, centre):
    """membership[u, a] = (sim[u, a] - S own) / (S (n_a - own)), own = [a = c_u]: NaN for an empty slot and for a row
    alone in its cluster"""
    rows = _np.arange(sim.shape[0], dtype=_np.int64) if rows is None else rows
    own = _np.zeros(sim.shape, dtype=_np.int64)
    own[_np.arange(rows.size), _np.asarray(centre, dtype=_np.int64)[rows] - 1] = 1
    den = (float(S) * (sizes[None, :] - own)).astype(_np.float64)
    num = sim.astype(_np.int64) - S * own
    with _np.errstate(divide="ignore", invalid="ignore"):
        mem = _np.where(den > 0, num / _np.where(den > 0, den, 1.0), _np.nan)
    return {"sim": sim, "membership": mem, "sizes": sizes, "rows": rows}


def credible_ball(z, centre, criterion="vi", level=0.95, membership=False, membership_of=None, device=0, Kc=None,
                  max_clusters=None):
    """Credible ball of Wade & Ghahramani (2018) around the partition `centre`, and the similarity of rows to its
    clusters, on the device (include/bmm_mcmc.h "credible ball").  z: S x N labels, 1-based, as
    partition_distances takes them; centre: N labels in 1 .. max_clusters (default: the larger of Kc and the largest
    label of centre, at most 64), e.g. partition["z"] or partition["search"]["z"].  The draws are ordered by their Binder
    or VI distance to the centre; the radius is the distance of draw ceil(level S) in that order, ties at the radius are
    all inside.  Returns {"level", "criterion", "centre" ("given"), "radius", "n_in", "n_used" (S), "distance" (S,): B
    or VI in nats per draw, "binder2" (S,): 2 B as Python integers under either criterion, "n_clusters" (S,): non-empty
    clusters per draw, "horizontal", "upper", "lower": {"sweep", "ties", "n_clusters", "distance", "z"}} -- the draw
    of the ball farthest from the centre, and the farthest among those with the fewest and with the most clusters, the
    lowest row on ties and how many tie.  `membership=True` (all rows) or `membership_of=` (rows 0 .. N-1, any order,
    repeats allowed) adds "sim" (M, Ka) uint64: how often the row sat with each member of each cluster of the centre,
    summed over draws and members (the row itself included S times in its own cluster), "membership" (M, Ka): the mean
    posterior similarity of the row to the other members of each cluster (NaN for an empty cluster and for a row alone
    in its own) -- a soft membership that needs no relabelling and works for gibbs_dp --, "sizes" (Ka,) and "rows".
    Kc: number of categories of z (default: the largest label), at most 64."""
    z = _as_trace(z)
    S, N = z.shape
    code = _criterion(criterion)
    level = _ball_level(level)
    rows = _ball_rows(membership_of, N)
    c = _np.ascontiguousarray(centre, dtype=_np.int32)
    if c.shape != (N,):
        raise ValueError("centre must have one label per observation")
    Kc = max(1, int(z.max())) if Kc is None else int(Kc)
    Ka = max(Kc, int(c.max())) if max_clusters is None else int(max_clusters)
    if Ka < 1 or Ka > PARTITION_SEARCH_MAX_K:
        raise ValueError("credible_ball: max_clusters must be in 1 .. %d" % PARTITION_SEARCH_MAX_K)
    b = _Ball(criterion, level, S, N, Ka, membership, rows, centre="given")
    _capi.check(_capi.lib().bmm_device_credible_ball(
        _C.c_int(device), _capi.vp(z), _C.c_int(S), _C.c_int64(N), _C.c_int(Kc), _C.c_int(code), _capi.vp(c),
        _C.c_int(Ka), _C.c_double(level), _C.byref(b.s)))
    b._centre_labels = c
    return b.result()


_CB_PLAN_FIELDS = ("label_bytes", "slot_stride", "threads_per_row", "rows_per_workgroup", "draws_per_block", "draw_blocks",
                   "block_bound", "lds_bytes", "workgroups", "gathered", "vi", "table_bytes")


def credible_ball_plan(S, N, Kc, max_clusters=None, criterion="vi", rows=None):
    """Which form of the credible-ball kernels a shape runs, read from the library's launch arithmetic without touching
    a device (bmm_credible_ball_plan): a dict of the fields include/bmm_mcmc.h lists.  `rows`: how many rows the
    similarity is asked for (default all N, read from the label block; fewer are gathered first); "block_bound" as
    partition_search_plan."""
    out = (_C.c_int64 * 12)()
    N = int(N)
    Ka = int(Kc) if max_clusters is None else int(max_clusters)
    M = N if rows is None else int(rows)
    _capi.check(_capi.lib().bmm_credible_ball_plan(_C.c_int(int(S)), _C.c_int64(N), _C.c_int(int(Kc)), _C.c_int(Ka),
                                                   _C.c_int(_criterion(criterion)), _C.c_int64(M), out))
    return dict(zip(_CB_PLAN_FIELDS, (int(v) for v in out)))


def _make_ball(credible_ball, partition, search, keep_trace, N, S, K, chains):
    """credible_ball= of run_options for a wrapper, checked before any device is touched: True (level 0.95), a level, or a dict of
    level, membership, membership_of.  One chain: the outputs to arm; several: the options (pooled afterwards)."""
    if credible_ball is None or credible_ball is False:
        return None
    if partition is None:
        raise ValueError('credible_ball= needs partition="binder" or "vi"')
    if not keep_trace:
        raise ValueError("keep_trace=False drops the label trace, which credible_ball= reads")
    level, membership, rows = _ball_opts(credible_ball, N)
    if K > PARTITION_SEARCH_MAX_K:
        raise ValueError("credible_ball= takes at most %d categories (got %d)" % (PARTITION_SEARCH_MAX_K, K))
    if int(chains) > 1:
        return {"level": level, "membership": membership, "membership_of": rows}
    Ka = K if search is None else search.opts.max_clusters
    return _Ball(partition, level, S, N, Ka, membership, rows, centre="visited" if search is None else "search")


def _pooled_ball(chains_out, kw, ps_kw, partition, K, device):
    """chains > 1: the ball over the stacked traces _pooled used, around the pooled centre, through the stand-alone call"""
    if kw is None:
        return chains_out
    rows = []
    for o in chains_out:
        z = o["z"]
        rows.append(z[[s for s in range(z.shape[0]) if z[s].min() >= 1]])
    zz = _np.asfortranarray(_np.concatenate(rows, axis=0))
    pt = chains_out[0]["partition"]
    searched = "search" in pt
    Ka = _search_opts(zz.shape[1], K, **ps_kw).max_clusters if searched else K
    res = credible_ball(zz, pt["search"]["z"] if searched else pt["z"], partition, device=device, Kc=K, max_clusters=Ka, **kw)
    res["centre"] = "search" if searched else "visited"
    pt["credible_ball"] = res  # (one dict shared by every chain object)
    return chains_out


# ---------------------------------------------------------------- relabel="ecr": relabelling from the label trace alone
ECR_MAX_K = 128  # include/bmm_mcmc.h BMM_ECR_MAX_K
_ECR_GIVEN, _ECR_PARTITION, _ECR_ITERATIVE = 0, 1, 2
_ECR_MAP = 3  # ecr_pivot="map": the best state of logpost=, relabelled to after the run (not a kind of the library's)


class _EcrOut(_C.Structure):  # bmm_ecr_out
    _fields_ = [("pivot_kind", _C.c_int), ("pivot", _C.c_void_p), ("max_iter", _C.c_int), ("permutations", _C.c_void_p),
                ("z_original", _C.c_void_p), ("theta_original", _C.c_void_p), ("agree", _C.c_void_p),
                ("pivot_out", _C.c_void_p), ("iterations", _C.c_void_p), ("converged", _C.c_void_p),
                ("n_used", _C.c_void_p)]


def _permute_theta(theta, perms):
    """theta_relab[perm[s, k], :, s] = theta[k, :, s]"""
    out = _np.empty_like(theta)
    for s in range(perms.shape[0]):
        out[perms[s], :, s] = theta[:, :, s]
    return out


def _ecr_pivot(ecr_pivot, N, partition):
    """ecr_pivot= of a wrapper, checked before any device is touched: (kind, labels or None)."""
    if isinstance(ecr_pivot, str):
        if ecr_pivot == "iterative":
            return _ECR_ITERATIVE, None
        if ecr_pivot == "map":
            return _ECR_MAP, None
        if ecr_pivot == "partition":
            if partition is None:
                raise ValueError('ecr_pivot="partition" needs partition="binder" or "vi"')
            return _ECR_PARTITION, None
        raise ValueError('ecr_pivot must be "iterative", "partition", "map" or N labels')
    pv = _np.ascontiguousarray(ecr_pivot, dtype=_np.int32).ravel()
    if pv.shape != (N,):
        raise ValueError("ecr_pivot must have one label per observation")
    return _ECR_GIVEN, pv


def _ecr_request(relabel, stephens, ecr_pivot, ecr_max_iter, N, partition):
    """relabel= of a wrapper: (relabel as the rest of the wrapper reads it, None or the checked ECR request)."""
    if not (isinstance(relabel, str) and relabel == "ecr"):
        return relabel, None
    if stephens is not None:
        raise ValueError('relabel="ecr" relabels from the label trace alone: not together with stephens= (two relabellings)')
    kind, pv = _ecr_pivot(ecr_pivot, N, partition)
    return False, (kind, pv, int(ecr_max_iter))


class _Ecr(_Option):
    """Outputs of an armed bmm_set_ecr_relabel: the run fills them after its last sweep (include/bmm_mcmc.h "ECR",
    DESIGN.md section 19).  With several chains nothing is armed: the traces are stacked afterwards (_ecr_chains)."""

    def __init__(self, req, N, K, P, S):
        kind, self.given, max_iter = req
        self.perms = _np.empty((S, K), dtype=_np.int32, order="F")
        self.z_orig = _np.empty((S, N), dtype=_np.int32, order="F")
        self.th_orig = _np.zeros((K, P, S), order="F")
        self.agree = _np.zeros(S, dtype=_np.int64)
        self.pivot = _np.zeros(N, dtype=_np.int32)
        self.iterations, self.converged, self.n_used = _C.c_int(0), _C.c_int(0), _C.c_int(0)
        self.s = _EcrOut(kind, None if self.given is None else self.given.ctypes.data, max_iter, self.perms.ctypes.data,
                         self.z_orig.ctypes.data, self.th_orig.ctypes.data, self.agree.ctypes.data,
                         self.pivot.ctypes.data, _C.addressof(self.iterations), _C.addressof(self.converged),
                         _C.addressof(self.n_used))

    def arm(self):
        _capi.check(_capi.lib().bmm_set_ecr_relabel(_C.byref(self.s)))

    def into(self, out):
        out.update(permutations=self.perms, z_original=self.z_orig, theta_original=self.th_orig,
                   ecr={"agree": self.agree, "pivot": self.pivot, "iterations": self.iterations.value,
                        "converged": bool(self.converged.value), "n_used": self.n_used.value})
        return out


def ecr_relabel(z, K, pivot=None, max_iter=50, theta=None, device=0, tables=False):
    """ECR relabelling of a label trace on the device (include/bmm_mcmc.h "ECR").  z: S x N
    labels in 1..K, as a run returns them -- or the traces of several chains stacked.  pivot: N labels in 1..K, every
    row is then permuted to agree with it on as many observations as possible; None: the iterative form, the pivot
    is the majority vote of the rows as relabelled so far, until the total agreement stops growing (at most max_iter
    iterations).  Returns {"permutations" (S, K) int32, 0-based: label l of row t becomes permutations[t, l]; "z" the
    relabelled trace; "agree" (S,) int64: observations on which a relabelled row agrees with the pivot; "pivot" (N,);
    "iterations"; "converged"} and, given theta (K, P, S), "theta" permuted alike; with tables=True "tables" (S, K, K)
    uint32: tables[t, a, b] = #{i : z[t, i] = a + 1, pivot[i] = b + 1} of the last iteration."""
    z = _as_trace(z)
    S, N = z.shape
    K = int(K)
    pv = None if pivot is None else _ecr_pivot(pivot, N, None)[1]
    perms = _np.zeros((S, max(K, 1)), dtype=_np.int32, order="F")
    agree = _np.zeros(S, dtype=_np.int64)
    pivot_out = _np.zeros(N, dtype=_np.int32)
    zr = _np.empty((S, N), dtype=_np.int32, order="F")
    tabs = _np.zeros((S, max(K, 1), max(K, 1)), dtype=_np.uint32) if tables else None
    it, conv = _C.c_int(0), _C.c_int(0)
    _capi.check(_capi.lib().bmm_device_ecr(
        _C.c_int(device), _capi.vp(z), _C.c_int(S), _C.c_int64(N), _C.c_int(K), None if pv is None else _capi.vp(pv),
        _C.c_int(int(max_iter)), _capi.vp(perms), _capi.vp(agree), _capi.vp(pivot_out), _capi.vp(zr),
        _capi.vp(tabs) if tables else None, _C.byref(it), _C.byref(conv)))
    out = {"permutations": perms, "z": zr, "agree": agree, "pivot": pivot_out, "iterations": it.value,
           "converged": bool(conv.value)}
    if theta is not None:
        theta = _np.asarray(theta)
        if theta.ndim != 3 or theta.shape[0] != K or theta.shape[2] != S:
            raise ValueError("theta must be K x P x S")
        out["theta"] = _permute_theta(theta, perms)
    if tables:
        out["tables"] = tabs
    return out


_ECR_PLAN_FIELDS = ("label_bytes", "tables_lds", "rows_per_workgroup", "copies", "row_blocks", "slices", "span",
                    "tables_lds_bytes", "votes_lds", "votes_workgroups", "votes_bytes", "pitch")


def ecr_plan(S, N, K):
    """Which form of the ECR kernels a shape runs (S rows, N observations, K categories), read from the library's launch
    arithmetic without touching a device (bmm_device_ecr_plan): a dict of the fields include/bmm_mcmc.h lists."""
    out = (_C.c_int64 * 12)()
    _capi.check(_capi.lib().bmm_device_ecr_plan(_C.c_int(int(S)), _C.c_int64(int(N)), _C.c_int(int(K)), out))
    return dict(zip(_ECR_PLAN_FIELDS, (int(v) for v in out)))


def _ecr_chains(chains_out, req, K, device):
    """chains > 1: the chains' traces stacked (rows that are no partition left out, as _pooled leaves them out), one
    stand-alone call against one pivot -- for "partition" the pooled estimate -- and every chain object receives its
    rows of the result, theta permuted on the host."""
    if req is None:
        return chains_out
    kind, pv, max_iter = req
    if kind == _ECR_PARTITION:
        pv = _np.ascontiguousarray(chains_out[0]["partition"]["z"], dtype=_np.int32)
    src = [[s for s in range(o["z"].shape[0]) if o["z"][s].min() >= 1] for o in chains_out]
    res = ecr_relabel(_np.concatenate([o["z"][keep] for o, keep in zip(chains_out, src)], axis=0), K, pv, max_iter,
                      device=device)
    at = 0
    for o, keep in zip(chains_out, src):
        S = o["z"].shape[0]
        perms = _np.asfortranarray(_np.tile(_np.arange(K, dtype=_np.int32), (S, 1)))
        agree = _np.zeros(S, dtype=_np.int64)
        zr = o["z"].copy(order="F")
        perms[keep] = res["permutations"][at:at + len(keep)]
        agree[keep] = res["agree"][at:at + len(keep)]
        zr[keep] = res["z"][at:at + len(keep)]
        at += len(keep)
        o.update(permutations=perms, z_original=o["z"], theta_original=o["theta"], z=zr,
                 theta=_permute_theta(o["theta"], perms),
                 ecr={"agree": agree, "pivot": res["pivot"], "iterations": res["iterations"],
                      "converged": res["converged"], "n_used": sum(len(k) for k in src)})  # rows of all chains
    return chains_out


# ---------------------------------------------------------------- logpost=: log joint trace, MAP allocation, ESS, R-hat
_LP_KEYS = ("log_lik", "log_prior", "log_hyper", "log_joint")


def ess(x):
    """Effective sample size of a scalar trace (NumPy, on the host): n / tau with tau from Geyer's initial monotone
    positive sequence over FFT autocovariances.  NaN for a constant series, a series with a non-finite value, or fewer
    than 4 values per half (n < 8)."""
    x = _np.asarray(x, dtype=_np.float64).ravel()
    n = x.size
    if n < 8 or not _np.all(_np.isfinite(x)):
        return float("nan")
    xc = x - x.mean()
    if not _np.any(xc != 0.0):
        return float("nan")
    nfft = 1 << int(2 * n - 1).bit_length()
    f = _np.fft.rfft(xc, nfft)
    acov = _np.fft.irfft(f * _np.conj(f), nfft)[:n] / n
    if not acov[0] > 0.0:
        return float("nan")
    rho = acov / acov[0]
    m = n // 2
    pairs = rho[0:2 * m:2] + rho[1:2 * m:2]  # Gamma_m = rho_2m + rho_2m+1
    neg = _np.nonzero(pairs <= 0.0)[0]
    if neg.size:
        pairs = pairs[:neg[0]]
    if pairs.size == 0:
        return float(n)
    pairs = _np.minimum.accumulate(pairs)  # monotone
    tau = -1.0 + 2.0 * pairs.sum()
    return float(n / tau) if tau > 0.0 else float("nan")


def rhat(chains):
    """Split-R-hat (Gelman et al., BDA3) of a scalar over several chains (NumPy, on the host): every chain is cut to
    the length of the shortest (its tail is kept) and split in two halves.  NaN for a constant series, a non-finite
    value, or fewer than 4 values per half."""
    xs = [_np.asarray(c, dtype=_np.float64).ravel() for c in chains]
    if not xs:
        return float("nan")
    n = min(x.size for x in xs) // 2
    if n < 4:
        return float("nan")
    halves = []
    for x in xs:
        t = x[x.size - 2 * n:]
        halves += [t[:n], t[n:]]
    h = _np.stack(halves)
    if not _np.all(_np.isfinite(h)):
        return float("nan")
    W = h.var(axis=1, ddof=1).mean()
    if not W > 0.0:
        return float("nan")
    B = n * h.mean(axis=1).var(ddof=1)
    return float(_np.sqrt(((n - 1.0) / n * W + B / n) / W))


def _lp_summary(rows, z):
    """out["logpost"] from the (S, 4) rows and the label trace as sampled: rows that were not folded are NaN"""
    lj = rows[:, 3]
    used = _np.nonzero(~_np.isnan(lj))[0]
    out = {k: _np.ascontiguousarray(rows[:, q]) for q, k in enumerate(_LP_KEYS)}
    best = int(used[_np.argmax(lj[used])]) if used.size else -1  # the first maximum
    out.update(best=best, z_map=z[best].copy() if best >= 0 else _np.full(z.shape[1], NA_INTEGER, dtype=_np.int32),
               ess=ess(lj[used]), n_used=int(used.size))
    return out


class _LogPostOut(_C.Structure):  # bmm_logpost_out
    _fields_ = [("rows", _C.c_void_p), ("z_best", _C.c_void_p), ("best_total", _C.c_void_p), ("best_row", _C.c_void_p)]


class _LogPost(_Option):
    """Outputs of an armed bmm_set_logpost: the run fills them (include/bmm_mcmc.h "log joint trace", DESIGN.md
    section 20).  With several chains nothing is armed: every chain is scored afterwards (_lp_chains).  relabel_to:
    (the ecr_pivot="map" request, K, device) of a run that is then relabelled to its best state."""
    key = "logpost"

    def __init__(self, N, S, relabel_to=None):
        self.relabel_to = relabel_to
        self.rows = _np.full((S, 4), _np.nan, order="F")
        self.z = _np.full(N, NA_INTEGER, dtype=_np.int32)
        self.total = _C.c_double(float("nan"))
        self.best = _C.c_int(-1)
        self.s = _LogPostOut(self.rows.ctypes.data, self.z.ctypes.data, _C.addressof(self.total), _C.addressof(self.best))

    def arm(self):
        _capi.check(_capi.lib().bmm_set_logpost(_C.byref(self.s)))

    def result(self):
        lj = self.rows[:, 3]
        used = _np.nonzero(~_np.isnan(lj))[0]
        out = {k: _np.ascontiguousarray(self.rows[:, q]) for q, k in enumerate(_LP_KEYS)}
        out.update(best=self.best.value, z_map=self.z, ess=ess(lj[used]), n_used=int(used.size))
        return out

    def into(self, out):
        """a single chain's object: the armed outputs attached, then the relabelling to the best state"""
        out["logpost"] = self.result()
        return out if self.relabel_to is None else _ecr_map([out], *self.relabel_to)[0]


# ---------------------------------------------------------------- temper=: parallel tempering, a replica ladder
TEMPER_MAX_RUNGS = 8


def temper_ladder(R, hottest=0.1):
    """R inverse temperatures from 1 down to `hottest`, geometrically spaced (R = 1: just 1)."""
    R = int(R)
    if not 1 <= R <= TEMPER_MAX_RUNGS:
        raise ValueError("a ladder has 1 to %d rungs" % TEMPER_MAX_RUNGS)
    if not 0.0 < hottest < 1.0:
        raise ValueError("hottest must lie in (0, 1)")
    b = _np.ones(R)
    if R > 1:
        b[1:] = float(hottest) ** (_np.arange(1, R) / (R - 1.0))
    return b


class _TemperOut(_C.Structure):  # bmm_temper_out
    _fields_ = [("R", _C.c_int), ("inv_temp", _C.c_void_p), ("swap_every", _C.c_int), ("proposed", _C.c_void_p),
                ("accepted", _C.c_void_p), ("walker_cold", _C.c_void_p), ("loglik", _C.c_void_p)]


class _Temper(_Option):
    """Outputs of an armed bmm_set_temper: the run fills them (include/bmm_mcmc.h "parallel tempering", DESIGN.md
    section 21)."""
    key = "temper"

    def __init__(self, inv_temp, swap_every, S):
        self.b = _np.ascontiguousarray(inv_temp, dtype=_np.float64)
        R = self.b.size
        self.proposed = _np.zeros(max(R - 1, 1), dtype=_np.int64)[:max(R - 1, 0)]
        self.accepted = _np.zeros(max(R - 1, 1), dtype=_np.int64)[:max(R - 1, 0)]
        self.walker = _np.zeros(S, dtype=_np.int32)
        self.loglik = _np.full((S, R), _np.nan, order="F")
        self.s = _TemperOut(R, self.b.ctypes.data, int(swap_every), self.proposed.ctypes.data, self.accepted.ctypes.data,
                            self.walker.ctypes.data, self.loglik.ctypes.data)

    def arm(self):
        _capi.check(_capi.lib().bmm_set_temper(_C.byref(self.s)))

    def result(self):
        with _np.errstate(invalid="ignore", divide="ignore"):
            rate = self.accepted / self.proposed.astype(_np.float64)
        return {"inv_temp": self.b, "proposed": self.proposed, "accepted": self.accepted, "rate": rate,
                "walker_cold": self.walker, "loglik": self.loglik}


def _make_temper(temper, swap_every, S, chains, hottest=0.1):
    """temper= of a wrapper: a sequence of inverse temperatures starting at 1, or the number of rungs of
    temper_ladder(); None when off"""
    if temper is None:
        return None
    if int(chains) > 1:
        raise _capi.BmmError(2, "temper= is offered per chain (chains=1): the rungs of a ladder are its chains")
    if _np.ndim(temper) == 0 and not 1 <= int(temper) <= TEMPER_MAX_RUNGS:  # (as the library refuses a sequence of that length)
        raise _capi.BmmError(1, "temper: a ladder has 1 to %d rungs" % TEMPER_MAX_RUNGS)
    b = temper_ladder(temper, hottest) if _np.ndim(temper) == 0 else _np.asarray(temper, dtype=_np.float64).ravel()
    return _Temper(b, swap_every, S)


def log_joint(X, z, sampler, K, alpha=1.0, beta=0.5, gamma=0.5, a=1, b=1, sample_alpha=False, k_open=None, prior_k=None,
              mask=None, rho=0.5, device=0):
    """The log joint rows of any stack of label rows over the data X, on the device (bmm_device_log_joint; include/bmm_mcmc.h
    "log joint trace").  z: (S, N) labels in 1..K, as a run returns them (or one row); sampler: "collapsed", "dp",
    "stickbreaking", "full" or "allocation"; K: K or maxK; alpha: one value or S values, the concentration after each
    sweep (a run's out["alpha"]; the allocation sampler: a); sample_alpha: whether the chain sampled alpha, so that its
    Gamma(a, b) prior enters log_hyper; k_open (S values) and prior_k (see log_prior_k): the allocation sampler's K
    trace and prior; mask: (P,) or (S, P) indicators in {0, 1} with rho (one mask per call: an (S, P) trace is scored
    row by row).  Returns {"log_lik", "log_prior", "log_hyper", "log_joint"}, each (S,).  A run's own z and alpha give
    the run's rows bit for bit."""
    _refuse_categorical(X, "log_joint")
    X = _capi.as_x(X)
    N, P = X.shape
    z = _np.asarray(z)
    z = _as_trace(z.reshape(1, -1) if z.ndim == 1 else z)
    S = z.shape[0]
    if z.shape[1] != N:
        raise ValueError("z must have one column per observation")
    alloc = sampler == "allocation"
    code = 0 if alloc else _capi.SAMPLER_CODE[sampler]
    K = int(K)
    al = _np.ascontiguousarray(_np.broadcast_to(_np.asarray(alpha, dtype=_np.float64).ravel(), (S,)))
    lp = ko = None
    if alloc:
        if k_open is None:
            raise ValueError('sampler="allocation" needs k_open, the K trace')
        lp = log_prior_k("poisson" if prior_k is None else prior_k, K)
        ko = _np.ascontiguousarray(_np.broadcast_to(_np.asarray(k_open, dtype=_np.int32).ravel(), (S,)))
    if mask is not None:
        m = _np.asarray(mask, dtype=_np.uint8)
        if m.ndim == 2:
            if m.shape != (S, P):
                raise ValueError("a mask trace must be S x P")
            parts = [log_joint(X, z[s:s + 1], sampler, K, al[s], beta, gamma, a, b, sample_alpha,
                               None if ko is None else ko[s:s + 1], prior_k, m[s], rho, device) for s in range(S)]
            return {k: _np.concatenate([p_[k] for p_ in parts]) for k in _LP_KEYS}
        m = _np.ascontiguousarray(m.ravel())
        if m.shape != (P,):
            raise ValueError("mask must have one indicator per feature")
    else:
        m = None
    out = _np.full((S, 4), _np.nan, order="F")
    _capi.check(_capi.lib().bmm_device_log_joint(
        _C.c_int(device), _capi.vp(X), _C.c_int64(N), _C.c_int(P), _C.c_int(code), _C.c_int(K), _C.c_double(beta),
        _C.c_double(gamma), _C.c_int(1 if sample_alpha else 0), _C.c_double(a), _C.c_double(b),
        None if lp is None else _capi.vp(lp), _capi.vp(z), _C.c_int(S), _capi.vp(al), None if ko is None else _capi.vp(ko),
        None if m is None else _capi.vp(m), _C.c_double(rho), _capi.vp(out)))
    return {k: _np.ascontiguousarray(out[:, q]) for q, k in enumerate(_LP_KEYS)}


def _lp_chains(chains_out, X, sampler, K, alpha, beta, gamma, a, b, device):
    """chains > 1: every chain object is scored through the stand-alone call (rows that are no partition -- the
    unassigned starting state of a run without burn-in -- stay NaN) and gains "logpost", with "rhat", the split-R-hat of
    log_joint over the chains, and "chain", the chain that holds the overall best state."""
    sample = alpha is None or float(alpha) == 0.0
    for o in chains_out:
        z = o["z"]
        S = z.shape[0]
        keep = [s for s in range(S) if z[s].min() >= 1]
        rows = _np.full((S, 4), _np.nan)
        if keep:
            r = log_joint(X, z[keep], sampler, K, o["alpha"].ravel()[keep], beta, gamma, a, b, sample, device=device)
            for q, k in enumerate(_LP_KEYS):
                rows[keep, q] = r[k]
        o["logpost"] = _lp_summary(rows, z)
    lps = [o["logpost"] for o in chains_out]
    r = rhat([lp["log_joint"][~_np.isnan(lp["log_joint"])] for lp in lps])
    tops = [lp["log_joint"][lp["best"]] if lp["best"] >= 0 else -_np.inf for lp in lps]
    top = int(_np.argmax(tops))
    for lp in lps:
        lp.update(rhat=r, chain=top)
    return chains_out


def _logpost_request(logpost, ecr_req, N, S, chains, K, device):
    """logpost= of a wrapper (ecr_pivot="map" implies it): (lp, ecr_req for the run, the "map" request or None); lp:
    the outputs to arm for a single chain, True for several (they are scored afterwards), None when off"""
    ecr_map = ecr_req if ecr_req is not None and ecr_req[0] == _ECR_MAP else None
    if not logpost and ecr_map is None:
        return None, ecr_req, None
    lp = True if chains > 1 else _LogPost(N, S, None if ecr_map is None else (ecr_map, K, device))
    return lp, None if ecr_map is not None else ecr_req, ecr_map


def _ecr_map(outs, req, K, device):
    """ecr_pivot="map": the chains' traces relabelled to the best state among them all, after the run(s)"""
    lps = [o["logpost"] for o in outs]
    top = lps[0].get("chain", 0)
    return _ecr_chains(outs, (_ECR_GIVEN, _np.ascontiguousarray(lps[top]["z_map"], dtype=_np.int32), req[2]), K, device)


# ---------------------------------------------------------------- pair_check=: pairwise local-dependence check
PAIR_CHECK_MAX_M = 128  # include/bmm_mcmc.h BMM_PAIR_CHECK_MAX_M


class _PairCheckOut(_C.Structure):  # bmm_pair_check_out
    _fields_ = [("feat", _C.c_void_p), ("M", _C.c_int), ("stride", _C.c_int), ("z_rows", _C.c_void_p), ("x2_rows", _C.c_void_p),
                ("sum_z", _C.c_void_p), ("sum_z2", _C.c_void_p), ("sum_x2", _C.c_void_p), ("sum_df", _C.c_void_p),
                ("n_z", _C.c_void_p), ("n11", _C.c_void_p), ("n_folded", _C.c_void_p)]


class _PairCheckPlanOut(_C.Structure):  # bmm_pair_check_plan_out
    _fields_ = [("bytes_slices", _C.c_int64), ("bytes_counts", _C.c_int64), ("bytes_fold", _C.c_int64), ("chunks", _C.c_int64),
                ("chunks_per_slice", _C.c_int64), ("chunks_per_round", _C.c_int), ("tiles", _C.c_int), ("row_slices", _C.c_int),
                ("label_blocks", _C.c_int), ("ka", _C.c_int), ("pairs_per_lane", _C.c_int), ("threads", _C.c_int)]


def _pc_features(features, P):
    """the chosen features as int32: True / None means all P of them, which needs P <= PAIR_CHECK_MAX_M"""
    if features is None or features is True:
        if P > PAIR_CHECK_MAX_M:
            raise ValueError("pair_check=True checks every pair of the %d features, more than %d: give a list of feature "
                             "indices" % (P, PAIR_CHECK_MAX_M))
        return _np.arange(P, dtype=_np.int32)
    f = _np.ascontiguousarray(_np.asarray(features).ravel(), dtype=_np.int32)
    if not 2 <= f.size <= PAIR_CHECK_MAX_M:
        raise ValueError("pair_check takes 2 to %d features, not %d" % (PAIR_CHECK_MAX_M, f.size))
    if f.min() < 0 or f.max() >= P:
        raise ValueError("pair_check: a feature index lies outside 0..%d" % (P - 1))
    if _np.unique(f).size != f.size:
        raise ValueError("pair_check: the chosen features must be distinct")
    return f


def pair_check_pairs(M):
    """the (npairs, 2) positions (i < j) in the feature list, in the library's pair order: numpy.triu_indices(M, 1)"""
    i, j = _np.triu_indices(int(M), 1)
    return _np.stack([i, j], axis=1).astype(_np.int32)


class _PairFold(_Option):
    """the host side of a fold: the buffers a bmm_pair_check_out points at, and the summary made of them"""
    key = "pair_check"

    def __init__(self, feat, stride=1, S=0, trace=False):
        self.feat = feat
        M = feat.size
        np_ = M * (M - 1) // 2
        self.sum_z, self.sum_z2, self.sum_x2 = _np.zeros(np_), _np.zeros(np_), _np.zeros(np_)
        self.sum_df = _np.zeros(np_, dtype=_np.int64)
        self.n_z = _np.zeros(np_, dtype=_np.int32)
        self.n11 = _np.zeros(np_, dtype=_np.uint32)
        self.n_folded = _C.c_int(0)
        self.z = _np.full((S, np_), _np.nan, order="F") if trace else None
        self.x2 = _np.full((S, np_), _np.nan, order="F") if trace else None
        self.s = _PairCheckOut(feat.ctypes.data, M, int(stride), None if self.z is None else self.z.ctypes.data,
                               None if self.x2 is None else self.x2.ctypes.data, self.sum_z.ctypes.data, self.sum_z2.ctypes.data,
                               self.sum_x2.ctypes.data, self.sum_df.ctypes.data, self.n_z.ctypes.data, self.n11.ctypes.data,
                               _C.addressof(self.n_folded))

    def arm(self):
        _capi.check(_capi.lib().bmm_set_pair_check(_C.byref(self.s)))

    def result(self):
        n, nz = self.n_folded.value, self.n_z
        with _np.errstate(invalid="ignore", divide="ignore"):
            out = {"features": self.feat.copy(), "pairs": pair_check_pairs(self.feat.size), "n11": self.n11,
                   "z_mean": _np.where(nz > 0, self.sum_z / nz, _np.nan), "z_rms": _np.where(nz > 0, _np.sqrt(self.sum_z2 / nz), _np.nan),
                   "x2_mean": self.sum_x2 / n if n else _np.full(self.sum_x2.shape, _np.nan),
                   "df_mean": self.sum_df / n if n else _np.full(self.sum_x2.shape, _np.nan), "n_folded": n,
                   "sum_z": self.sum_z, "sum_z2": self.sum_z2, "sum_x2": self.sum_x2, "sum_df": self.sum_df, "n_z": nz}
        if self.z is not None:
            out["z"], out["x2"] = self.z, self.x2
        return out


def _make_pair_check(pair_check, stride, trace, P, S, chains):
    """pair_check= of a wrapper: the outputs to arm, None when off; refused before a device is touched"""
    if pair_check is None or pair_check is False:
        return None
    if int(chains) > 1:
        raise ValueError("pair_check= is offered per chain (chains=1)")
    if int(stride) < 1:
        raise ValueError("pair_check_stride must be >= 1")
    return _PairFold(_pc_features(pair_check, P), stride, S, bool(trace))


def pair_check(X, z, Kc, features=None, counts=False, device=0):
    """The pairwise local-dependence check of any stack of label rows over the data X, on the device
    (bmm_device_pair_check; include/bmm_mcmc.h "pairwise local-dependence check").  z: (S, N)
    labels in 1..Kc, as a run returns them (or one row); features: the chosen feature indices (default: all P, which
    needs P <= 128).  Returns the summary of a run's out["pair_check"] folded over the S rows, with "z" and "x2" (S,
    npairs), and with counts=True "counts" (S, Kc, npairs) uint32, the co-occurrence counts per label.  A run's own z
    gives the run's rows bit for bit."""
    _refuse_categorical(X, "pair_check")
    X = _capi.as_x(X)
    N, P = X.shape
    z = _np.asarray(z)
    z = _as_trace(z.reshape(1, -1) if z.ndim == 1 else z)
    S = z.shape[0]
    if z.shape[1] != N:
        raise ValueError("z must have one column per observation")
    fold = _PairFold(_pc_features(features, P))
    np_ = fold.sum_z.size
    rows = _np.full((S, 2 * np_), _np.nan, order="F")
    cnt = _np.zeros((S, int(Kc), np_), dtype=_np.uint32) if counts else None
    _capi.check(_capi.lib().bmm_device_pair_check(
        _C.c_int(device), _capi.vp(X), _C.c_int64(N), _C.c_int(P), _C.c_int(int(Kc)), _capi.vp(z), _C.c_int(S),
        _capi.vp(fold.feat), _C.c_int(fold.feat.size), None if cnt is None else _capi.vp(cnt), _capi.vp(rows), _C.byref(fold.s)))
    out = fold.result()
    out["z"], out["x2"] = _np.ascontiguousarray(rows[:, :np_]), _np.ascontiguousarray(rows[:, np_:])
    if counts:
        out["counts"] = cnt
    return out


def pair_check_plan(N, Kc, M):
    """What the check needs on the device and the grid of its counting kernel (bmm_pair_check_plan): a dict of
    bytes_slices, bytes_counts, bytes_fold, chunks (of 64 rows), chunks_per_slice, chunks_per_round, tiles, row_slices,
    label_blocks, ka, pairs_per_lane, threads"""
    o = _PairCheckPlanOut()
    _capi.check(_capi.lib().bmm_pair_check_plan(_C.c_int64(int(N)), _C.c_int(int(Kc)), _C.c_int(int(M)), _C.byref(o)))
    return {k: int(getattr(o, k)) for k, _ in _PairCheckPlanOut._fields_}


# ---------------------------------------------------------------- split_merge=: Jain & Neal's move for the DP chain
SPLIT_MERGE_SCANS = 5  # the default of split_merge_scans (DESIGN.md section 15 says where it comes from)
_SM_FIELDS = ("split_proposed", "split_accepted", "merge_proposed", "merge_accepted", "skipped")


# ---------------------------------------------------------------- summary=: online pivot relabelling, memberships
_SUMMARY_PIVOT_NONE, _SUMMARY_PIVOT_FIRST, _SUMMARY_PIVOT_GIVEN = 0, 1, 2
_SUMMARY_PLAN_FIELDS = ("threads", "fold_workgroups", "grid_cap", "pitch", "fold_lds_bytes", "profile_workgroups",
                        "finish_workgroups", "finish_lds_bytes", "bytes_counts", "bytes_block", "launches_pivot",
                        "launches_plain")


class _SummaryOpts(_C.Structure):  # bmm_summary_opts
    _fields_ = [("pivot_kind", _C.c_int), ("pivot", _C.c_void_p), ("stride", _C.c_int), ("keep_trace", _C.c_int)]


class _SummaryOut(_C.Structure):  # bmm_summary_out
    _fields_ = [("pivot", _C.c_void_p), ("z_hat", _C.c_void_p), ("n_max", _C.c_void_p), ("n_folded", _C.c_void_p),
                ("size_sum", _C.c_void_p), ("theta_sum", _C.c_void_p), ("theta_sq", _C.c_void_p), ("theta_n", _C.c_void_p),
                ("alpha_sum", _C.c_void_p), ("agree", _C.c_void_p), ("permutations", _C.c_void_p), ("counts", _C.c_void_p)]


def _summary_pivot(pivot, N):
    """summary_pivot= of a wrapper: (kind, labels or None); the labels' range is the library's to check"""
    if pivot is None:
        return _SUMMARY_PIVOT_NONE, None
    if isinstance(pivot, str):
        if pivot != "first":
            raise ValueError('summary_pivot must be "first", None or N labels')
        return _SUMMARY_PIVOT_FIRST, None
    pv = _np.ascontiguousarray(pivot, dtype=_np.int32).ravel()
    if pv.shape != (N,):
        raise ValueError("summary_pivot must have one label per observation")
    return _SUMMARY_PIVOT_GIVEN, pv


class _SummaryFold(_Option):
    """the host side of a summary: the buffers a bmm_summary_out points at, and the result derived from them"""
    key = "summary"

    def __init__(self, N, K, P, pivot, stride, counts=False, S=0, keep_trace=True):
        kind, self.given = _summary_pivot(pivot, N)
        self.N, self.keep_trace = N, bool(keep_trace)
        self.pivot = _np.zeros(N, dtype=_np.int32)
        self.z_hat = _np.zeros(N, dtype=_np.int32)
        self.n_max = _np.zeros(N, dtype=_np.uint32)
        self.n_folded = _C.c_int(0)
        self.size_sum = _np.zeros(K, dtype=_np.int64)
        self.theta_sum = _np.zeros((K, P), order="F")
        self.theta_sq = _np.zeros((K, P), order="F")
        self.theta_n = _np.zeros(K, dtype=_np.int32)
        self.alpha_sum = _np.zeros(2)
        self.agree = _np.full(S, -1, dtype=_np.int64) if S else None
        self.perms = _np.empty((S, K), dtype=_np.int32, order="F") if S else None
        self.counts = _np.zeros((N, K), dtype=_np.uint32, order="F") if counts else None
        self.opts = _SummaryOpts(kind, None if self.given is None else self.given.ctypes.data, int(stride), int(self.keep_trace))
        self.s = _SummaryOut(self.pivot.ctypes.data, self.z_hat.ctypes.data, self.n_max.ctypes.data, _C.addressof(self.n_folded),
                             self.size_sum.ctypes.data, self.theta_sum.ctypes.data, self.theta_sq.ctypes.data,
                             self.theta_n.ctypes.data, self.alpha_sum.ctypes.data,
                             None if self.agree is None else self.agree.ctypes.data,
                             None if self.perms is None else self.perms.ctypes.data,
                             None if self.counts is None else self.counts.ctypes.data)

    def arm(self):
        _capi.check(_capi.lib().bmm_set_summary(_C.byref(self.opts), _C.byref(self.s)))

    def result(self):
        n = self.n_folded.value
        tn = self.theta_n.astype(_np.float64)[:, None]
        with _np.errstate(divide="ignore", invalid="ignore"):
            mean = self.theta_sum / tn
            sd = _np.sqrt(_np.maximum(self.theta_sq / tn - mean * mean, 0.0))
            total = self.size_sum.sum()
            pi_mean = self.size_sum / float(total) if total else _np.full(self.size_sum.shape, _np.nan)
        out = {"pivot": None if self.opts.pivot_kind == _SUMMARY_PIVOT_NONE else self.pivot, "z_hat": self.z_hat,
               "n_max": self.n_max, "n_folded": n, "size_sum": self.size_sum, "pi_mean": pi_mean,
               "theta_sum": self.theta_sum, "theta_sq": self.theta_sq, "theta_n": self.theta_n, "theta_mean": mean,
               "theta_sd": sd, "alpha_mean": self.alpha_sum[0] / n if n else float("nan"), "alpha_sum": self.alpha_sum,
               "agree": self.agree, "permutations": self.perms}
        if self.counts is not None:
            out["counts"] = self.counts
        return out

    def into(self, out):
        out["summary"] = self.result()
        if not self.keep_trace:
            out["z"] = None
        return out


def _make_summary(summary, pivot, stride, keep_trace, N, K, P, S, chains, relabel=False, partition=None, similarity_of=None):
    """summary= and keep_trace= of a wrapper: the outputs to arm, None when off.  What the wrapper itself cannot run is
    refused here, before a device is touched; the library refuses the rest with its codes (include/bmm_mcmc.h)."""
    on = not (summary is None or summary is False)
    if not on:
        if not keep_trace:
            raise ValueError("keep_trace=False drops the label trace: it needs summary=, which folds the labels on the device")
        return None
    if not (summary is True or (isinstance(summary, str) and summary == "counts")):
        raise ValueError('summary must be True, "counts" or None')
    if int(chains) > 1:
        raise ValueError("summary= is offered per chain (chains=1)")
    if relabel:
        raise ValueError("summary= relabels against its pivot as the chain runs: not together with relabel= (two relabellings)")
    if not keep_trace and (partition is not None or similarity_of is not None):
        raise ValueError("keep_trace=False drops the label trace, which partition= and similarity_of= read")
    return _SummaryFold(N, K, P, pivot, stride, counts=summary == "counts", S=S, keep_trace=keep_trace)


def _z_trace(S, N, su):
    """the (S, N) label trace a run fills, or None for a run that keeps none (keep_trace=False)"""
    if su is not None and not su.keep_trace:
        return None
    return _np.empty((S, N), dtype=_np.int32, order="F")  # every cell is written by the library


def _vp0(a):
    return None if a is None else _capi.vp(a)


def run_bytes(sampler, N, P, K, S, keep_trace=True, summary=False):
    """The bytes of device memory a run's own buffers take (bmm_run_bytes): the theta, alpha and pi traces, with
    keep_trace the S x N label trace and the two staging blocks of its way out, and with summary the summary's block
    (K planes of N counters, N-sized pivot and outputs, the sums) and its per-sweep rows.  The chain's resident state
    (the bit planes of X, two label rows, the tables) is not part of it.  Pure: no device is touched."""
    code = _capi.SAMPLER_CODE[sampler] if isinstance(sampler, str) else int(sampler)
    v = _capi.lib().bmm_run_bytes(_C.c_int(code), _C.c_int64(int(N)), _C.c_int(int(P)), _C.c_int(int(K)), _C.c_int(int(S)),
                        _C.c_int(int(bool(keep_trace))), _C.c_int(int(bool(summary))))
    if v < 0:
        raise ValueError("run_bytes: sampler, N, P, K and S must name a run")
    return int(v)


def summary_plan(N, P, K):
    """The launch shapes of the summary's kernels and the bytes of its block (bmm_summary_plan), read from the function
    the launches read without touching a device: a dict of the fields include/bmm_mcmc.h lists."""
    out = (_C.c_int64 * 12)()
    _capi.check(_capi.lib().bmm_summary_plan(_C.c_int64(int(N)), _C.c_int(int(P)), _C.c_int(int(K)), out))
    return dict(zip(_SUMMARY_PLAN_FIELDS, (int(v) for v in out)))


class _SplitMergeStep(_C.Structure):  # bmm_split_merge_step
    _fields_ = [("row_i", _C.c_int64), ("row_j", _C.c_int64), ("label_a", _C.c_int32), ("label_b", _C.c_int32),
                ("kind", _C.c_int32), ("accepted", _C.c_int32), ("members", _C.c_int64), ("n_before", _C.c_int64 * 2),
                ("n_after", _C.c_int64 * 2), ("log_prior", _C.c_double), ("log_lik", _C.c_double),
                ("log_q", _C.c_double), ("log_u", _C.c_double), ("log_r", _C.c_double), ("sweep", _C.c_uint32),
                ("move", _C.c_uint32), ("launch_side", _C.c_void_p), ("proposal_side", _C.c_void_p)]


class _SplitMerge(_Option):
    """split_merge= of gibbs_dp and (alloc) of gibbs_allocation, checked before any device is touched and armed for
    exactly one run"""
    key = "split_merge"

    def __init__(self, moves, scans, alloc=False):
        self.moves, self.scans = int(moves), int(scans)
        self.infix, self.fields = ("alloc_", _AS_FIELDS) if alloc else ("", _SM_FIELDS)

    def arm(self):
        _capi.check(getattr(_capi.lib(), "bmm_set_%ssplit_merge" % self.infix)(_C.c_int(self.moves), _C.c_int(self.scans)))

    def result(self):
        out = (_C.c_int64 * 5)()
        _capi.check(getattr(_capi.lib(), "bmm_last_%ssplit_merge_stats" % self.infix)(out))
        return dict(zip(self.fields, (int(v) for v in out)))


def _make_split_merge(split_merge, scans, chains, alloc=False):
    moves = int(split_merge or 0)
    scans = SPLIT_MERGE_SCANS if scans is None else int(scans)
    if moves < 0 or scans < 0:
        raise ValueError("split_merge and split_merge_scans must be >= 0")
    if moves == 0:
        return None
    if int(chains) > 1:
        raise ValueError("split_merge= is offered per chain (chains=1)")
    return _SplitMerge(moves, scans, alloc)


# ---------------------------------------------------------------- gibbs_allocation: unknown K for the finite chain
_EA_FIELDS = ("eject_proposed", "eject_accepted", "absorb_proposed", "absorb_accepted")


class _AllocStep(_C.Structure):  # bmm_alloc_step
    _fields_ = [("kind", _C.c_int32), ("accepted", _C.c_int32), ("j1", _C.c_int32), ("j2", _C.c_int32),
                ("k_before", _C.c_int32), ("k_after", _C.c_int32), ("pe_bits", _C.c_uint64), ("members", _C.c_int64),
                ("n_before", _C.c_int64 * 2), ("n_after", _C.c_int64 * 2), ("log_prior", _C.c_double),
                ("log_lik", _C.c_double), ("log_q", _C.c_double), ("log_move", _C.c_double), ("log_u", _C.c_double),
                ("log_r", _C.c_double), ("sweep", _C.c_uint32), ("move", _C.c_uint32), ("side", _C.c_void_p)]


class _AllocSplitStep(_C.Structure):  # bmm_alloc_split_step
    _fields_ = [("row_i", _C.c_int64), ("row_j", _C.c_int64), ("label_a", _C.c_int32), ("label_b", _C.c_int32),
                ("kind", _C.c_int32), ("accepted", _C.c_int32), ("k_before", _C.c_int32), ("k_after", _C.c_int32),
                ("moved", _C.c_int32), ("pad", _C.c_int32), ("members", _C.c_int64), ("n_before", _C.c_int64 * 2),
                ("n_after", _C.c_int64 * 2), ("log_prior", _C.c_double), ("log_lik", _C.c_double),
                ("log_q", _C.c_double), ("log_u", _C.c_double), ("log_r", _C.c_double), ("sweep", _C.c_uint32),
                ("move", _C.c_uint32), ("launch_side", _C.c_void_p), ("proposal_side", _C.c_void_p)]


_AS_FIELDS = ("proposed_splits", "accepted_splits", "proposed_merges", "accepted_merges", "skipped")


def log_prior_k(prior_k, maxK):
    """log p(K), K = 1..maxK: "poisson" (Poisson(1) truncated to 1..maxK, the default of Nobile & Fearnside 2007),
    "uniform", or maxK positive weights (normalised here)"""
    maxK = int(maxK)
    if isinstance(prior_k, str):
        if prior_k == "poisson":
            lw = -_np.cumsum(_np.log(_np.arange(1.0, maxK + 1.0)))  # -log K!
        elif prior_k == "uniform":
            lw = _np.zeros(maxK)
        else:
            raise ValueError('prior_k is "poisson", "uniform" or an array of maxK weights')
    else:
        w = _np.asarray(prior_k, dtype=_np.float64)
        if w.shape != (maxK,) or not _np.all(_np.isfinite(w)) or not _np.all(w > 0.0):
            raise ValueError("prior_k needs maxK finite positive weights: the moves must be able to reach every K")
        lw = _np.log(w)
    return _np.ascontiguousarray(lw - _np.log(_np.sum(_np.exp(lw - lw.max()))) - lw.max())


def gibbs_allocation(data, nsamples, maxK, a=1.0, prior_k="poisson", K0=None, moves=1, eject_a=1.0, beta=0.5, gamma=0.5,
                     burnin=None, *, seed=None, batch=None, device=0, initial_K=None, partition=None, partition_stride=1,
                     similarity_of=None, relabel=False, ecr_pivot="iterative", ecr_max_iter=50, logpost=False,
                     split_merge=0, split_merge_scans=SPLIT_MERGE_SCANS):
    """The allocation sampler of Nobile & Fearnside (2007): the finite collapsed Beta-Bernoulli mixture with the number of
    components K unknown, 1 <= K <= maxK <= 64 (include/bmm_mcmc.h "allocation sampler").  The
    weights are Dirichlet(a, ..., a) with `a` fixed per component; `prior_k`: see log_prior_k.  A sweep is the finite
    sampler's with empty labels below K kept open at their prior weight; `moves` eject / absorb moves (p_E ~
    Beta(eject_a, eject_a)) at the start of every sweep from the second change K.  The chain starts from `K0` components
    (default min(maxK, 2)) and `initial_K` (1-based labels in 1..K0; default uniform).  Returns z (S, N), theta (maxK, P,
    S) with NaN where a label is empty, K (S,), k_posterior (maxK,): the kept-sweep frequencies of K = 1..maxK, k_used
    (S,): the non-empty labels per sweep, moves: the four counts, and with `partition=` the summary of gibbs_collapsed.
    `relabel="ecr"` is refused by the library (BMM_E_UNSUPPORTED): the relabelling assumes a fixed number of components.
    `logpost=True`: as gibbs_collapsed, with log p(K) and the Dirichlet(a) prior over the open labels as log_prior.
    `split_merge=m`: m split-merge moves of the allocation sampler behind the eject / absorb moves
    of every sweep from the second, each with `split_merge_scans` intermediate restricted scans: a split opens component
    K + 1 along the data, a merge closes one.  The result gains `split_merge = {"proposed_splits", "accepted_splits",
    "proposed_merges", "accepted_merges", "skipped"}`."""
    _refuse_categorical(data, "gibbs_allocation")
    sm = _make_split_merge(split_merge, split_merge_scans, 1, alloc=True)
    X = _capi.as_x(data)
    N, P = X.shape
    nsamples, maxK = int(nsamples), int(maxK)
    burnin = _burnin(burnin, nsamples)
    seed = _seed(seed)
    K0 = min(maxK, 2) if K0 is None else int(K0)
    if not 1 <= K0 <= maxK:
        raise ValueError("K0 must lie in 1..maxK")
    lp = log_prior_k(prior_k, maxK)
    if initial_K is None:
        initial_K = _np.random.default_rng(seed).integers(1, K0 + 1, N)
    z0 = _np.ascontiguousarray(initial_K, dtype=_np.int32)
    if z0.shape != (N,):
        raise ValueError("initial_K must have one label per observation")
    S = nsamples - burnin
    pt = _make_partition(partition, partition_stride, similarity_of, N, S, 1)
    cb = _make_ball(_run_option("credible_ball"), partition, None, True, N, S, maxK, 1)
    z = _np.empty((S, N), dtype=_np.int32, order="F")
    theta = _np.zeros((maxK, P, S), order="F")
    Ks = _np.zeros(S, dtype=_np.int32)
    counts = (_C.c_int64 * 4)()
    ec = None
    if relabel:
        ecr_req = _ecr_request(relabel, None, ecr_pivot, ecr_max_iter, N, partition)[1]
        if ecr_req is None:
            raise ValueError('gibbs_allocation offers no relabelling (relabel must be False)')
        ec = _Ecr(ecr_req, N, maxK, P, S)  # armed below: the library refuses the run
    lj = _LogPost(N, S) if logpost else None
    _arm((ec, pt, cb, lj, sm))
    _capi.check(_capi.lib().bmm_alloc_run(
        _capi.vp(X), _C.c_int64(N), _C.c_int(P), _capi.vp(z0), _C.c_int(nsamples), _C.c_int(maxK), _C.c_double(a),
        _C.c_double(beta), _C.c_double(gamma), _capi.vp(lp), _C.c_int(K0), _C.c_int(int(moves)), _C.c_double(eject_a),
        _C.c_int(burnin), _C.c_int64(0 if batch is None else batch), _C.c_uint64(seed), _C.c_int(device), _capi.vp(z),
        _capi.vp(theta), _capi.vp(Ks), counts))
    used = _np.array([len(_np.unique(row)) for row in z], dtype=_np.int32)
    out = {"z": z, "theta": theta, "K": Ks, "k_posterior": _np.bincount(Ks, minlength=maxK + 1)[1:] / float(S), "k_used": used,
           "moves": dict(zip(_EA_FIELDS, (int(v) for v in counts)))}
    return _collect(out, (sm, pt, cb, lj))


# ---------------------------------------------------------------- select_features=: noise features (White, Wyse & Murphy 2016)
class _FeatureStep(_C.Structure):  # bmm_feature_step
    _fields_ = [("lambda_", _C.c_void_p), ("p", _C.c_void_p), ("u", _C.c_void_p), ("gamma", _C.c_void_p),
                ("sweep", _C.c_uint32)]


class _FeatureOut(_C.Structure):  # bmm_feature_out
    _fields_ = [("rho", _C.c_double), ("gamma", _C.c_void_p), ("inclusion", _C.c_void_p), ("inclusion_rb", _C.c_void_p),
                ("n_selected", _C.c_void_p), ("n_folded", _C.POINTER(_C.c_int))]


class _Features(_Option):
    """select_features= of gibbs_collapsed / gibbs_dp, checked before any device is touched and armed for one run"""
    key = "features"

    def __init__(self, rho, P, S):
        self.rho = float(rho)
        self.gamma = _np.zeros((S, P), dtype=_np.uint8)
        self.inclusion, self.inclusion_rb = _np.zeros(P), _np.zeros(P)
        self.n_selected = _np.zeros(S, dtype=_np.int32)
        self.n = _C.c_int(0)
        self.s = _FeatureOut(self.rho, _capi.vp(self.gamma), _capi.vp(self.inclusion), _capi.vp(self.inclusion_rb),
                             _capi.vp(self.n_selected), _C.pointer(self.n))

    def arm(self):
        _capi.check(_capi.lib().bmm_set_feature_select(_C.byref(self.s)))

    def result(self):
        return {"gamma": self.gamma, "inclusion": self.inclusion, "inclusion_rb": self.inclusion_rb,
                "n_selected": self.n_selected, "rho": self.rho, "n_folded": self.n.value}


def _make_features(select_features, rho, P, S, chains, beta, gamma, dp, newdata, loo, split_merge=0):
    if not select_features:
        return None
    rho = float(rho)
    if not 0.0 < rho < 1.0:
        raise ValueError("rho must lie strictly inside (0, 1): it is the prior probability that a feature clusters")
    if int(chains) > 1:
        raise ValueError("select_features= is offered per chain (chains=1)")
    if dp and float(beta) != float(gamma):
        raise ValueError("select_features= on the DP sampler needs beta == gamma: its new-cluster term is the model's only then")
    if newdata is not None or (loo is not None and loo is not False) or int(split_merge or 0) > 0:
        raise ValueError("select_features= is not offered together with newdata=, loo= or split_merge=: their tables and "
                         "ratios are written for the all-features model")
    return _Features(rho, P, S)


# ---------------------------------------------------------------- missing=: NA cells imputed on the device
class _MissingOut(_C.Structure):  # bmm_missing_out
    _fields_ = [("mean_rb", _C.c_void_p), ("mean_draw", _C.c_void_p), ("last", _C.c_void_p), ("n_folded", _C.POINTER(_C.c_int64))]


class _Missing(_Option):
    """missing= of the four samplers: the sorted cell list, armed for exactly one run"""
    key = "missing"

    def __init__(self, rows, cols, N, P):
        self.rows, self.cols, self.size = rows, cols, N * P
        n = rows.size
        self.mean, self.mean_draw = _np.full(n, _np.nan), _np.full(n, _np.nan)
        self.last = _np.zeros(n, dtype=_np.uint8)
        self.n = _C.c_int64(0)
        self.s = _MissingOut(_capi.vp(self.mean), _capi.vp(self.mean_draw), _capi.vp(self.last), _C.pointer(self.n))

    def arm(self):
        _capi.check(_capi.lib().bmm_set_missing(_capi.vp(self.rows), _capi.vp(self.cols), _C.c_int64(self.rows.size), _C.byref(self.s)))

    def result(self):
        return {"rows": self.rows, "cols": self.cols, "n_cells": int(self.rows.size),
                "fraction": self.rows.size / self.size if self.size else 0.0, "mean": self.mean, "mean_draw": self.mean_draw,
                "last": self.last, "n_folded": int(self.n.value)}


def _take_missing(data, missing):
    """(cleaned data, the cells or None): what the wrappers do with missing= before the matrix is looked at"""
    if missing is None:
        return data, None
    rows, cols, data = _capi.missing_cells(data, missing)
    return data, (rows, cols)


# ---------------------------------------------------------------- known= / allowed=: constrained allocations
class _Constraints(_Option):
    """known= / allowed= of the four samplers: the sorted row list and the masks, armed for exactly one run"""
    key = "constraints"

    def __init__(self, rows, masks):
        self.rows, self.masks = rows, masks

    def arm(self):
        _capi.check(_capi.lib().bmm_set_constraints(_C.c_int64(self.rows.size), _capi.vp(self.rows), _capi.vp(self.masks)))

    def result(self):
        pr, rv = _C.c_int64(0), _C.c_int64(0)
        _capi.check(_capi.lib().bmm_last_constraint_stats(_C.byref(pr), _C.byref(rv)))
        return _constraint_result(self.rows, self.masks, pr.value, rv.value)


def _constraint_result(rows, masks, proposed, reverted):
    return {"rows": rows, "n_rows": int(rows.size), "n_known": int(((masks & (masks - _np.uint64(1))) == 0).sum()),
            "proposed": int(proposed), "reverted": int(reverted), "rate": reverted / proposed if proposed else float("nan")}


def _take_constraints(known, allowed, N, K, sets=True):
    """None, or the armed list of known= / allowed=; `sets`: whether the sampler takes allowed= (its labels are classes)"""
    if known is None and allowed is None:
        return None
    if allowed is not None and not sets:
        raise ValueError("allowed= is offered by gibbs_collapsed and gibbs_full only: a label of gibbs_dp and "
                         "gibbs_stickbreaking is whatever cluster holds it, so only known= rows can pin one")
    rows, masks, _ = _capi.constraint_list(N, K, known, allowed)
    return _Constraints(rows, masks)


# ---------------------------------------------------------------- init=: the k-modes++ start on the device
INIT_KINDS = {"kmodes": 1}
INIT_ITERS = 10  # a cap, not a tuned value: the refinement stops at the first round that changes no label


class _InitInfo(_C.Structure):  # bmm_init_info
    _fields_ = [("k_eff", _C.c_int32), ("rounds_run", _C.c_int32), ("changed_last", _C.c_int64), ("cost", _C.c_int64),
                ("device_ms", _C.c_double)]

    def as_dict(self):
        return {"k_eff": int(self.k_eff), "rounds_run": int(self.rounds_run), "changed_last": int(self.changed_last),
                "cost": int(self.cost), "device_ms": float(self.device_ms)}


def _init_kind(init, init_iters, allowed=True):
    """None for the random start, else (kind, iters); `allowed`: whether the sampler offers a data-driven start"""
    if init is None or init == "random":
        return None
    if not allowed:
        raise ValueError("init=%r: a data-driven start is offered by gibbs_collapsed only (Chain.init_labels seats a "
                         "resident DP chain)" % (init,))
    if init not in INIT_KINDS:
        raise ValueError('init must be "random" or "kmodes"')
    iters = int(init_iters)
    if iters < 0:
        raise ValueError("init_iters must be >= 0")
    return INIT_KINDS[init], iters


class _Init(_Option):
    """init= of gibbs_collapsed, armed for exactly one run"""
    key = "init"

    def __init__(self, kind, iters):
        self.kind, self.iters = kind, iters

    def arm(self):
        _capi.check(_capi.lib().bmm_set_init(_C.c_int(self.kind), _C.c_int(self.iters)))

    def result(self):
        info = _InitInfo()
        _capi.check(_capi.lib().bmm_last_init_info(_C.byref(info)))
        return info.as_dict()


# ---------------------------------------------------------------- categorical features: the data says what it is
class Categorical(_np.ndarray):
    """What categorical() returns: the expanded N x P 0/1 matrix (int32, column-major), carrying `levels` (F,: the levels
    of every feature), `chain_levels` (F,: what the library is told -- 1 for a two-level feature, which is one Bernoulli
    column, else L), `columns` (feature -> slice of its columns) and decode().  Only the object itself carries them: a
    slice, a copy or numpy.asarray of it is a plain 0/1 matrix, and is modelled as one."""

    def __array_finalize__(self, obj):
        self.levels = self.chain_levels = self.columns = None

    def decode(self, theta):
        """theta (K, P), or (K, P, S), as the chain reports it (S / Nk per column) -> a list of F arrays (K, L_j[, S]): the
        level proportions of every feature; a two-level feature's are (1 - theta, theta)."""
        theta = _np.asarray(theta)
        if self.columns is None or theta.ndim < 2 or theta.shape[1] != self.shape[1]:
            raise ValueError("decode takes the K x P theta of a chain over these columns")
        out = []
        for L, sl in zip(self.levels, self.columns):
            t = theta[:, sl]
            out.append(_np.concatenate((1.0 - t, t), axis=1) if L == 2 else t)
        return out


def categorical(X, levels=None):
    """An N x F integer matrix of categorical features -- feature j takes the values 0 .. L_j - 1 -- as data for
    gibbs_collapsed and gibbs_dp (include/bmm_mcmc.h "categorical features").  `levels`: L_j per
    feature, each >= 2; None: the column's maximum + 1 (at least 2).  Returns the expanded 0/1 matrix (Categorical): a
    feature of L >= 3 levels is a block of L neighbouring one-hot columns, modelled with a symmetric Dirichlet(beta, ...,
    beta) prior on its level probabilities (beta: the run's); a feature of 2 levels is ONE Bernoulli column (its value)
    under the run's Beta(beta, gamma) -- with gamma != beta its two levels are not exchangeable, as in the Bernoulli
    model.  Handing the object to gibbs_collapsed or gibbs_dp arms the levels: the result gains `categorical = {"levels",
    "columns"}`, `theta` holds the level proportions column by column (decode() splits it per feature), and a partition
    is scored under the categorical likelihood, not under L independent Bernoulli columns.  Not offered (ValueError,
    before the library is asked): the other samplers, chains > 1, temper=, select_features=, split_merge=, missing=,
    newdata=, loo=, logpost= (and ecr_pivot="map"), pair_check=, init="kmodes", relabel=True.  partition= with its search
    and credible ball, relabel="ecr", known= / allowed=, summary= and keep_trace= work as ever.  A resident chain takes
    the raw vector instead: Chain.set_categorical."""
    X = _np.asarray(X)
    if X.ndim != 2 or X.dtype.kind not in "iub" or X.shape[1] < 1:
        raise ValueError("categorical takes an N x F integer matrix")
    N, F = X.shape
    X = X.astype(_np.int64)
    if levels is None:
        lv = _np.maximum(X.max(axis=0) + 1, 2) if N else _np.full(F, 2, dtype=_np.int64)
    else:
        lv = _np.asarray(levels)
        if lv.shape != (F,) or lv.dtype.kind not in "iu":
            raise ValueError("levels must hold one integer per feature")
        lv = lv.astype(_np.int64)
    if (lv < 2).any():
        raise ValueError("feature %d has %d levels: a feature has at least 2" % (int(_np.flatnonzero(lv < 2)[0]), int(lv[lv < 2][0])))
    if (lv > 255).any():
        raise ValueError("feature %d has %d levels: at most 255 are offered" % (int(_np.flatnonzero(lv > 255)[0]), int(lv[lv > 255][0])))
    bad = (X < 0) | (X >= lv[None, :])
    if bad.any():
        i, j = (int(v[0]) for v in _np.nonzero(bad))
        raise ValueError("row %d, feature %d: the value %d lies outside 0 .. %d" % (i, j, int(X[i, j]), int(lv[j]) - 1))
    width = _np.where(lv == 2, 1, lv)
    first = _np.concatenate(([0], _np.cumsum(width)))
    out = _np.zeros((N, int(first[-1])), dtype=_np.int32, order="F").view(Categorical)
    rows = _np.arange(N)
    for j in range(F):
        if lv[j] == 2:
            out[:, first[j]] = X[:, j]
        else:
            _np.asarray(out)[rows, first[j] + X[:, j]] = 1
    out.levels = lv.astype(_np.int32)
    out.chain_levels = _np.ascontiguousarray(width, dtype=_np.int32)
    out.columns = [slice(int(first[j]), int(first[j + 1])) for j in range(F)]
    return out


def _categorical_of(data):
    return data if isinstance(data, Categorical) and data.levels is not None else None


def _refuse_categorical(data, who, **options):
    """categorical data handed to something that models a Bernoulli cell per column: refused before the library is asked"""
    if _categorical_of(data) is None:
        return
    if who is not None:
        raise ValueError("%s models every column as a Bernoulli cell: categorical data go to gibbs_collapsed and gibbs_dp" % who)
    armed = [k for k, v in options.items() if v]
    if armed:
        raise ValueError("%s= is not offered with categorical data: it knows the Bernoulli cell only" % armed[0])


class _Categorical(_Option):
    """the levels of categorical data, armed for exactly one run"""
    key = "categorical"

    def __init__(self, data):
        self.levels, self.columns, self.raw = data.levels.copy(), list(data.columns), data.chain_levels

    def arm(self):
        _capi.check(_capi.lib().bmm_set_categorical(_capi.vp(self.raw), _C.c_int(self.raw.size)))

    def result(self):
        return {"levels": self.levels, "columns": self.columns}


class _CategoricalPlanOut(_C.Structure):  # bmm_categorical_plan_out
    _fields_ = [("n_columns", _C.c_int32), ("n_blocks", _C.c_int32), ("generic", _C.c_int32), ("threads", _C.c_int32),
                ("lanes", _C.c_int32), ("packed", _C.c_int32), ("builds_own_tables", _C.c_int32), ("batch", _C.c_int64)]


def categorical_plan(sampler, N, K, levels, batch=None, num_cus=256):
    """What bmm_categorical_plan reports of a raw levels vector (1: a Bernoulli column, L >= 2: a block of L one-hot
    columns) without touching a device: {"P", "n_blocks", "first_column" (F,), "lev" (P,) uint8: 0 or the L of the column's
    block, "generic", "threads", "lanes_per_observation", "packed", "builds_own_tables", "batch"}."""
    lv = _np.ascontiguousarray(levels, dtype=_np.int32)
    if lv.ndim != 1:
        raise ValueError("levels is a vector")
    first = _np.zeros(max(lv.size, 1), dtype=_np.int32)
    lev = _np.zeros(max(int(_np.maximum(lv, 1).sum()), 1), dtype=_np.uint8)
    o = _CategoricalPlanOut()
    _capi.check(_capi.lib().bmm_categorical_plan(_C.c_int(_capi.SAMPLER_CODE[sampler]), _C.c_int64(N), _C.c_int(K),
                                                 _C.c_int64(0 if batch is None else batch), _C.c_int(num_cus), _capi.vp(lv),
                                                 _C.c_int(lv.size), _capi.vp(first), _capi.vp(lev), _C.byref(o)))
    return {"P": int(o.n_columns), "n_blocks": int(o.n_blocks), "first_column": first[:lv.size], "lev": lev[:o.n_columns],
            "generic": bool(o.generic), "threads": int(o.threads), "lanes_per_observation": int(o.lanes),
            "packed": bool(o.packed), "builds_own_tables": bool(o.builds_own_tables), "batch": int(o.batch)}


def _run(base, args, options, pr=None, hooks=None, rel=None):
    """One *_run call: plain / hooked (bmm_<base>_run_probs), relabelled on the device (_run_relabel), or either of
    them with the predictive of new rows (_run_predict).  options: what is armed for exactly this call, in the order
    of arming -- _gibbs lists it with the start of init= last, just ahead of the call: a run of another sampler
    refuses an armed start."""
    L = _capi.lib()
    _arm(options)
    if pr is None:
        if rel is not None:
            return getattr(L, "bmm_%s_run_relabel" % base)(*args, rel.ref())
        return getattr(L, "bmm_%s_run_probs" % base)(*args, hooks.ref() if hooks else None)
    pr.arm()
    pr.s.relabel = _C.addressof(rel.s) if rel is not None else None
    pr.s.hooks = _C.addressof(hooks.hooks) if hooks is not None else None
    return getattr(L, "bmm_%s_run_predict" % base)(*args, _capi.vp(pr.X), _C.c_int64(pr.M), _C.byref(pr.s))


def stephens_batch(p, device=0):
    """my_stephens_batch (src/stephens.cpp:6-66) on the device: p is an N x K x M cube of allocation
    probabilities; returns (Q, perm) -- Q (N x K) the one computed at the start of the last of the 100
    iterations, perm (M x K, 0-based) that iteration's permutations."""
    p = _np.asfortranarray(p, dtype=_np.float64)
    if p.ndim != 3:
        raise ValueError("p must be an N x K x M cube")
    N, K, M = p.shape
    Q = _np.zeros((N, K), order="F")
    perm = _np.zeros((M, K), dtype=_np.int32, order="F")
    _capi.check(_capi.lib().bmm_device_stephens_batch(_C.c_int(device), _capi.vp(p), _C.c_int64(N), _C.c_int(K),
                                                      _C.c_int(M), _capi.vp(Q), _capi.vp(perm)))
    return Q, perm


def stephens_online(Q, p, j, device=0, with_cost=False):
    """my_stephens_online (src/stephens.cpp:68-94) on the device for sweep j: returns (perm, Q_new), and the
    K x K cost matrix the assignment was solved on with with_cost=True."""
    Q = _np.asfortranarray(Q, dtype=_np.float64)
    p = _np.asfortranarray(p, dtype=_np.float64)
    if p.ndim != 2 or Q.shape != p.shape:
        raise ValueError("Q and p must both be N x K")
    N, K = p.shape
    perm = _np.zeros(K, dtype=_np.int32)
    Qn = _np.zeros((N, K), order="F")
    C = _np.zeros((K, K), order="F")
    _capi.check(_capi.lib().bmm_device_stephens_online(_C.c_int(device), _capi.vp(Q), _capi.vp(p), _C.c_int64(N),
                                                       _C.c_int(K), _C.c_int(int(j)), _capi.vp(perm), _capi.vp(Qn),
                                                       _capi.vp(C)))
    return (perm, Qn, C) if with_cost else (perm, Qn)


_PLAN_FIELDS = ("groups_online", "groups_batch", "rows_online", "rows_batch", "blocks_per_thread", "tile_rows",
                "blocks", "thread_groups", "cost_in_lds", "cols_per_lane")


def stephens_plan(N, K, M=0):
    """Which form of the relabelling kernels the shape (N rows, K categories, M batch slices; M = 0: the online
    step only) runs, read from the library's own launch arithmetic without touching a device (include/bmm_mcmc.h,
    bmm_device_stephens_plan): a dict of workgroups and rows per workgroup of the cost pass (online, and per slice
    of the batch), 4 x 4 blocks per thread, rows per LDS tile, blocks, thread groups, cost-in-LDS (0/1) and columns
    per lane of the assignment."""
    out = (_C.c_int64 * 12)()
    _capi.check(_capi.lib().bmm_device_stephens_plan(_C.c_int64(int(N)), _C.c_int(int(K)), _C.c_int(int(M)), out))
    return dict(zip(_PLAN_FIELDS, (int(v) for v in out)))


class DeviceStephens:
    """The two functions of src/stephens.h on a device, for the hook path (stephens=DeviceStephens(0)): each call
    moves its inputs over PCIe.  stephens="device" keeps the whole relabelling resident instead."""

    def __init__(self, device=0):
        self.device = int(device)

    def batch(self, p):
        return stephens_batch(p, self.device)[0]

    def online(self, Q, p, j):
        return stephens_online(Q, p, j, self.device)


# ---------------------------------------------------------------- progress ("Sample j", as the reference prints it)
_PROGRESS_FN = _C.CFUNCTYPE(_C.c_int, _C.c_void_p, _C.c_int, _C.c_int, _C.c_int)
_progress_every = 0


def set_progress(every=0):
    """The reference prints "Sample j" at every sweep (src/collapsed_gibbs.cpp:85; gibbs_dp adds the number of
    clusters, src/collapsed_gibbs_dp.cpp:99).  Here a run is silent unless asked: set_progress(100) prints that
    line every 100 sweeps of the single-chain calls that follow, set_progress(0) turns it off; debug=True prints
    every sweep.  Returns the previous setting (the R wrapper is bmm_progress(), R/gibbs.R)."""
    global _progress_every
    old, _progress_every = _progress_every, max(0, int(every))
    return old


def _print_progress(user, sample, nsamples, k_used):
    print("Sample %d" % sample if k_used < 0 else "Sample %d\tK: %d" % (sample, k_used), flush=True)
    return 0


_progress_cb = _PROGRESS_FN(_print_progress)


class _progress:
    """the hook around one run: every sweep with debug=True, else what set_progress asked for"""

    def __init__(self, debug):
        self.every = 1 if debug else _progress_every

    def __enter__(self):
        if self.every:
            _capi.lib().bmm_set_progress(_progress_cb, None, _C.c_int(self.every))

    def __exit__(self, *exc):
        if self.every:
            _capi.lib().bmm_set_progress(_PROGRESS_FN(0), None, _C.c_int(0))


def _clamp_burnrelabel(burnrelabel, burnin):
    return int(round(0.1 * burnin)) if burnrelabel > burnin else int(burnrelabel)  # R/utils.R:26,41,72


def _ptr_table(arrays, ctype=_C.c_void_p):
    return (ctype * len(arrays))(*[a.ctypes.data for a in arrays])


def _devices(chains, devices):
    if devices is None:
        return None
    dv = [int(d) for d in devices]
    if len(dv) != chains:
        raise ValueError("devices must name one device per chain")
    return (_C.c_int * chains)(*dv)


def _multi(sampler, X, chains, devices, z0s, pi0s, th0s, nsamples, K, alpha, beta, gamma, a, b, burnin, batch,
           seed, with_pi):
    """bmm_multi_run: `chains` independent chains (seed + c) over one upload of the data."""
    N, P = X.shape
    S = nsamples - burnin
    zs = [_np.empty((S, N), dtype=_np.int32, order="F") for _ in range(chains)]  # every cell is written by the library
    ths = [_np.zeros((K, P, S), order="F") for _ in range(chains)]
    als = [_np.zeros((S, 1), order="F") for _ in range(chains)]
    pis = [_np.zeros((S, K), order="F") for _ in range(chains)] if with_pi else None
    rc = _capi.lib().bmm_multi_run(
        _C.c_int(_capi.SAMPLER_CODE[sampler]), _C.c_int(chains), _devices(chains, devices), _capi.vp(X),
        _C.c_int64(N), _C.c_int(P), _ptr_table(z0s) if z0s else None, _ptr_table(pi0s) if pi0s else None,
        _ptr_table(th0s) if th0s else None, _C.c_int(nsamples), _C.c_int(K),
        _C.c_double(0.0 if alpha is None else alpha), _C.c_double(beta), _C.c_double(gamma), _C.c_double(a),
        _C.c_double(b), _C.c_int(burnin), _C.c_int64(0 if batch is None else batch), _C.c_uint64(seed),
        _ptr_table(pis) if with_pi else None, _ptr_table(zs), _ptr_table(ths), _ptr_table(als))
    _capi.check(rc)
    out = []
    for c in range(chains):
        d = {"alpha": als[c], "permutations": _na_perm(S, K), "z": zs[c], "theta": ths[c]}
        if with_pi:
            d = {"pi": pis[c], **d}
        out.append(d)
    return out


_Sampler = _namedtuple("_Sampler", "name base start new_column waic sets clamp")
# What differs between the four samplers, beside the layout of their arguments (_run_args).  name, base: what the
# library calls the sampler and its entry points; start: the state a run starts from -- labels (initial_K), the
# parameters (initial_pi, initial_theta: such a run also returns "pi") or nothing; new_column: the new-cluster column of
# the predictive beside the K labels; waic: loo= reports WAIC; sets: allowed= is offered; clamp: burnrelabel is cut to
# the burn-in (R/utils.R:26,41,72; :97-101 has no clamp).
_COLLAPSED = _Sampler(name="collapsed", base="collapsed", start="labels", new_column=0, waic=False, sets=True, clamp=True)
_DP = _Sampler(name="dp", base="dp", start=None, new_column=1, waic=False, sets=False, clamp=True)
_STICKBREAKING = _Sampler(name="stickbreaking", base="sb", start="params", new_column=0, waic=True, sets=False, clamp=False)
_FULL = _Sampler(name="full", base="full", start="params", new_column=0, waic=True, sets=True, clamp=True)


def _start_params(seed, pi, th, K, P):
    rng = _np.random.default_rng(seed)
    if pi is None:  # R/utils.R:68-70, 98-100
        pi = _np.exp(rng.random(K))
        pi = pi / pi.sum()
    if th is None:  # R/utils.R:74, 103
        th = rng.random(K * P).reshape((K, P), order="F")
    pi = _np.ascontiguousarray(pi, dtype=_np.float64)
    th = _np.asfortranarray(th, dtype=_np.float64)
    if pi.shape != (K,) or th.shape != (K, P):
        raise ValueError("initial_pi must have K entries and initial_theta be K x P")
    return pi, th


def _run_args(spec, X, start, nsamples, K, alpha, beta, gamma, a, b, burnin, batch, seed, device, pi, z, theta, al):
    """the arguments the three entry points of a sampler share, as include/bmm_mcmc.h orders them; z: None for a run
    that keeps no label trace"""
    data = (_capi.vp(X), _C.c_int64(X.shape[0]), _C.c_int(X.shape[1]))
    n, k, burn, bt = _C.c_int(nsamples), _C.c_int(K), _C.c_int(burnin), _C.c_int64(0 if batch is None else batch)
    hyper = (_C.c_double(0.0 if alpha is None else alpha), _C.c_double(beta), _C.c_double(gamma), _C.c_double(a), _C.c_double(b))
    where = (_C.c_uint64(seed), _C.c_int(device))
    out = (_vp0(z), _capi.vp(theta), _capi.vp(al))
    if spec.base == "collapsed":
        return data + (_capi.vp(start), n, k) + hyper + (burn, bt) + where + out
    if spec.base == "dp":
        return data + (n,) + hyper + (burn, k, bt) + where + out
    return data + (_capi.vp(start[0]), _capi.vp(start[1]), n, k) + hyper + (burn,) + where + (_capi.vp(pi),) + out


def _gibbs(spec, data, nsamples, K, *, alpha, beta, gamma, a, b, burnin, relabel, burnrelabel, debug, seed, device, chains,
           devices, stephens, newdata, predictive_trace, responsibilities, partition, partition_stride, similarity_of, loo,
           ecr_pivot, ecr_max_iter, logpost, pair_check, pair_check_stride, pair_check_trace, missing, known, allowed,
           summary, summary_pivot, summary_stride, keep_trace, partition_search, newdata_missing, credible_ball=None, batch=None,
           initial_K=None, initial_pi=None, initial_theta=None, init="random", init_iters=INIT_ITERS, select_features=False, rho=0.5,
           split_merge=0, split_merge_scans=None, temper=None, swap_every=1, temper_hottest=0.1):
    """The run behind gibbs_collapsed, gibbs_dp, gibbs_stickbreaking and gibbs_full (K: K or maxK): the keywords parsed
    into the run's options and refused where they do not go together, several chains handed to the multi-chain call and
    pooled, or one run with its options armed (_run) and what they hold collected into the result.  An option a sampler
    does not offer is one its wrapper does not pass: the defaults here mean off."""
    ct = None
    if _categorical_of(data) is not None:  # (plain data: nothing new is looked at, nothing new is called)
        _refuse_categorical(data, None if spec in (_COLLAPSED, _DP) else "gibbs_" + spec.name)
        _refuse_categorical(data, None, chains=int(chains) > 1, temper=temper is not None, select_features=select_features,
                            split_merge=int(split_merge or 0) > 0, missing=missing is not None, newdata=newdata is not None,
                            loo=loo is not None and loo is not False, logpost=bool(logpost) or ecr_pivot == "map",
                            pair_check=pair_check is not None and pair_check is not False,
                            init=init is not None and init != "random", relabel=bool(relabel) and relabel != "ecr")
        ct = _Categorical(data)
    data, cells = _take_missing(data, missing)
    X = _capi.as_x(data)
    N, P = X.shape
    mi = None if cells is None else _Missing(cells[0], cells[1], N, P)
    nsamples, K = int(nsamples), int(K)
    cs = _take_constraints(known, allowed, N, K, sets=spec.sets)
    ik = _init_kind(init, init_iters)
    if ik is not None and initial_K is not None:
        raise ValueError('init="kmodes" computes the starting labels: not together with initial_K')
    ini = None if ik is None else _Init(*ik)
    burnin = _burnin(burnin, nsamples)
    seed = _seed(seed)
    chains = int(chains)
    S = nsamples - burnin
    with_pi = spec.start == "params"
    relabel, ecr_req = _ecr_request(relabel, stephens, ecr_pivot, ecr_max_iter, N, partition)
    pr = None if newdata is None else _Predict(newdata, P, S, K + spec.new_column, predictive_trace, responsibilities, chains,
                                               newdata_missing, burnin)
    pt = _make_partition(partition, partition_stride, similarity_of, N, S, chains)
    ps = _make_search(partition_search, partition, N, K, chains)
    cb = _make_ball(credible_ball, partition, ps, keep_trace, N, S, K, chains)
    features = (select_features, rho, P, S, chains, beta, gamma, spec is _DP, newdata, loo, split_merge)
    if spec is _COLLAPSED:  # (whose refusals of select_features= have always come ahead of those of loo=; gibbs_dp: behind them)
        fs = _make_features(*features)
    lo = _make_loo(loo, N, S, chains, spec.waic)
    if spec is not _COLLAPSED:
        fs = _make_features(*features)
    sm = _make_split_merge(split_merge, split_merge_scans, chains)
    lp, ecr_req, ecr_map = _logpost_request(logpost, ecr_req, N, S, chains, K, device)
    pc = _make_pair_check(pair_check, pair_check_stride, pair_check_trace, P, S, chains)
    tp = _make_temper(temper, swap_every, S, chains, temper_hottest)
    su = _make_summary(summary, summary_pivot, summary_stride, keep_trace, N, K, P, S, chains,
                       bool(relabel) or ecr_req is not None, partition, similarity_of)
    if chains > 1:
        _arm((mi, cs))  # (the run of several chains answers them)
        if relabel:
            raise NotImplementedError("relabel=TRUE is offered per chain (chains=1)")
        z0s = pi0s = th0s = None
        infos = []
        if ini is not None:
            initial_K = []
            for c in range(chains):
                with Chain("collapsed", N, P, K, alpha=alpha, beta=beta, gamma=gamma, a=a, b=b, seed=seed + c, device=0) as ch:
                    ch.set_data(X)
                    info = ch.init_labels("kmodes", iters=ik[1])
                    infos.append({k: info[k] for k in ("k_eff", "rounds_run", "changed_last", "cost", "device_ms")})
                    initial_K.append(ch.labels())
        if spec.start == "labels":
            z0s = [_np.ascontiguousarray(_np.random.default_rng(seed + c).integers(1, K + 1, N), dtype=_np.int32)
                   for c in range(chains)] if initial_K is None else [_np.ascontiguousarray(z, dtype=_np.int32) for z in initial_K]
        elif with_pi:
            st = [_start_params(seed + c, initial_pi[c] if initial_pi is not None else None,
                                initial_theta[c] if initial_theta is not None else None, K, P) for c in range(chains)]
            pi0s, th0s = [p for p, _ in st], [t for _, t in st]
        dev0 = device if devices is None else int(devices[0])
        outs = _multi(spec.name, X, chains, devices, z0s, pi0s, th0s, nsamples, K, alpha, beta, gamma, a, b, burnin, batch, seed, with_pi)
        if lp is not None:
            _lp_chains(outs, X, spec.name, K, alpha, beta, gamma, a, b, dev0)
        outs = _pooled_search(_pooled(outs, partition, partition_stride, similarity_of, dev0), ps, partition, K, dev0)
        outs = _ecr_chains(_pooled_ball(outs, cb, ps, partition, K, dev0), ecr_req, K, dev0)
        if ecr_map is not None:
            outs = _ecr_map(outs, ecr_map, K, dev0)
        for o, info in zip(outs, infos):
            o["init"] = info
        return outs
    start = None
    if spec.start == "labels":
        if initial_K is None:
            initial_K = _np.random.default_rng(seed).integers(1, K + 1, N)
        start = _np.ascontiguousarray(initial_K, dtype=_np.int32)
        if start.shape != (N,):
            raise ValueError("initial_K must have one label per observation")
    W = _clamp_burnrelabel(burnrelabel, burnin) if spec.clamp else int(burnrelabel)
    on_device = _device_relabel(stephens, relabel, burnin, W)
    if with_pi:
        start = _start_params(seed, initial_pi, initial_theta, K, P)
    if on_device:
        rel = _DeviceRelabelRun(N, K, P, S, W)
    else:
        rel = _Relabel(stephens, N, K, nsamples, burnin, W) if relabel else None
    ec = None if ecr_req is None else _Ecr(ecr_req, N, K, P, S)
    z = _z_trace(S, N, su)
    theta = _np.zeros((K, P, S), order="F")
    al = _np.zeros((S, 1), order="F")
    pi = _np.zeros((S, K), order="F") if with_pi else None
    args = _run_args(spec, X, start, nsamples, K, alpha, beta, gamma, a, b, burnin, batch, seed, device, pi, z, theta, al)
    with _progress(debug):
        rc = _run(spec.base, args, (sm, fs, pt, ps, cb, lo, ec, lp, tp, pc, mi, cs, su, ct, ini), pr,
                  hooks=None if on_device else rel, rel=rel if on_device else None)
    out = {"alpha": al, "permutations": None if on_device else _na_perm(S, K), "z": z, "theta": theta}
    if with_pi:
        out = {"pi": pi, **out}
    if rel is not None:
        out = rel.finish(rc, out)
    else:
        _capi.check(rc)
    return _collect(out, (ec, pr, pt, lo, su, ps, cb, tp, sm, fs, ini, lp, pc, mi, cs, ct))


def gibbs_collapsed(data, nsamples, K, alpha=None, beta=0.5, gamma=0.5, a=1, b=1, burnin=None,
                    relabel=False, burnrelabel=50, debug=False, *, seed=None, batch=None, device=0,
                    initial_K=None, chains=1, devices=None, stephens=None, newdata=None, predictive_trace=False,
                    responsibilities=False, partition=None, partition_stride=1, similarity_of=None, loo=False,
                    select_features=False, rho=0.5, init="random", init_iters=INIT_ITERS, ecr_pivot="iterative",
                    ecr_max_iter=50, logpost=False, temper=None, swap_every=1, temper_hottest=0.1, pair_check=None,
                    pair_check_stride=1, pair_check_trace=False, missing=None, known=None, allowed=None, summary=None,
                    summary_pivot="first", summary_stride=1, keep_trace=True, partition_search=None, newdata_missing=None):
    """Collapsed Gibbs sampler, finite K (R/utils.R:37-47 -> src/collapsed_gibbs.cpp:24).

    Extra keyword-only arguments: `seed` (Philox key; default drawn from the global NumPy
    RNG), `batch` (observations resampled per frozen-statistics batch; 1 = the reference's
    sequential scan; None = library default), `device`, `initial_K` (1-based labels; default
    sampled uniformly as R/utils.R:42 does), `chains` / `devices` (several independent chains,
    seed + c, in one call: returns a list of chain objects), `stephens` (relabel=True: "device" runs
    Stephens' relabelling on the device; an object with batch / online runs host code on the hook
    path, see _Relabel).  `newdata` (M x P binary rows the chain has not seen): the result gains
    `predictive = {"lppd": (M,)}`, the log pointwise predictive density over the kept sweeps, computed on the
    device; `predictive_trace=True` adds "logdens", the (S, M) trace of log p(x_m | state of sweep s) (without
    burn-in its first row, the starting state, is NaN), `responsibilities=True` adds "resp", the (M, K) mean
    normalised category weights -- in the sampler's label order of each sweep, so they mean something only for a
    chain that does not switch labels (relabel=True does not reorder them).  The predictive itself does not
    depend on the labels.  `newdata_missing=`: None (an NA cell in newdata is an error), "na" (the NA_INTEGER / NaN cells
    of newdata) or a boolean M x P mask: incomplete new rows (include/bmm_mcmc.h "incomplete new rows", DESIGN.md section
    28).  A new row is not in the fit, so its missing cells marginalise out exactly: "lppd" and "logdens" are the density
    of the row's observed cells, and "resp" comes from the observed cells alone.  `predictive` gains `cells = {"rows",
    "cols", "n_cells", "mean", "n_folded"}` (cells sorted by (row, column), 0-based): "mean" is P(x_d = 1 | the row's
    observed cells, the fitted data), the ratio sum_s p(x_O, x_d = 1 | s) / sum_s p(x_O | s) over the kept sweeps -- the
    states weighted by the density of the row's observed cells, NOT the plain mean over the sweeps of the per-state
    probability (the chain samples its states given the fitted data, not given the new row).  A set without a missing
    cell gives exactly what it gives without the keyword.  `partition="binder"` or `"vi"`: the result gains `partition = {"criterion", "loss", "binder2",
    "best", "z", "n_used"}` -- the kept sweep that minimises the posterior expected Binder or variation-of-information
    loss over the kept sweeps (candidates every `partition_stride`-th), computed on the device from the resident trace;
    `best` is its row of `z` (of `z_original` under stephens="device": the summary is on the labels as sampled and does
    not depend on their numbering), "z" that row, `n_used` the rows used (the unassigned starting row of a run without
    burn-in is left out).  `similarity_of=` indices (0-based) adds "similarity", how often each pair of those
    observations shared a cluster.  With `chains > 1` the chains' traces are pooled into one estimate, attached to
    every chain object with "chain" naming the chain `best` indexes.  `loo=True`: the result gains `loo = {"log_cpo",
    "ess", "lppd", "mean", "var" (N,), "lpml", "min_ess", "n_folded"}`, the leave-one-out predictive of every fitted
    row over the kept sweeps, computed on the device (include/bmm_mcmc.h): log_cpo[i] estimates
    log p(x_i | X_-i), lpml is their sum (the log pseudo-marginal likelihood: compare K, priors or samplers with it),
    ess the effective sample size of each row's harmonic mean (between 1 and n_folded; small values flag an
    unreliable log_cpo).  gibbs_stickbreaking and gibbs_full add "p_waic" and "elpd_waic".  `loo="trace"` adds "ell",
    the (S, N) trace of the per-state values (without burn-in its first row is NaN).  Not offered with chains > 1.
    `select_features=True`: every feature gets an inclusion indicator with prior Bernoulli(`rho`), redrawn on the device
    behind every sweep (White, Wyse & Murphy 2016; include/bmm_mcmc.h "feature selection"): an
    excluded feature is noise, one rate shared by every row, and drops out of the allocation.  The result gains
    `features = {"gamma": (S, P) uint8, "inclusion": (P,), "inclusion_rb": (P,), "n_selected": (S,), "rho", "n_folded"}`:
    the indicators per kept sweep, their mean, the mean of their conditional probabilities (less noisy) and the number
    of included features per sweep; "n_folded" is the number of kept sweeps behind the two means (the starting row of a
    run without burn-in is not one).  Per chain; not with newdata=, loo= (or split_merge= on gibbs_dp).
    `init="kmodes"`: the chain starts from a k-modes++ allocation computed on the device from the resident bit planes
    (k-means++ seeding under Hamming distance with K centres, then at most `init_iters` k-modes rounds, stopping at the
    first that changes no label; include/bmm_mcmc.h "initial allocation") instead of the uniform
    random one; no label crosses PCIe, and the result gains `init = {"k_eff", "rounds_run", "changed_last", "cost",
    "device_ms"}`.  Not together with `initial_K`.  With `chains > 1` chain c is initialised with seed + c by a resident
    chain on device 0 and its labels are handed to the multi-chain call as `initial_K`: that one round trip of N labels
    per chain over PCIe is accepted there.  `init="random"`, the default, is the code path it always was.
    `relabel="ecr"`: the kept sweeps are relabelled from the label trace alone, on the device, after the last sweep
    (ECR, include/bmm_mcmc.h): every row gets the permutation that agrees with a pivot allocation
    on as many observations as possible.  `ecr_pivot="iterative"` (the default) votes the pivot from the rows themselves
    until the agreement stops growing (at most `ecr_max_iter` iterations), `"partition"` takes the point estimate of
    `partition=`, an array of N labels is used as given.  No probability matrix, any burnin, and the result has the keys of
    a stephens="device" run (`permutations`, `z`, `theta` relabelled, `z_original`, `theta_original`) plus `ecr = {"agree",
    "pivot", "iterations", "converged", "n_used"}`.  With `chains > 1` the chains' traces are stacked and relabelled to one
    common pivot (for "partition" the pooled estimate), so their `theta` can be averaged across chains.
    `logpost=True`: the result gains `logpost = {"log_lik", "log_prior", "log_hyper", "log_joint": (S,), "best", "z_map":
    (N,), "ess", "n_used"}` -- the log joint of the state after every kept sweep, computed on the device from the folded
    counts (include/bmm_mcmc.h "log joint trace"), the row of its first maximum and that row's
    labels (the MAP allocation among the kept states; a row of `z_original` under a relabelling: the values are those
    of the state as sampled), the effective sample size of log_joint (ess()) and the rows used (without burn-in row 0,
    the starting state, is NaN and never best).  With `chains > 1` every chain is scored afterwards and every object
    also gains "rhat", the split-R-hat of log_joint over the chains (rhat()), and "chain", the chain holding the overall
    best state.  `ecr_pivot="map"` relabels to that state (over several chains the overall best) and implies logpost.
    `temper=`: parallel tempering (include/bmm_mcmc.h "parallel tempering") -- a sequence of inverse
    temperatures starting at 1 and strictly decreasing, or an integer R meaning temper_ladder(R, temper_hottest).  Helper
    chains (seed + r, the same starting labels, the same planes) sample the posterior with the likelihood raised to
    those powers on the same device, and after every `swap_every`-th sweep neighbouring rungs exchange their states by a
    Metropolis test; everything returned is the chain at power 1, which samples the untouched posterior.  The result
    gains `temper = {"inv_temp", "proposed", "accepted", "rate": (R - 1,), "walker_cold": (S,), "loglik": (S, R)}`:
    the exchanges per neighbouring pair, which starting rung's state sat at power 1 after each kept sweep, and every
    rung's log_lik after the exchange points of kept sweeps (NaN elsewhere).  temper=[1.0] is the run without it, byte
    for byte.  Not with chains > 1, relabel=, select_features= (or split_merge= on gibbs_dp).
    `pair_check=True` or a list of 2 to 128 feature indices: the model check of local independence (include/bmm_mcmc.h
    "pairwise local-dependence check").  For every pair of the chosen features and every
    `pair_check_stride`-th kept sweep the device counts the co-occurrences per cluster and scores them against their
    hypergeometric reference given the labels and the margins: Z, the Cochran-Mantel-Haenszel score (about N(0, 1)
    under the model, signed), and X2, the per-cluster chi-square sum with df degrees of freedom (it also sees
    dependence whose sign differs between clusters).  The result gains `pair_check = {"features", "pairs" (npairs, 2:
    positions in `features`, numpy.triu_indices order), "n11" (co-occurrences in the data), "z_mean", "z_rms", "x2_mean",
    "df_mean" (npairs,), "n_folded"}` plus the raw sums, and with `pair_check_trace=True` "z" and "x2" (S, npairs), NaN
    where a sweep was not evaluated.  |z_mean| well above 4, or x2_mean far above df_mean, names a pair of features
    that stays associated inside the clusters.  It reads state only and changes no chain.  True needs P <= 128; per
    chain (chains=1); not with select_features=.
    `missing=`: None (an NA cell is an error), "na" (the NA_INTEGER cells of an integer matrix, the NaN cells of a
    floating-point one) or a boolean N x P mask.  The named cells are taken as missing at random and imputed on the device
    by data augmentation (include/bmm_mcmc.h "missing data"): they are redrawn exactly behind every
    sweep, the sweep itself runs on the completed matrix, and the labels are draws from the posterior given the observed
    cells alone.  The result gains `missing = {"rows", "cols", "n_cells", "fraction", "mean", "mean_draw", "last",
    "n_folded"}`: the cells sorted by (row, column), the posterior probability that each is a 1 ("mean", the mean over
    the kept sweeps of the rate it was drawn from; "mean_draw" is the share of ones drawn), the cells after the last
    sweep and the sweeps folded.  The `theta` row of a sweep belongs to that sweep's labels and the cells as they stood
    before its imputation step; `logpost=` gives the joint of the completed state.  With many cells missing the chain
    mixes more slowly than one that integrates them out: run longer.  Works with partition=, relabel="ecr", newdata=
    (complete rows, or incomplete ones with newdata_missing=: those cells are integrated out, not imputed) and logpost=; not with chains > 1, loo=, select_features=, temper=, pair_check=, init="kmodes",
    relabel=True (or split_merge= on gibbs_dp).
    `known=`: N integers, the rows' known classes -- 0, a negative value or NaN marks a free row, any other value is the
    row's 1-based label, which it holds in every sweep.  `allowed=`: an N x K boolean array, the labels each row may take
    (a row that is all True is free); where both name a row they must agree.  The constrained sweep is exact (include/
    bmm_mcmc.h "constraints"): a listed row is drawn as ever and keeps its label when the draw
    falls outside its set.  A few known rows per class pin the labelling, so `theta` needs no relabelling.  The starting
    labels of listed rows are put inside their sets.  The result gains `constraints = {"rows", "n_rows", "n_known",
    "proposed", "reverted", "rate"}`: the listed rows (0-based), how many hold a single label, the listed rows drawn,
    those reverted and their share (how sticky partial sets are).  Works with newdata=, partition=, relabel="ecr",
    logpost= (the joint of the whole state, held rows included), pair_check=, select_features= and missing=; not with
    chains > 1, loo=, temper=, init="kmodes", relabel=True (or split_merge= on gibbs_dp, or gibbs_allocation).
    `summary=True`: what a latent-class user takes out of a run, under one labelling, folded on the device behind the kept
    sweeps (include/bmm_mcmc.h "posterior summary").  Every `summary_stride`-th kept sweep is
    relabelled against a pivot allocation as relabel="ecr" would relabel it (`summary_pivot="first"`: the first kept
    state that is assigned, copied device to device; an array of N labels in 1..K, e.g. the partition= estimate of a
    short pilot run; None: no relabelling, the state is folded as sampled -- the choice with known=, where held rows pin
    the labelling) and folded into per-row membership counters and per-class sums.  The result gains `summary = {"pivot",
    "z_hat" (N,): each row's most frequent class, 1-based, the lowest on a tie; "n_max" (N,): in how many folded sweeps
    it sat there, so n_max / n_folded is how sure the row is; "n_folded"; "size_sum" (K,) int64, "pi_mean" (K,): the
    classes' sizes added over the folded sweeps and their shares; "theta_sum", "theta_sq" (K, P), "theta_n" (K,),
    "theta_mean", "theta_sd": the classes' item profiles (a sweep in which a class was empty is left out of its row);
    "alpha_mean"; "agree" (S,) int64 and "permutations" (S, K) int32, 0-based, per kept sweep: -1 and the identity where a
    sweep was not folded}`.  `summary="counts"` adds "counts", the (N, K) uint32 memberships (4 N K bytes).  It reads
    state only: z, theta and alpha are those of the run without it, byte for byte.  `keep_trace=False` (needs summary=):
    the run carves no S x N label trace on the device and none on the host, `z` is None, theta and alpha stay; run_bytes()
    tells what either run takes.  Per chain (chains=1); not with relabel=, temper= (two relabellings; a ladder), and
    keep_trace=False not with partition=, similarity_of=.
    `partition_search=True` (needs partition=), or a dict of `batch`, `min_batch`, `max_passes`, `max_clusters`: after the
    summary the device searches from the chosen sweep for a better estimate, moving single rows to whichever cluster
    lowers the expected loss most until none wants to move (partition_search(); include/bmm_mcmc.h "greedy search",
    DESIGN.md section 27).  `partition` gains `search = {"z", "loss", "binder2", "start_loss", "start_binder2", "passes",
    "batch", "moved", "total", "converged", "n_clusters"}`; its other keys, z, theta and alpha are those of the run without
    it, and `ecr_pivot="partition"` goes on using the visited sweep.  At most 64 categories.  With `chains > 1` the search
    runs once over the pooled traces from the pooled estimate.
    """
    return _gibbs(_COLLAPSED, data, nsamples, K, alpha=alpha, beta=beta, gamma=gamma, a=a, b=b, burnin=burnin, relabel=relabel,
                  burnrelabel=burnrelabel, debug=debug, seed=seed, batch=batch, device=device, initial_K=initial_K, chains=chains,
                  devices=devices, stephens=stephens, newdata=newdata, predictive_trace=predictive_trace,
                  responsibilities=responsibilities, partition=partition, partition_stride=partition_stride,
                  similarity_of=similarity_of, loo=loo, select_features=select_features, rho=rho, init=init, init_iters=init_iters,
                  ecr_pivot=ecr_pivot, ecr_max_iter=ecr_max_iter, logpost=logpost, temper=temper, swap_every=swap_every,
                  temper_hottest=temper_hottest, pair_check=pair_check, pair_check_stride=pair_check_stride,
                  pair_check_trace=pair_check_trace, missing=missing, known=known, allowed=allowed, summary=summary,
                  summary_pivot=summary_pivot, summary_stride=summary_stride, keep_trace=keep_trace,
                  partition_search=partition_search, newdata_missing=newdata_missing, credible_ball=_run_option("credible_ball"))


def gibbs_dp(data, nsamples, alpha=None, a=1, b=1, beta=0.5, gamma=0.5, burnin=None, relabel=False,
             burnrelabel=50, maxK=30, debug=False, *, seed=None, batch=None, device=0, chains=1, devices=None,
             stephens=None, newdata=None, predictive_trace=False, responsibilities=False, partition=None,
             partition_stride=1, similarity_of=None, loo=False, split_merge=0, split_merge_scans=None,
             select_features=False, rho=0.5, init="random", ecr_pivot="iterative", ecr_max_iter=50, logpost=False,
             temper=None, swap_every=1, temper_hottest=0.1, pair_check=None, pair_check_stride=1, pair_check_trace=False,
             missing=None, known=None, allowed=None, summary=None, summary_pivot="first", summary_stride=1, keep_trace=True,
             partition_search=None, newdata_missing=None):
    """Collapsed Gibbs sampler with a Dirichlet-process prior, truncated at maxK
    (R/utils.R:23-30 -> src/collapsed_gibbs_dp.cpp:27).  `newdata`, `predictive_trace`, `responsibilities`, `loo`: as
    gibbs_collapsed; `newdata_missing`: as gibbs_collapsed ("mean" is the importance-weighted ratio over the kept sweeps,
    the states weighted by the density of the row's observed cells; "resp" comes from the observed cells, the new-cluster
    column included); "resp" is (M, maxK + 1), the maxK labels and then the new-cluster column.  `split_merge=m`: m
    split-merge Metropolis-Hastings moves (Jain & Neal 2004, include/bmm_mcmc.h) at the start of every sweep from the
    second, each with `split_merge_scans` intermediate restricted scans (default SPLIT_MERGE_SCANS); the result gains
    `split_merge = {"split_proposed", "split_accepted", "merge_proposed", "merge_accepted", "skipped"}`.  Per chain.
    `select_features`, `rho`: as gibbs_collapsed (needs beta == gamma; not with split_merge=).  `init`: "random" only (a
    DP run seats its rows in its first sweep; Chain.init_labels re-seats a resident DP chain).  `logpost`,
    `ecr_pivot="map"`, `pair_check`, `pair_check_stride`, `pair_check_trace`: as gibbs_collapsed.  `temper`,
    `swap_every`, `temper_hottest`: as gibbs_collapsed (the helper chains seat their own rows in their first sweep; the
    new-cluster option carries the power on its likelihood part).  `missing`: as gibbs_collapsed.  `known`: as
    gibbs_collapsed, but the values name the chain's labels 1..maxK: the rows known to share a class hold one label, which
    pins that cluster there; a label that no held row occupies is an ordinary free label, and the free rows open new
    clusters as ever (the semi-supervised, novelty-detection run).  Not with split_merge=.  `allowed=` is refused here
    (ValueError): a label is whatever cluster holds it, so a set of labels says nothing about classes.  `summary`,
    `summary_pivot`, `summary_stride`, `keep_trace`: as gibbs_collapsed, over the maxK labels.  `partition_search`: as
    gibbs_collapsed (maxK <= 64)."""
    _init_kind(init, 0, allowed=False)
    return _gibbs(_DP, data, nsamples, maxK, alpha=alpha, beta=beta, gamma=gamma, a=a, b=b, burnin=burnin, relabel=relabel,
                  burnrelabel=burnrelabel, debug=debug, seed=seed, batch=batch, device=device, chains=chains, devices=devices,
                  stephens=stephens, newdata=newdata, predictive_trace=predictive_trace, responsibilities=responsibilities,
                  partition=partition, partition_stride=partition_stride, similarity_of=similarity_of, loo=loo,
                  split_merge=split_merge, split_merge_scans=split_merge_scans, select_features=select_features, rho=rho,
                  ecr_pivot=ecr_pivot, ecr_max_iter=ecr_max_iter, logpost=logpost, temper=temper, swap_every=swap_every,
                  temper_hottest=temper_hottest, pair_check=pair_check, pair_check_stride=pair_check_stride,
                  pair_check_trace=pair_check_trace, missing=missing, known=known, allowed=allowed, summary=summary,
                  summary_pivot=summary_pivot, summary_stride=summary_stride, keep_trace=keep_trace,
                  partition_search=partition_search, newdata_missing=newdata_missing, credible_ball=_run_option("credible_ball"))


def gibbs_stickbreaking(data, nsamples, maxK, alpha=None, beta=0.5, gamma=0.5, a=1, b=1, burnin=None,
                        relabel=False, burnrelabel=50, debug=False, *, seed=None, device=0, initial_pi=None,
                        initial_theta=None, chains=1, devices=None, stephens=None, newdata=None,
                        predictive_trace=False, responsibilities=False, partition=None, partition_stride=1,
                        similarity_of=None, loo=False, init="random", ecr_pivot="iterative", ecr_max_iter=50, logpost=False,
                        pair_check=None, pair_check_stride=1, pair_check_trace=False, missing=None, known=None,
                        allowed=None, summary=None, summary_pivot="first", summary_stride=1, keep_trace=True,
                        partition_search=None, newdata_missing=None):
    """Blocked Gibbs sampler, truncated stick-breaking prior (R/utils.R:95-107 ->
    src/stickbreaking.cpp:10).  The z-step is exactly parallel, so there is no batch.  `newdata`,
    `predictive_trace`, `responsibilities`, `loo`: as gibbs_collapsed; `newdata_missing`: as gibbs_collapsed, from the
    pi and theta of each kept sweep ("mean" is the importance-weighted ratio over the kept sweeps, the states weighted
    by the density of the row's observed cells; "resp" comes from the observed cells; a row with every cell missing has
    density sum(pi)); `loo` adds "p_waic" and "elpd_waic".  `init`:
    "random" only (the sampler starts from pi and theta).  `logpost`, `ecr_pivot="map"`: as gibbs_collapsed; log_prior is
    the stick-breaking prior with the sticks integrated out, which depends on the order of the labels.  `pair_check`,
    `pair_check_stride`, `pair_check_trace`: as gibbs_collapsed.  `missing`: as gibbs_collapsed; the cells are drawn from
    the theta the sweep has just drawn.  `known`, `allowed`: as gibbs_dp (the values name the chain's labels 1..maxK; allowed= is refused).
    `partition_search`: as gibbs_collapsed."""
    _init_kind(init, 0, allowed=False)
    return _gibbs(_STICKBREAKING, data, nsamples, maxK, alpha=alpha, beta=beta, gamma=gamma, a=a, b=b, burnin=burnin, relabel=relabel,
                  burnrelabel=burnrelabel, debug=debug, seed=seed, device=device, initial_pi=initial_pi,
                  initial_theta=initial_theta, chains=chains, devices=devices, stephens=stephens, newdata=newdata,
                  predictive_trace=predictive_trace, responsibilities=responsibilities, partition=partition,
                  partition_stride=partition_stride, similarity_of=similarity_of, loo=loo, ecr_pivot=ecr_pivot,
                  ecr_max_iter=ecr_max_iter, logpost=logpost, pair_check=pair_check, pair_check_stride=pair_check_stride,
                  pair_check_trace=pair_check_trace, missing=missing, known=known, allowed=allowed, summary=summary,
                  summary_pivot=summary_pivot, summary_stride=summary_stride, keep_trace=keep_trace,
                  partition_search=partition_search, newdata_missing=newdata_missing, credible_ball=_run_option("credible_ball"))


def gibbs_full(data, nsamples, K, alpha=None, beta=0.5, gamma=0.5, a=1, b=1, burnin=None, relabel=False,
               burnrelabel=50, debug=False, *, seed=None, device=0, initial_pi=None, initial_theta=None, chains=1,
               devices=None, stephens=None, newdata=None, predictive_trace=False, responsibilities=False,
               partition=None, partition_stride=1, similarity_of=None, loo=False, init="random", ecr_pivot="iterative",
               ecr_max_iter=50, logpost=False, pair_check=None, pair_check_stride=1, pair_check_trace=False, missing=None,
               known=None, allowed=None, summary=None, summary_pivot="first", summary_stride=1, keep_trace=True,
               partition_search=None, newdata_missing=None):
    """Full (uncollapsed) Gibbs sampler, finite K (R/utils.R:64-78 -> src/full_gibbs.cpp:32).  `newdata`,
    `predictive_trace`, `responsibilities`, `loo`: as gibbs_collapsed; `newdata_missing`: as gibbs_stickbreaking ("mean" is
    the importance-weighted ratio over the kept sweeps, the states weighted by the density of the row's observed cells;
    "resp" comes from the observed cells); `loo` adds "p_waic" and "elpd_waic".  `init`:
    "random" only (the sampler starts from pi and theta).  `logpost`, `ecr_pivot="map"`, `pair_check`,
    `pair_check_stride`, `pair_check_trace`, `missing`, `known`, `allowed`, `summary`, `summary_pivot`, `summary_stride`,
    `keep_trace`, `partition_search`: as gibbs_collapsed."""
    _init_kind(init, 0, allowed=False)
    return _gibbs(_FULL, data, nsamples, K, alpha=alpha, beta=beta, gamma=gamma, a=a, b=b, burnin=burnin, relabel=relabel,
                  burnrelabel=burnrelabel, debug=debug, seed=seed, device=device, initial_pi=initial_pi,
                  initial_theta=initial_theta, chains=chains, devices=devices, stephens=stephens, newdata=newdata,
                  predictive_trace=predictive_trace, responsibilities=responsibilities, partition=partition,
                  partition_stride=partition_stride, similarity_of=similarity_of, loo=loo, ecr_pivot=ecr_pivot,
                  ecr_max_iter=ecr_max_iter, logpost=logpost, pair_check=pair_check, pair_check_stride=pair_check_stride,
                  pair_check_trace=pair_check_trace, missing=missing, known=known, allowed=allowed, summary=summary,
                  summary_pivot=summary_pivot, summary_stride=summary_stride, keep_trace=keep_trace,
                  partition_search=partition_search, newdata_missing=newdata_missing, credible_ball=_run_option("credible_ball"))


class Chain:
    """One chain resident on one GPU (bmm_chain_* in include/bmm_mcmc.h): the data matrix
    and the chain state stay in HBM between `sweeps()` calls."""

    _CODE = _capi.SAMPLER_CODE

    X_LAYOUT = {"bits": 0, "int32": 1}

    def __init__(self, sampler, N, P, K, alpha=None, beta=0.5, gamma=0.5, a=1, b=1, batch=None, seed=0,
                 device=0, x_layout=None):
        self._h = _C.c_void_p()
        self.sampler, self.N, self.P, self.K = sampler, int(N), int(P), int(K)
        self._keep = None
        self._M = 0
        rc = _capi.lib().bmm_chain_create(
            _C.byref(self._h), _C.c_int(self._CODE[sampler]), _C.c_int64(N), _C.c_int(P), _C.c_int(K),
            _C.c_double(0.0 if alpha is None else alpha), _C.c_double(beta), _C.c_double(gamma),
            _C.c_double(a), _C.c_double(b), _C.c_int64(0 if batch is None else batch),
            _C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _C.c_int(device))
        _capi.check(rc)
        if x_layout is not None:  # "bits" (default: X packed once into bit planes) or "int32" (as handed over)
            _capi.check(_capi.lib().bmm_chain_set_x_layout(self._h, _C.c_int(self.X_LAYOUT[x_layout])))

    def x_layout(self):
        v = _C.c_int(0)
        _capi.check(_capi.lib().bmm_chain_get_x_layout(self._h, _C.byref(v)))
        return "int32" if v.value else "bits"

    def close(self):
        if self._h:
            _capi.lib().bmm_chain_destroy(self._h)
            self._h = _C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_data(self, X):
        X = _capi.as_x(X)
        if X.shape != (self.N, self.P):
            raise ValueError("data shape does not match the chain")
        _capi.check(_capi.lib().bmm_chain_set_data_host(self._h, _capi.vp(X)))

    def set_data_device(self, ptr, keepalive=None):
        """Borrow an int32 column-major N x P matrix already on this device (e.g. a torch
        tensor's data_ptr()); `keepalive` is held so the owner outlives the chain."""
        self._keep = keepalive
        _capi.check(_capi.lib().bmm_chain_set_data_device(self._h, _C.c_void_p(int(ptr))))

    def share_data(self, other):
        """Share the bit planes `other` (same device, N, P) already holds: several chains over one copy
        (reference-counted in the library: chains may be closed in any order)."""
        _capi.check(_capi.lib().bmm_chain_share_data(self._h, other._h))

    def planes(self):
        """(device address, words) of the chain's bit planes, allocated on first call."""
        a, n = _C.c_void_p(), _C.c_int64(0)
        _capi.check(_capi.lib().bmm_chain_planes(self._h, _C.byref(a), _C.byref(n)))
        return a.value, n.value

    def planes_filled(self):
        _capi.check(_capi.lib().bmm_chain_planes_filled(self._h))

    def set_initial_labels(self, z1):
        z1 = _np.ascontiguousarray(z1, dtype=_np.int32)
        if z1.shape != (self.N,):
            raise ValueError("one label per observation")
        _capi.check(_capi.lib().bmm_chain_set_initial_labels(self._h, _capi.vp(z1)))

    def set_initial_params(self, pi, theta):
        pi = _np.ascontiguousarray(pi, dtype=_np.float64)
        theta = _np.asfortranarray(theta, dtype=_np.float64)
        if pi.shape != (self.K,) or theta.shape != (self.K, self.P):
            raise ValueError("pi must have K entries and theta be K x P")
        _capi.check(_capi.lib().bmm_chain_set_initial_params(self._h, _capi.vp(pi), _capi.vp(theta)))

    def sweeps(self, n):
        _capi.check(_capi.lib().bmm_chain_sweeps(self._h, _C.c_int(n)))

    # -- one chain over several ranks (stick-breaking / full): see multi.ShardedChain
    def set_shard(self, N_total, first_row):
        _capi.check(_capi.lib().bmm_chain_set_shard(self._h, _C.c_int64(N_total), _C.c_int64(first_row)))

    def shard_resample(self, wait=True):
        fn = _capi.lib().bmm_chain_shard_resample if wait else _capi.lib().bmm_chain_shard_resample_async
        _capi.check(fn(self._h))

    def stream(self):
        """The chain's HIP stream handle (for ordering a caller's collective behind it)."""
        st = _C.c_void_p()
        _capi.check(_capi.lib().bmm_chain_stream(self._h, _C.byref(st)))
        return st.value

    def shard_deltas(self):
        """Device addresses of the int32 statistic deltas (dNk: K, dS: K*P) to be summed over ranks."""
        a, b = _C.c_void_p(), _C.c_void_p()
        _capi.check(_capi.lib().bmm_chain_shard_deltas(self._h, _C.byref(a), _C.byref(b)))
        return a.value, b.value

    def shard_finish(self):
        _capi.check(_capi.lib().bmm_chain_shard_finish(self._h))

    def sweep_probs(self):
        """One more sweep; returns the (N, K) matrix of allocation probabilities it drew from (the
        input of the reference's host-side relabelling)."""
        out = _np.zeros((self.N, self.K), order="F")
        _capi.check(_capi.lib().bmm_chain_sweep_probs(self._h, _capi.vp(out)))
        return out

    def sweeps_counts(self, n):
        """n more sweeps; returns the (n, K) cluster sizes after each, computed on the device."""
        out = _np.zeros((n, self.K), dtype=_np.int32)
        _capi.check(_capi.lib().bmm_chain_sweeps_counts(self._h, _C.c_int(n), _capi.vp(out)))
        return out

    def sync(self):
        _capi.check(_capi.lib().bmm_chain_sync(self._h))

    @property
    def batch(self):
        return int(_capi.lib().bmm_chain_batch(self._h))

    @property
    def sweep_index(self):
        return int(_capi.lib().bmm_chain_sweep_index(self._h))

    def labels(self):
        z = _np.zeros(self.N, dtype=_np.int32)
        _capi.check(_capi.lib().bmm_chain_get_labels(self._h, _capi.vp(z)))
        return z

    def counts(self):
        Nk = _np.zeros(self.K, dtype=_np.int32)
        S = _np.zeros((self.K, self.P), dtype=_np.int32)
        _capi.check(_capi.lib().bmm_chain_get_counts(self._h, _capi.vp(Nk), _capi.vp(S)))
        return Nk, S

    def alpha(self):
        v = _C.c_double(0.0)
        _capi.check(_capi.lib().bmm_chain_get_alpha(self._h, _C.byref(v)))
        return v.value

    def params(self):
        pi = _np.zeros(self.K)
        theta = _np.zeros((self.K, self.P), order="F")
        _capi.check(_capi.lib().bmm_chain_get_params(self._h, _capi.vp(pi), _capi.vp(theta)))
        return pi, theta

    # -- posterior predictive density of new rows (include/bmm_mcmc.h)
    def set_newdata(self, Xnew, responsibilities=False, missing=None):
        """M x P binary rows the chain has not seen, validated and packed on the device; replaces any earlier set and
        empties the accumulators (None or zero rows: drops it).  `responsibilities`: sweeps_predict also accumulates
        the mean normalised category weights (Kc more doubles per row and sweep).  `missing`: None, "na" or a boolean
        M x P mask, as newdata_missing= of the gibbs_* wrappers: the rows are incomplete, their observed cells are
        scored and their missing cells predicted."""
        if Xnew is None:
            Xnew = _np.zeros((0, self.P), dtype=_np.int32)
        cells = None
        if missing is not None:
            rows, cols, Xnew = _capi.missing_cells(Xnew, missing)
            cells = (rows, cols) if rows.size else None
        Xn = _capi.as_x(Xnew)
        if Xn.shape[1] != self.P:
            raise ValueError("newdata must have the %d columns of data" % self.P)
        _capi.check(_capi.lib().bmm_chain_predict_responsibilities(self._h, _C.c_int(1 if responsibilities else 0)))
        _capi.check(_capi.lib().bmm_chain_set_newdata_host(self._h, _capi.vp(Xn), _C.c_int64(Xn.shape[0])))
        self._M = Xn.shape[0]
        self._cells = None
        if cells is not None:
            _capi.check(_capi.lib().bmm_chain_set_newdata_missing(self._h, _capi.vp(cells[0]), _capi.vp(cells[1]), _C.c_int64(cells[0].size)))
            self._cells = cells

    def _kc(self):
        return self.K + 1 if self.sampler == "dp" else self.K

    def predict_state(self, responsibilities=False, cells=False):
        """log p(x_m | current state) for every new row, (M,); no sweep is run and the accumulators are untouched.
        With responsibilities=True returns (logdens, resp): resp (M, Kc) are the normalised category weights (DP:
        the maxK labels, then the new-cluster column), in the sampler's label order.  Incomplete new rows
        (set_newdata(missing=)): the density and the weights of the observed cells; cells=True appends the per-state
        P(x_d = 1 | the row's observed cells, this state) of every missing cell, in the order of the sorted cell list."""
        ld = _np.zeros(self._M)
        rp = _np.zeros((self._M, self._kc()), order="F") if responsibilities else None
        if cells:
            if getattr(self, "_cells", None) is None:
                raise ValueError("cells=True needs new rows with missing cells (set_newdata(missing=))")
            cl = _np.zeros(self._cells[0].size)
            _capi.check(_capi.lib().bmm_chain_predict_state_cells(self._h, _capi.vp(ld), _capi.vp(rp) if responsibilities else None,
                                                                  _capi.vp(cl)))
            return (ld, rp, cl) if responsibilities else (ld, cl)
        _capi.check(_capi.lib().bmm_chain_predict_state(self._h, _capi.vp(ld), _capi.vp(rp) if responsibilities else None))
        return (ld, rp) if responsibilities else ld

    def sweeps_predict(self, n, trace=False):
        """n more sweeps, each state folded into the running predictive.  trace=True returns the (n, M) matrix of
        log p(x_m | state after sweep s) (and waits); otherwise returns None without waiting, as sweeps()."""
        out = _np.zeros((n, self._M), order="F") if trace else None
        _capi.check(_capi.lib().bmm_chain_sweeps_predict(self._h, _C.c_int(n), _capi.vp(out) if trace else None))
        return out

    def predictive(self, responsibilities=False):
        """{"lppd": (M,), "n": states folded, "resp": (M, Kc) with responsibilities=True} over the sweeps folded so
        far.  resp is in the sampler's label order of each sweep: it means something only for a chain that does not
        switch labels."""
        lp = _np.zeros(self._M)
        rp = _np.zeros((self._M, self._kc()), order="F") if responsibilities else None
        n = _C.c_int(0)
        _capi.check(_capi.lib().bmm_chain_get_predictive(self._h, _capi.vp(lp), _capi.vp(rp) if responsibilities else None,
                                                         _C.byref(n)))
        out = {"lppd": lp, "n": n.value}
        if responsibilities:
            out["resp"] = rp
        if getattr(self, "_cells", None) is not None:
            rows, cols = self._cells
            mean = _np.zeros(rows.size)
            nf = _C.c_int(0)
            _capi.check(_capi.lib().bmm_chain_get_predictive_cells(self._h, _capi.vp(mean), _C.byref(nf)))
            out["cells"] = {"rows": rows, "cols": cols, "n_cells": int(rows.size), "mean": mean, "n_folded": nf.value}
        return out

    def set_newdata_missing(self, rows, cols):
        """the missing cells of the new rows as a sorted 0-based (row, column) list (bmm_chain_set_newdata_missing); an
        empty list drops the mask.  set_newdata(missing=) calls this."""
        rows = _np.ascontiguousarray(rows, dtype=_np.int64)
        cols = _np.ascontiguousarray(cols, dtype=_np.int32)
        if rows.shape != cols.shape or rows.ndim != 1:
            raise ValueError("rows and cols must be vectors of one length")
        _capi.check(_capi.lib().bmm_chain_set_newdata_missing(self._h, _capi.vp(rows), _capi.vp(cols), _C.c_int64(rows.size)))
        self._cells = (rows, cols) if rows.size else None

    def predict_reset(self):
        _capi.check(_capi.lib().bmm_chain_predict_reset(self._h))

    # -- leave-one-out predictive of the fitted rows (include/bmm_mcmc.h)
    def set_loo(self, on=True):
        """Arm (or disarm) the leave-one-out summary: 12 doubles per fitted row on the device.  Arming an armed chain
        empties the accumulators.  An armed chain that is not folding sweeps exactly as an unarmed one."""
        _capi.check(_capi.lib().bmm_chain_set_loo(self._h, _C.c_int(1 if on else 0)))

    def loo_state(self):
        """ell[i] = log p(x_i | everything else in the current state), (N,); no sweep is run and the accumulators
        are untouched.  Refused for a state with unseated rows (every sampler but the finite collapsed one before
        its first sweep)."""
        out = _np.zeros(self.N)
        _capi.check(_capi.lib().bmm_chain_loo_state(self._h, _capi.vp(out)))
        return out

    def sweeps_loo(self, n, trace=False):
        """n more sweeps, each state folded into the leave-one-out accumulators.  trace=True returns the (n, N)
        matrix of ell (and waits); otherwise returns None without waiting, as sweeps()."""
        out = _np.zeros((n, self.N), order="F") if trace else None
        _capi.check(_capi.lib().bmm_chain_sweeps_loo(self._h, _C.c_int(n), _capi.vp(out) if trace else None))
        return out

    def loo(self):
        """The summary over the sweeps folded so far: {"log_cpo", "ess", "lppd", "mean", "var" (N,), "lpml", "min_ess",
        "n_folded"} and, for stick-breaking and full, "p_waic" and "elpd_waic"."""
        lo = _Loo(self.N, waic=self.sampler in ("stickbreaking", "full"))
        _capi.check(_capi.lib().bmm_chain_get_loo(self._h, _C.byref(lo.s)))
        return lo.result()

    def loo_reset(self):
        _capi.check(_capi.lib().bmm_chain_loo_reset(self._h))

    # -- split-merge moves of a DP chain (include/bmm_mcmc.h)
    def set_logpost(self, on=True):
        """Arm (or disarm) the log joint trace and the keep-best state (include/bmm_mcmc.h "log joint trace", DESIGN.md
        section 20).  Arming an armed chain empties the best state."""
        _capi.check(_capi.lib().bmm_chain_set_logpost(self._h, _C.c_int(1 if on else 0)))

    def logpost_state(self):
        """{"log_lik", "log_prior", "log_hyper", "log_joint"} of the current state: no sweep, the best state untouched"""
        out = (_C.c_double * 4)()
        _capi.check(_capi.lib().bmm_chain_logpost_state(self._h, out))
        return dict(zip(_LP_KEYS, (float(v) for v in out)))

    def sweeps_logpost(self, n, trace=False):
        """n more sweeps, each offered to the keep-best state; trace=True returns their (n, 4) rows (log_lik, log_prior,
        log_hyper, log_joint) and waits"""
        rows = _np.full((int(n), 4), _np.nan, order="F") if trace else None
        _capi.check(_capi.lib().bmm_chain_sweeps_logpost(self._h, _C.c_int(int(n)), _capi.vp(rows) if trace else None))
        return rows

    def best(self):
        """{"z_map": (N,) 1-based labels of the best folded state, "log_joint", "sweep"}"""
        z = _np.empty(self.N, dtype=_np.int32)
        total, sweep = _C.c_double(0.0), _C.c_int(-1)
        _capi.check(_capi.lib().bmm_chain_get_best(self._h, _capi.vp(z), _C.byref(total), _C.byref(sweep)))
        return {"z_map": z, "log_joint": total.value, "sweep": sweep.value}

    def logpost_reset(self):
        _capi.check(_capi.lib().bmm_chain_logpost_reset(self._h))

    # -- parallel tempering (include/bmm_mcmc.h "parallel tempering")
    def set_temper(self, inv_temp=1.0, on=True):
        """The chain targets p(alpha) p(z | alpha) p(x | z)^inv_temp from its next table build on (0 < inv_temp <= 1;
        1.0 runs the tempered table kernel and gives an unarmed chain's values); on=False: as it was."""
        _capi.check(_capi.lib().bmm_chain_set_temper(self._h, _C.c_int(1 if on else 0), _C.c_double(float(inv_temp))))

    def temper(self):
        """(armed, inverse temperature)"""
        on, b = _C.c_int(0), _C.c_double(1.0)
        _capi.check(_capi.lib().bmm_chain_get_temper(self._h, _C.byref(on), _C.byref(b)))
        return bool(on.value), b.value

    # -- pairwise local-dependence check (include/bmm_mcmc.h)
    def set_pair_check(self, features=True, stride=1):
        """Arm the pair check on `features` (True: all P, which needs P <= 128; a list of 2 to 128 distinct indices), every
        `stride`-th folded sweep evaluated; None or False disarms and frees its memory.  Arming an armed chain empties
        the fold and takes the new features."""
        if features is None or features is False:
            _capi.check(_capi.lib().bmm_chain_set_pair_check(self._h, None, _C.c_int(0), _C.c_int(1)))
            self._pc_feat = None
            return
        f = _pc_features(features, self.P)
        _capi.check(_capi.lib().bmm_chain_set_pair_check(self._h, _capi.vp(f), _C.c_int(f.size), _C.c_int(int(stride))))
        self._pc_feat = f

    def _pc_np(self):
        f = getattr(self, "_pc_feat", None)
        if f is None:
            raise _capi.BmmError(5, "the pair check is not armed (Chain.set_pair_check)")
        return f.size * (f.size - 1) // 2

    def pair_check_state(self):
        """{"z", "x2" (npairs,), "df" (npairs,) int32} of the current state: no sweep, the fold untouched"""
        n = self._pc_np()
        z, x2, df = _np.empty(n), _np.empty(n), _np.empty(n, dtype=_np.int32)
        _capi.check(_capi.lib().bmm_chain_pair_check_state(self._h, _capi.vp(z), _capi.vp(x2), _capi.vp(df)))
        return {"z": z, "x2": x2, "df": df}

    def pair_counts(self, margins=False):
        """the (Kc, npairs) uint32 co-occurrence counts of the current state; margins=True: also the (Kc, M) ones per
        label and chosen feature and the (Kc,) rows per label, counted in the same pass"""
        n, K, M = self._pc_np(), self.K, self._pc_feat.size
        c = _np.empty((K, n), dtype=_np.uint32)
        m, r = _np.empty((K, M), dtype=_np.uint32), _np.empty(K, dtype=_np.uint32)
        _capi.check(_capi.lib().bmm_chain_pair_counts(self._h, _capi.vp(c), _capi.vp(m), _capi.vp(r)))
        return (c, m, r) if margins else c

    def sweeps_pair_check(self, n, trace=False):
        """n more sweeps, sweeps 0, stride, 2 stride, ... of them evaluated and folded; trace=True returns {"z", "x2"}, each
        (n, npairs) with NaN where a sweep was not evaluated, and waits"""
        n, np_ = int(n), self._pc_np()
        rows = _np.full((n, 2 * np_), _np.nan, order="F") if trace else None
        _capi.check(_capi.lib().bmm_chain_sweeps_pair_check(self._h, _C.c_int(n), _capi.vp(rows) if trace else None))
        return {"z": _np.ascontiguousarray(rows[:, :np_]), "x2": _np.ascontiguousarray(rows[:, np_:])} if trace else None

    def pair_check(self):
        """the fold so far: the summary of a run's out["pair_check"]"""
        self._pc_np()
        fold = _PairFold(self._pc_feat)
        _capi.check(_capi.lib().bmm_chain_get_pair_check(self._h, _C.byref(fold.s)))
        return fold.result()

    def pair_check_reset(self):
        _capi.check(_capi.lib().bmm_chain_pair_check_reset(self._h))

    # -- posterior summary (include/bmm_mcmc.h "posterior summary")
    def set_summary(self, pivot="first", stride=1, on=True):
        """Arm the summary: `pivot` "first" (the state after the first sweep of sweeps_summary), N labels in 1..K, or None
        (the state is folded as sampled); every `stride`-th sweep of sweeps_summary is folded.  on=False disarms and frees
        its memory.  Arming an armed chain empties the fold."""
        if not on:
            _capi.check(_capi.lib().bmm_chain_set_summary(self._h, None))
            self._sum = None
            return
        fold = _SummaryFold(self.N, self.K, self.P, pivot, stride)
        _capi.check(_capi.lib().bmm_chain_set_summary(self._h, _C.byref(fold.opts)))
        self._sum = (pivot, int(stride))

    def _sum_armed(self):
        if getattr(self, "_sum", None) is None:
            raise _capi.BmmError(5, "the summary is not armed (Chain.set_summary)")
        return self._sum

    def summary_state(self):
        """{"permutation" (K,) int32, 0-based, "agree"} of the current state against the pivot: no sweep, the fold untouched"""
        self._sum_armed()
        perm, agree = _np.zeros(self.K, dtype=_np.int32), _C.c_int64(0)
        _capi.check(_capi.lib().bmm_chain_summary_state(self._h, _capi.vp(perm), _C.byref(agree)))
        return {"permutation": perm, "agree": int(agree.value)}

    def sweeps_summary(self, n, trace=False):
        """n more sweeps, sweeps 0, stride, 2 stride, ... of them folded; trace=True returns {"agree" (n,), "permutations"
        (n, K)}, -1 and the identity where a sweep was not folded, and waits"""
        self._sum_armed()
        n = int(n)
        agree = _np.full(n, -1, dtype=_np.int64) if trace else None
        perms = _np.empty((n, self.K), dtype=_np.int32, order="F") if trace else None
        _capi.check(_capi.lib().bmm_chain_sweeps_summary(self._h, _C.c_int(n), _vp0(agree), _vp0(perms)))
        return {"agree": agree, "permutations": perms} if trace else None

    def summary(self, counts=False):
        """the fold so far: the summary of a run's out["summary"] (without its per-sweep "agree" and "permutations")"""
        pivot, stride = self._sum_armed()
        fold = _SummaryFold(self.N, self.K, self.P, pivot, stride, counts=counts)
        _capi.check(_capi.lib().bmm_chain_get_summary(self._h, _C.byref(fold.s)))
        return fold.result()

    def summary_reset(self):
        _capi.check(_capi.lib().bmm_chain_summary_reset(self._h))

    def set_split_merge(self, moves_per_sweep, scans=SPLIT_MERGE_SCANS):
        """`moves_per_sweep` moves at the start of every sweep from the second (0: off), `scans` intermediate scans each."""
        _capi.check(_capi.lib().bmm_chain_set_split_merge(self._h, _C.c_int(int(moves_per_sweep)), _C.c_int(int(scans))))

    def split_merge(self, n):
        """n moves now, enqueued behind whatever the chain is doing."""
        _capi.check(_capi.lib().bmm_chain_split_merge(self._h, _C.c_int(int(n))))

    def split_merge_step(self, sides=False):
        """One move, waited for; its diagnostics as a dict (labels 1-based, rows 0-based).  `sides=True` adds
        "launch_side" and "proposal_side": one byte per row (0 / 1 a member's side, 2 / 3 the anchors, 255 outside)."""
        s = _SplitMergeStep()
        la = pr = None
        if sides:
            la, pr = _np.zeros(self.N, dtype=_np.uint8), _np.zeros(self.N, dtype=_np.uint8)
            s.launch_side, s.proposal_side = la.ctypes.data, pr.ctypes.data
        _capi.check(_capi.lib().bmm_chain_split_merge_step(self._h, _C.byref(s)))
        out = {"rows": (int(s.row_i), int(s.row_j)), "labels": (int(s.label_a), int(s.label_b)),
               "kind": ("split", "merge", "skipped")[s.kind], "accepted": bool(s.accepted), "members": int(s.members),
               "n_before": (int(s.n_before[0]), int(s.n_before[1])), "n_after": (int(s.n_after[0]), int(s.n_after[1])),
               "log_prior": s.log_prior, "log_lik": s.log_lik, "log_q": s.log_q, "log_u": s.log_u, "log_r": s.log_r,
               "sweep": int(s.sweep), "move": int(s.move)}
        if sides:
            out["launch_side"], out["proposal_side"] = la, pr
        return out

    def split_merge_stats(self):
        out = (_C.c_int64 * 5)()
        _capi.check(_capi.lib().bmm_chain_split_merge_stats(self._h, out))
        return dict(zip(_SM_FIELDS, (int(v) for v in out)))

    # -- the allocation sampler: a finite collapsed chain with K unknown (include/bmm_mcmc.h)
    def set_alloc(self, prior_k="poisson", moves_per_sweep=1, eject_a=1.0):
        """Arms the chain, for good: K = maxK components open (set_k changes it), the chain's alpha the Dirichlet
        parameter a per component, `moves_per_sweep` eject / absorb moves at the start of every sweep from the second."""
        lp = log_prior_k(prior_k, self.K)
        _capi.check(_capi.lib().bmm_chain_set_alloc(self._h, _capi.vp(lp), _C.c_int(int(moves_per_sweep)), _C.c_double(eject_a)))

    def set_k(self, K):
        _capi.check(_capi.lib().bmm_chain_set_k(self._h, _C.c_int(int(K))))

    def k(self):
        v = _C.c_int(0)
        _capi.check(_capi.lib().bmm_chain_get_k(self._h, _C.byref(v)))
        return v.value

    def alloc(self, n):
        """n eject / absorb moves now, enqueued behind whatever the chain is doing."""
        _capi.check(_capi.lib().bmm_chain_alloc(self._h, _C.c_int(int(n))))

    def alloc_step(self, sides=False):
        """One move, waited for; its diagnostics as a dict (labels 1-based).  `sides=True` adds "side": one byte per row
        (BMM_EA_OUTSIDE = 255 for a row the move does not touch)."""
        s = _AllocStep()
        sd = None
        if sides:
            sd = _np.zeros(self.N, dtype=_np.uint8)
            s.side = sd.ctypes.data
        _capi.check(_capi.lib().bmm_chain_alloc_step(self._h, _C.byref(s)))
        out = {"kind": ("eject", "absorb")[s.kind], "labels": (int(s.j1), int(s.j2)), "accepted": bool(s.accepted),
               "k_before": int(s.k_before), "k_after": int(s.k_after), "pe_bits": int(s.pe_bits), "members": int(s.members),
               "n_before": (int(s.n_before[0]), int(s.n_before[1])), "n_after": (int(s.n_after[0]), int(s.n_after[1])),
               "log_prior": s.log_prior, "log_lik": s.log_lik, "log_q": s.log_q, "log_move": s.log_move, "log_u": s.log_u,
               "log_r": s.log_r, "sweep": int(s.sweep), "move": int(s.move)}
        if sides:
            out["side"] = sd
        return out

    def alloc_stats(self):
        out = (_C.c_int64 * 4)()
        _capi.check(_capi.lib().bmm_chain_alloc_stats(self._h, out))
        return dict(zip(_EA_FIELDS, (int(v) for v in out)))

    # -- split-merge moves of the allocation sampler (include/bmm_mcmc.h)
    def set_alloc_split_merge(self, moves_per_sweep, scans=SPLIT_MERGE_SCANS):
        """`moves_per_sweep` moves at the start of every sweep from the second, behind its eject / absorb moves (0: off;
        the scans of the manual moves are still set), `scans` intermediate scans each.  An armed allocation chain only."""
        _capi.check(_capi.lib().bmm_chain_set_alloc_split_merge(self._h, _C.c_int(int(moves_per_sweep)), _C.c_int(int(scans))))

    def alloc_split_merge(self, n):
        """n moves now, enqueued behind whatever the chain is doing."""
        _capi.check(_capi.lib().bmm_chain_alloc_split_merge(self._h, _C.c_int(int(n))))

    def alloc_split_merge_step(self, sides=False):
        """One move, waited for; its diagnostics as a dict (labels 1-based, rows 0-based; "moved": the label a committed
        merge moved into the gap, or -1).  `sides=True` adds "launch_side" and "proposal_side" as split_merge_step."""
        s = _AllocSplitStep()
        la = pr = None
        if sides:
            la, pr = _np.zeros(self.N, dtype=_np.uint8), _np.zeros(self.N, dtype=_np.uint8)
            s.launch_side, s.proposal_side = la.ctypes.data, pr.ctypes.data
        _capi.check(_capi.lib().bmm_chain_alloc_split_merge_step(self._h, _C.byref(s)))
        out = {"rows": (int(s.row_i), int(s.row_j)), "labels": (int(s.label_a), int(s.label_b)),
               "kind": ("split", "merge", "skipped")[s.kind], "accepted": bool(s.accepted), "k_before": int(s.k_before),
               "k_after": int(s.k_after), "moved": int(s.moved), "members": int(s.members),
               "n_before": (int(s.n_before[0]), int(s.n_before[1])), "n_after": (int(s.n_after[0]), int(s.n_after[1])),
               "log_prior": s.log_prior, "log_lik": s.log_lik, "log_q": s.log_q, "log_u": s.log_u, "log_r": s.log_r,
               "sweep": int(s.sweep), "move": int(s.move)}
        if sides:
            out["launch_side"], out["proposal_side"] = la, pr
        return out

    def alloc_split_merge_stats(self):
        out = (_C.c_int64 * 5)()
        _capi.check(_capi.lib().bmm_chain_alloc_split_merge_stats(self._h, out))
        return dict(zip(_AS_FIELDS, (int(v) for v in out)))

    def set_labels(self, z1):
        """Replace the allocation of a seated DP chain between sweeps (1-based labels); Nk and S are recounted."""
        z1 = _np.ascontiguousarray(z1, dtype=_np.int32)
        if z1.shape != (self.N,):
            raise ValueError("one label per observation")
        _capi.check(_capi.lib().bmm_chain_set_labels(self._h, _capi.vp(z1)))

    # -- feature selection (include/bmm_mcmc.h "feature selection")
    def init_labels(self, kind="kmodes", centres=None, iters=INIT_ITERS):
        """The k-modes++ start on the device (include/bmm_mcmc.h "initial allocation"): the initial labels of a collapsed
        chain that has its data and has not started, or a new allocation of a seated DP chain between sweeps (`centres`
        must be given there; default K for the collapsed sampler).  Returns the record {"k_eff", "rounds_run",
        "changed_last", "cost", "device_ms"} with "rows" (the picked rows, 0-based), "centres" (k_eff x P, 0/1) and "Nk"
        (k_eff)."""
        if kind not in INIT_KINDS:
            raise ValueError('kind must be "kmodes"')
        info = _InitInfo()
        L = _capi.lib()
        _capi.check(L.bmm_chain_init_labels(self._h, _C.c_int(INIT_KINDS[kind]), _C.c_int(0 if centres is None else int(centres)),
                                            _C.c_int(int(iters)), _C.byref(info)))
        out = info.as_dict()
        ke, W = out["k_eff"], (self.P + 31) // 32
        words = _np.zeros((ke, W), dtype=_np.uint32)
        rows, nk = _np.zeros(ke, dtype=_np.int64), _np.zeros(ke, dtype=_np.int32)
        _capi.check(L.bmm_chain_get_init_centres(self._h, _capi.vp(words)))
        _capi.check(L.bmm_chain_get_init_rows(self._h, _capi.vp(rows), _capi.vp(nk)))
        bits = (words[:, :, None] >> _np.arange(32, dtype=_np.uint32)[None, None, :]) & _np.uint32(1)
        out.update(rows=rows, Nk=nk, centres=bits.reshape(ke, W * 32)[:, :self.P].astype(_np.uint8))
        return out

    def set_feature_select(self, on=True, rho=0.5):
        """a gamma-step behind every sweep from now on (on=False: no more steps, the mask stays)"""
        _capi.check(_capi.lib().bmm_chain_set_feature_select(self._h, _C.c_int(1 if on else 0), _C.c_double(float(rho))))

    def set_categorical(self, levels=None):
        """the levels of the chain's features (bmm_chain_set_categorical): the raw vector, one entry per feature -- 1: a
        binary feature in one column under Beta(beta, gamma); L >= 2: a block of L neighbouring one-hot columns under a
        symmetric Dirichlet(beta, ..., beta), blocks of 2 included -- whose columns add up to P.  Before or after the
        data, before the first sweep or between sweeps; when levels and data meet the device checks that every row has
        exactly one 1 in every block (BmmError names the first bad row and its feature).  None or an empty vector
        withdraws the levels.  Returns the number of features."""
        lv = _np.ascontiguousarray(() if levels is None else levels, dtype=_np.int32)
        if lv.ndim != 1:
            raise ValueError("levels is a vector with one entry per feature")
        _capi.check(_capi.lib().bmm_chain_set_categorical(self._h, _capi.vp(lv), _C.c_int(lv.size)))
        return int(lv.size)

    def categorical(self):
        """the levels the chain carries (an empty vector: none)"""
        F = _C.c_int(0)
        _capi.check(_capi.lib().bmm_chain_get_categorical(self._h, None, _C.byref(F)))
        lv = _np.zeros(F.value, dtype=_np.int32)
        if F.value:
            _capi.check(_capi.lib().bmm_chain_get_categorical(self._h, _capi.vp(lv), _C.byref(F)))
        return lv

    def set_features(self, gamma):
        """the inclusion mask, between sweeps: P values in {0, 1}"""
        g = _np.ascontiguousarray(gamma)
        if g.shape != (self.P,):
            raise ValueError("one indicator per feature")
        if not _np.all((g == 0) | (g == 1)):
            raise ValueError("indicators are 0 or 1")
        g = g.astype(_np.uint8)
        _capi.check(_capi.lib().bmm_chain_set_features(self._h, _capi.vp(g)))

    def features(self):
        g = _np.zeros(self.P, dtype=_np.uint8)
        _capi.check(_capi.lib().bmm_chain_get_features(self._h, _capi.vp(g)))
        return g

    def feature_step(self):
        """the last gamma-step: {"lambda", "p", "u", "gamma", "sweep"}"""
        lam, pr, u = _np.zeros(self.P), _np.zeros(self.P), _np.zeros(self.P)
        g = _np.zeros(self.P, dtype=_np.uint8)
        s = _FeatureStep(_capi.vp(lam), _capi.vp(pr), _capi.vp(u), _capi.vp(g), 0)
        _capi.check(_capi.lib().bmm_chain_feature_step(self._h, _C.byref(s)))
        return {"lambda": lam, "p": pr, "u": u, "gamma": g, "sweep": int(s.sweep)}

    def sweeps_features(self, n):
        """n more sweeps of an armed chain; returns the (n, P) indicators after each"""
        out = _np.zeros((int(n), self.P), dtype=_np.uint8)
        _capi.check(_capi.lib().bmm_chain_sweeps_features(self._h, _C.c_int(int(n)), _capi.vp(out)))
        return out

    def feature_summary(self):
        inc, rb, n = _np.zeros(self.P), _np.zeros(self.P), _C.c_int(0)
        _capi.check(_capi.lib().bmm_chain_get_feature_summary(self._h, _capi.vp(inc), _capi.vp(rb), _C.byref(n)))
        return {"inclusion": inc, "inclusion_rb": rb, "n_folded": n.value}

    def feature_reset(self):
        _capi.check(_capi.lib().bmm_chain_feature_reset(self._h))

    def set_missing(self, rows=None, cols=None, mask=None):
        """declare the missing cells (bmm_chain_set_missing): `mask`, a boolean N x P matrix, or `rows` / `cols`, 0-based
        and strictly ascending in (row, column); nothing, or empty lists, withdraws the declaration.  Returns the
        number of cells."""
        if mask is not None:
            rows, cols = _np.nonzero(_np.asarray(mask, dtype=bool))
        rows = _np.ascontiguousarray(() if rows is None else rows, dtype=_np.int64)
        cols = _np.ascontiguousarray(() if cols is None else cols, dtype=_np.int32)
        if rows.shape != cols.shape or rows.ndim != 1:
            raise ValueError("rows and cols must be two lists of one length")
        _capi.check(_capi.lib().bmm_chain_set_missing(self._h, _capi.vp(rows), _capi.vp(cols), _C.c_int64(rows.size)))
        self._na_cells = int(rows.size)
        return self._na_cells

    def impute_step(self):
        """one imputation step now, under the index of the last sweep (bmm_chain_impute_step)"""
        _capi.check(_capi.lib().bmm_chain_impute_step(self._h))

    def missing_state(self):
        """the declared cells' current values, uint8, in the order declared"""
        bits = _np.zeros(getattr(self, "_na_cells", 0), dtype=_np.uint8)
        _capi.check(_capi.lib().bmm_chain_get_missing_state(self._h, _capi.vp(bits)))
        return bits

    def missing_summary(self):
        """{"mean", "mean_draw" (n_cells,), "n_folded"} over the steps folded so far"""
        n = getattr(self, "_na_cells", 0)
        rb, dr, nf = _np.zeros(n), _np.zeros(n), _C.c_int64(0)
        _capi.check(_capi.lib().bmm_chain_get_missing_summary(self._h, _capi.vp(rb), _capi.vp(dr), _C.byref(nf)))
        return {"mean": rb, "mean_draw": dr, "n_folded": int(nf.value)}

    def missing_reset(self):
        _capi.check(_capi.lib().bmm_chain_missing_reset(self._h))

    # -- constrained allocations (include/bmm_mcmc.h "constraints")
    def set_constraints(self, rows=None, masks=None):
        """the constrained rows (bmm_chain_set_constraints): `rows` 0-based and strictly ascending, `masks` their allowed
        labels as 64-bit masks (bit k: label k + 1 of labels()); nothing, or empty lists, withdraws them.  Returns the
        number of rows."""
        rows = _np.ascontiguousarray(() if rows is None else rows, dtype=_np.int64)
        masks = _np.ascontiguousarray(() if masks is None else masks, dtype=_np.uint64)
        if rows.shape != masks.shape or rows.ndim != 1:
            raise ValueError("rows and masks must be two lists of one length")
        _capi.check(_capi.lib().bmm_chain_set_constraints(self._h, _C.c_int64(rows.size), _capi.vp(rows), _capi.vp(masks)))
        self._cs = (rows, masks)
        return int(rows.size)

    def set_known(self, z):
        """the rows' known labels: N integers, 0, a negative value or NaN for a free row, else the 1-based label"""
        rows, masks, _ = _capi.constraint_list(self.N, self.K, known=z)
        return self.set_constraints(rows, masks)

    def constraint_stats(self):
        """{"rows", "n_rows", "n_known", "proposed", "reverted", "rate"} since the constraints were set"""
        pr, rv = _C.c_int64(0), _C.c_int64(0)
        _capi.check(_capi.lib().bmm_chain_constraint_stats(self._h, _C.byref(pr), _C.byref(rv)))
        rows, masks = getattr(self, "_cs", (_np.zeros(0, dtype=_np.int64), _np.zeros(0, dtype=_np.uint64)))
        return _constraint_result(rows, masks, pr.value, rv.value)

    def profile(self, every=1):
        """Time the resample launches of every `every`-th sweep with HIP events (0/False: off)."""
        _capi.check(_capi.lib().bmm_chain_profile(self._h, _C.c_int(int(every))))

    def profile_read(self):
        ms, n = _C.c_double(0.0), _C.c_int64(0)
        _capi.check(_capi.lib().bmm_chain_profile_read(self._h, _C.byref(ms), _C.byref(n)))
        return ms.value, n.value

    def kernel_shape(self):
        lds, th, g = _C.c_int(0), _C.c_int(0), _C.c_int(0)
        _capi.check(_capi.lib().bmm_chain_kernel_shape(self._h, _C.byref(lds), _C.byref(th), _C.byref(g)))
        lanes, own = _C.c_int(0), _C.c_int(0)
        _capi.check(_capi.lib().bmm_chain_kernel_form(self._h, _C.byref(lanes), _C.byref(own)))
        return {"lds_bytes": lds.value, "threads": th.value, "grid_max": g.value,
                "lanes_per_observation": lanes.value, "builds_own_tables": bool(own.value)}


def sweep_chains(chains, n):
    """n more sweeps of every chain in `chains`, one host thread per chain (bmm_chains_sweeps): chains on
    one device overlap on their streams.  Returns without waiting; sync each chain afterwards."""
    tab = (_C.c_void_p * len(chains))(*[c._h.value for c in chains])
    _capi.check(_capi.lib().bmm_chains_sweeps(tab, _C.c_int(len(chains)), _C.c_int(int(n))))


class _ExchangeStep(_C.Structure):  # bmm_exchange_step
    _fields_ = [("d", _C.c_double), ("u", _C.c_double), ("proposed", _C.c_int32), ("accepted", _C.c_int32),
                ("point", _C.c_int32), ("pad", _C.c_int32)]


class Ladder:
    """A replica ladder over resident chains (bmm_ladder_* in include/bmm_mcmc.h): chains[0] at
    inverse temperature 1, the others armed with set_temper at strictly decreasing powers, all over one copy of the data
    (share_data) on one device.  The chains stay the caller's and must outlive the ladder."""

    def __init__(self, chains, seed=0):
        self._h = _C.c_void_p()
        self.chains = list(chains)
        self.R = len(self.chains)
        tab = (_C.c_void_p * self.R)(*[c._h.value for c in self.chains])
        _capi.check(_capi.lib().bmm_ladder_create(_C.byref(self._h), tab, _C.c_int(self.R), _C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)))

    def close(self):
        if self._h:
            _capi.lib().bmm_ladder_destroy(self._h)
            self._h = _C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sweeps(self, n, swap_every=1):
        """n sweeps of every rung, an exchange point behind every sweep whose index is a multiple of swap_every.
        Returns without waiting."""
        _capi.check(_capi.lib().bmm_ladder_sweeps(self._h, _C.c_int(int(n)), _C.c_int(int(swap_every))))

    def exchange_step(self):
        """One exchange point now, waited for: a list of R - 1 records {"d", "u", "proposed", "accepted", "point"}."""
        rec = (_ExchangeStep * max(self.R - 1, 1))()
        _capi.check(_capi.lib().bmm_ladder_exchange_step(self._h, rec))
        return [{"d": rec[r].d, "u": rec[r].u, "proposed": bool(rec[r].proposed), "accepted": bool(rec[r].accepted),
                 "point": int(rec[r].point)} for r in range(self.R - 1)]

    def stats(self):
        """{"proposed", "accepted": (R - 1,), "walker": (R,)}: the exchanges per neighbouring pair and which starting
        rung's state sits at each rung now."""
        pr, ac = _np.zeros(max(self.R - 1, 1), dtype=_np.int64), _np.zeros(max(self.R - 1, 1), dtype=_np.int64)
        w = _np.zeros(self.R, dtype=_np.int32)
        _capi.check(_capi.lib().bmm_ladder_stats(self._h, _capi.vp(pr), _capi.vp(ac), _capi.vp(w)))
        return {"proposed": pr[:self.R - 1], "accepted": ac[:self.R - 1], "walker": w}


def broadcast_planes(chains):
    """Resident chains on different devices of this process, one per device: chains[0] holds the data, the
    others receive its bit planes with one RCCL broadcast (bmm_chains_broadcast_planes)."""
    tab = (_C.c_void_p * len(chains))(*[c._h.value for c in chains])
    _capi.check(_capi.lib().bmm_chains_broadcast_planes(tab, _C.c_int(len(chains))))


def chain_summary(obj, cluster_threshold=0.1):
    """The numbers `plot_gibbs` draws from a returned chain object (R/utils.R:147-190), without the plots:
    `proportions` S x K, the share of the observations holding each label in each kept sample (labels that
    are NA -- the DP and explicit samplers' row 0 at burnin = 0 -- do not count); `clusters`, the 1-based
    labels that exceed `cluster_threshold` in some sample after the first (plot_gibbs drops sample 1), in
    order of first appearance; `theta` K x P x S restricted to those labels (others NaN), as the theta
    panel shows it."""
    z = _np.asarray(obj["z"])
    th = _np.asarray(obj["theta"], dtype=_np.float64)
    K = th.shape[0]
    S, N = z.shape
    props = _np.zeros((S, K))
    for s in range(S):
        lab = z[s]
        lab = lab[(lab >= 1) & (lab <= K)]
        if lab.size:
            props[s] = _np.bincount(lab - 1, minlength=K) / lab.size
    clusters = []
    for s in range(1, S):
        for k in _np.nonzero(props[s] > cluster_threshold)[0]:
            if k + 1 not in clusters:
                clusters.append(int(k) + 1)
    shown = _np.full_like(th, _np.nan)
    for k in clusters:
        shown[k - 1] = th[k - 1]
    return {"proportions": props, "clusters": clusters, "theta": shown}


# ---------------------------------------------------------------- an ensemble of exact chains
_ENSEMBLE_SAMPLERS = ("collapsed", "dp")


def ensemble_plan(sampler, N, P, K, chains=64):
    """What bmm_ensemble_plan reports of an ensemble of `chains` exact chains of that shape (K: K, or maxK for "dp"),
    without touching a device: {"group_width", "lds_bytes_per_chain", "chains_per_workgroup", "workgroups",
    "launches_per_sweep", "state_bytes", "bytes_per_kept_sweep", "label_bytes_per_kept_sweep"}.  A shape that does not
    fit -- more than 64 categories, P > 128, N >= 65536, terms beyond the LDS of a workgroup -- raises BmmError
    (BMM_E_UNSUPPORTED)."""
    if sampler not in _capi.SAMPLER_CODE:
        raise ValueError("unknown sampler %r" % (sampler,))
    out = _np.zeros(8, dtype=_np.int64)
    _capi.check(_capi.lib().bmm_ensemble_plan(_C.c_int(_capi.SAMPLER_CODE[sampler]), _C.c_int64(N), _C.c_int(P), _C.c_int(K),
                                              _C.c_int(chains), _capi.vp(out)))
    keys = ("group_width", "lds_bytes_per_chain", "chains_per_workgroup", "workgroups", "launches_per_sweep", "state_bytes",
            "bytes_per_kept_sweep", "label_bytes_per_kept_sweep")
    return {k: int(v) for k, v in zip(keys, out)}


def _ensemble_run(*args):
    return _capi.lib().bmm_ensemble_run(*args)


class _EnsembleFolds(_C.Structure):  # bmm_ensemble_folds
    _fields_ = [("newdata", _C.c_void_p), ("M", _C.c_int64), ("loo", _C.c_int32), ("loo_trace", _C.c_int32),
                ("predictive_trace", _C.c_int32), ("pred_lppd", _C.c_void_p), ("pred_logdens", _C.c_void_p),
                ("loo_log_cpo", _C.c_void_p), ("loo_ess", _C.c_void_p), ("loo_lppd", _C.c_void_p), ("loo_mean", _C.c_void_p),
                ("loo_var", _C.c_void_p), ("loo_ell", _C.c_void_p), ("loo_lpml", _C.c_void_p), ("loo_min_ess", _C.c_void_p),
                ("n_folded", _C.c_void_p)]


def ensemble_fold_plan(sampler, N, P, K, chains=64, M=0, loo=False):
    """What bmm_ensemble_fold_plan reports of the folds of an ensemble, without touching a device:
    {"lds_bytes_per_chain", "chains_per_workgroup", "accumulator_bytes", "ell_bytes_per_kept_sweep",
    "logdens_bytes_per_kept_sweep", "launches_per_kept_sweep"}; M: the new rows (0: no newdata=).  The shapes ensemble_plan
    refuses are refused here."""
    if sampler not in _capi.SAMPLER_CODE:
        raise ValueError("unknown sampler %r" % (sampler,))
    out = _np.zeros(6, dtype=_np.int64)
    _capi.check(_capi.lib().bmm_ensemble_fold_plan(_C.c_int(_capi.SAMPLER_CODE[sampler]), _C.c_int64(N), _C.c_int(P), _C.c_int(K),
                                                   _C.c_int(chains), _C.c_int64(M), _C.c_int(1 if loo else 0), _capi.vp(out)))
    keys = ("lds_bytes_per_chain", "chains_per_workgroup", "accumulator_bytes", "ell_bytes_per_kept_sweep",
            "logdens_bytes_per_kept_sweep", "launches_per_kept_sweep")
    return {k: int(v) for k, v in zip(keys, out)}


def _ensemble_run_ex(*args):
    return _capi.lib().bmm_ensemble_run_ex(*args)


def _logsumexp(v):
    v = _np.asarray(v, dtype=_np.float64)
    m = _np.max(v, axis=0)
    m = _np.where(_np.isfinite(m), m, 0.0)
    with _np.errstate(divide="ignore"):
        return m + _np.log(_np.sum(_np.exp(v - m), axis=0))


def ensemble_pool(outs):
    """The leave-one-out and predictive summaries of the chains of gibbs_ensemble(..., loo=..., newdata=...) pooled over
    chains, on the host, from the per-chain results alone.  With n_c = chain c's n_folded:
      loo         A_c = log n_c - log_cpo_c; log_cpo = log(sum n_c) - logsumexp_c A_c; B_c = 2 A_c - log ess_c;
                  ess = exp(2 logsumexp_c A_c - logsumexp_c B_c); lppd = logsumexp_c(log n_c + lppd_c) - log(sum n_c):
                  what one summary over the concatenated states would give.  {"log_cpo", "ess", "lppd", "lpml" (sum of
                  log_cpo), "min_ess", "n_folded", "lpml_chains" (per chain), "lpml_sd" (their standard deviation, ddof = 1)}
      predictive  {"lppd" (pooled as above), "n_folded", "lppd_chains" (chain c's lppd summed over the new rows)}
    Returns a dict with the key of every summary all chains carry."""
    outs = list(outs)
    if not outs:
        raise ValueError("ensemble_pool: no chain")
    res = {}
    if all("loo" in o for o in outs):
        n = _np.array([float(o["loo"]["n_folded"]) for o in outs])
        if _np.any(n < 1):
            raise ValueError("ensemble_pool: a chain has folded no state")
        ln = _np.log(n)[:, None]
        lt = _np.log(n.sum())
        A = ln - _np.stack([_np.asarray(o["loo"]["log_cpo"], dtype=_np.float64) for o in outs])
        lA = _logsumexp(A)
        B = 2.0 * A - _np.log(_np.stack([_np.asarray(o["loo"]["ess"], dtype=_np.float64) for o in outs]))
        lp = _logsumexp(ln + _np.stack([_np.asarray(o["loo"]["lppd"], dtype=_np.float64) for o in outs])) - lt
        log_cpo = lt - lA
        ess = _np.exp(2.0 * lA - _logsumexp(B))
        lc = _np.array([float(o["loo"]["lpml"]) for o in outs])
        res["loo"] = {"log_cpo": log_cpo, "ess": ess, "lppd": lp, "lpml": float(log_cpo.sum()), "min_ess": float(ess.min()),
                      "n_folded": int(n.sum()), "lpml_chains": lc,
                      "lpml_sd": float(_np.std(lc, ddof=1)) if lc.size > 1 else float("nan")}
    if all("predictive" in o for o in outs):
        n = _np.array([float(o["predictive"]["n_folded"]) for o in outs])
        if _np.any(n < 1):
            raise ValueError("ensemble_pool: a chain has folded no state")
        L = _np.stack([_np.asarray(o["predictive"]["lppd"], dtype=_np.float64) for o in outs])
        res["predictive"] = {"lppd": _logsumexp(_np.log(n)[:, None] + L) - _np.log(n.sum()), "n_folded": int(n.sum()),
                             "lppd_chains": L.sum(axis=1)}
    if not res:
        raise ValueError("ensemble_pool: the chains carry neither \"loo\" nor \"predictive\"")
    return res


def gibbs_ensemble(data, nsamples, K, sampler="collapsed", chains=64, alpha=None, beta=0.5, gamma=0.5, a=1, b=1, burnin=None,
                   seed=None, initial_K=None, keep_trace=True, device=0, newdata=None, predictive_trace=False, loo=False):
    """`chains` independent exact chains -- batch = 1, the reference's sequential scan -- of gibbs_collapsed
    (sampler="collapsed") or gibbs_dp (sampler="dp"; K is maxK) over one data set, one wavefront per chain, all of them
    advanced by one kernel launch per sweep.  For small data (N < 65536, P <= 128, at most 64 categories: ensemble_plan),
    where a single batch = 1 chain costs two launches per observation.  Chain c draws under seed + c and starts as
    chains= starts it: from numpy.random.default_rng(seed + c).integers(1, K + 1, N) unless `initial_K` lists one start
    per chain ("collapsed" only), so it is, bit for bit, the chain gibbs_collapsed(..., batch=1, seed=seed + c) runs.
    Returns a list of dicts {"alpha" (S, 1), "permutations", "z" (S, N) or None with keep_trace=False, "theta" (K, P, S),
    "sizes" (S, K), "z_last" (N,)}.  The traces go to the stand-alone tools (rhat, ess, partition_distances, ecr_relabel).
    Two of the run options are offered, scored on every chain by its own wavefront after each kept sweep (DESIGN.md section
    32): `newdata` (M >= 1 complete rows; `predictive_trace=True` adds the (S, M) trace) gives chain c
    "predictive" = {"lppd", ["logdens"], "n_folded"}, and `loo` (True or "trace") gives it "loo" = {"log_cpo", "ess", "lppd",
    "mean", "var", "lpml", "min_ess", "n_folded", ["ell"]}: the keys, meanings and bits of gibbs_collapsed / gibbs_dp(...,
    batch=1, seed=seed + c, newdata=..., loo=...).  Mean responsibilities are not offered (labels switch between chains);
    ensemble_pool pools the summaries over chains."""
    if sampler not in _ENSEMBLE_SAMPLERS:
        raise ValueError('gibbs_ensemble: sampler must be "collapsed" or "dp"')
    if _categorical_of(data) is not None:
        raise ValueError("gibbs_ensemble: categorical features are not offered")
    X = _capi.as_x(data)
    N, P = X.shape
    nsamples, K, chains = int(nsamples), int(K), int(chains)
    if chains < 1:
        raise ValueError("gibbs_ensemble: chains must be >= 1")
    dp = sampler == "dp"
    if dp and beta != gamma:
        raise ValueError("gibbs_ensemble: the DP sampler needs beta == gamma")
    if dp and initial_K is not None:
        raise ValueError("gibbs_ensemble: a DP chain seats its rows in its first sweep: no initial_K")
    burnin = _burnin(burnin, nsamples)
    seed = _seed(seed)
    if loo is not True and loo is not False and loo is not None and not (isinstance(loo, str) and loo == "trace"):
        raise ValueError('gibbs_ensemble: loo must be True, "trace" or False')
    Xn = None
    if newdata is not None:
        Xn = _capi.as_x(newdata)
        if Xn.ndim != 2 or Xn.shape[1] != P:
            raise ValueError("gibbs_ensemble: newdata must have the %d columns of data" % P)
        if Xn.shape[0] < 1:
            raise ValueError("gibbs_ensemble: newdata has no rows")
    elif predictive_trace:
        raise ValueError("gibbs_ensemble: predictive_trace needs newdata")
    folds = bool(loo) or Xn is not None
    ensemble_plan(sampler, N, P, K, chains)  # the limits, by name
    z0s = None
    if not dp:
        if initial_K is None:
            z0s = [_np.ascontiguousarray(_np.random.default_rng(seed + c).integers(1, K + 1, N), dtype=_np.int32) for c in range(chains)]
        else:
            z0s = [_np.ascontiguousarray(z, dtype=_np.int32) for z in initial_K]
            if len(z0s) != chains:
                raise ValueError("gibbs_ensemble: initial_K must list one start per chain (%d given, %d chains)" % (len(z0s), chains))
            if any(z.shape != (N,) for z in z0s):
                raise ValueError("gibbs_ensemble: every start in initial_K must have one label per observation")
    S = nsamples - burnin
    zs = [_np.empty((S, N), dtype=_np.int32, order="F") for _ in range(chains)] if keep_trace else None
    nks = [_np.zeros((S, K), dtype=_np.int32) for _ in range(chains)]
    ths = [_np.zeros((K, P, S), order="F") for _ in range(chains)]
    als = [_np.zeros((S, 1), order="F") for _ in range(chains)]
    zl = [_np.zeros(N, dtype=_np.int32) for _ in range(chains)]
    args = (
        _C.c_int(_capi.SAMPLER_CODE[sampler]), _capi.vp(X), _C.c_int64(N), _C.c_int(P), _C.c_int(chains),
        _ptr_table(z0s) if z0s is not None else None, _C.c_int(nsamples), _C.c_int(K),
        _C.c_double(0.0 if alpha is None else alpha), _C.c_double(beta), _C.c_double(gamma), _C.c_double(a), _C.c_double(b),
        _C.c_int(burnin), _C.c_uint64(seed), _C.c_int(device), _ptr_table(zs) if keep_trace else None, _ptr_table(nks),
        _ptr_table(ths), _ptr_table(als), _ptr_table(zl))
    if not folds:
        _capi.check(_ensemble_run(*args))
    else:
        each = lambda shape, order="C": [_np.full(shape, _np.nan, order=order) for _ in range(chains)]  # noqa: E731
        M = 0 if Xn is None else Xn.shape[0]
        pl = each(M) if M else None
        pt = each((S, M), "F") if M and predictive_trace else None
        lrows = {k: each(N) for k in ("log_cpo", "ess", "lppd", "mean", "var")} if loo else None
        lt = each((S, N), "F") if loo == "trace" else None
        lpml, mess = _np.full(chains, _np.nan), _np.full(chains, _np.nan)
        nf = _C.c_int32(0)
        tables = {}

        def tab(key, arrays):
            if arrays is None:
                return None
            tables[key] = _ptr_table(arrays)
            return _C.cast(tables[key], _C.c_void_p)

        fs = _EnsembleFolds(
            Xn.ctypes.data if M else None, M, 1 if loo else 0, 1 if lt is not None else 0, 1 if pt is not None else 0,
            tab("pl", pl), tab("pt", pt), *[tab(k, lrows[k] if loo else None) for k in ("log_cpo", "ess", "lppd", "mean", "var")],
            tab("lt", lt), lpml.ctypes.data if loo else None, mess.ctypes.data if loo else None, _C.addressof(nf))
        _capi.check(_ensemble_run_ex(*args, _C.byref(fs)))
    outs = [{"alpha": als[c], "permutations": _na_perm(S, K), "z": zs[c] if keep_trace else None, "theta": ths[c],
             "sizes": nks[c], "z_last": zl[c]} for c in range(chains)]
    if folds:
        for c, o in enumerate(outs):
            if M:
                o["predictive"] = {"lppd": pl[c], "n_folded": int(nf.value)}
                if pt is not None:
                    o["predictive"]["logdens"] = pt[c]
            if loo:
                o["loo"] = {k: lrows[k][c] for k in ("log_cpo", "ess", "lppd", "mean", "var")}
                o["loo"].update(lpml=float(lpml[c]), min_ess=float(mess[c]), n_folded=int(nf.value))
                if lt is not None:
                    o["loo"]["ell"] = lt[c]
    return outs
