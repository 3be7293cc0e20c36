"""ctypes binding of include/bmm_mcmc.h.  There is no fallback: if the HIP library is
missing or no GPU is visible, calls raise."""
import ctypes as C
import os

import numpy as np

from . import build as _build

_LIB = None

SAMPLER_COLLAPSED, SAMPLER_DP, SAMPLER_SB, SAMPLER_FULL = 0, 1, 2, 3
SAMPLER_CODE = {"collapsed": 0, "dp": 1, "stickbreaking": 2, "full": 3}
NA_INTEGER = -2147483648

# every symbol include/bmm_mcmc.h declares
SYMBOLS = [
    "bmm_last_error", "bmm_spec_group_width", "bmm_spec_group_width_own", "bmm_spec_group_width_for", "bmm_spec_pk_image_bytes", "bmm_default_batch", "bmm_collapsed_run", "bmm_dp_run",
    "bmm_sb_run", "bmm_full_run", "bmm_chain_create", "bmm_chain_destroy", "bmm_chain_set_data_host",
    "bmm_chain_set_data_device", "bmm_chain_set_x_layout", "bmm_chain_get_x_layout", "bmm_chain_set_initial_labels", "bmm_chain_set_initial_params",
    "bmm_chain_sweeps", "bmm_chain_sweeps_counts", "bmm_chain_sweep_probs", "bmm_chain_set_shard", "bmm_chain_shard_resample",
    "bmm_chain_shard_deltas", "bmm_chain_shard_finish", "bmm_chain_sync", "bmm_chain_sweep_index", "bmm_chain_get_labels",
    "bmm_chain_get_counts", "bmm_chain_get_alpha", "bmm_chain_get_params", "bmm_chain_profile",
    "bmm_chain_profile_read", "bmm_chain_kernel_shape", "bmm_chain_kernel_form", "bmm_chain_batch", "bmm_device_math", "bmm_device_variates", "bmm_device_variates_ex",
    "bmm_device_count", "bmm_collapsed_run_probs", "bmm_dp_run_probs", "bmm_sb_run_probs", "bmm_full_run_probs",
    "bmm_multi_run", "bmm_multi_selfcheck", "bmm_chains_sweeps", "bmm_chain_share_data", "bmm_chain_planes",
    "bmm_chain_planes_filled", "bmm_chain_shard_resample_async", "bmm_chain_stream",
    "bmm_chains_broadcast_planes", "bmm_set_progress", "bmm_last_run_phases", "bmm_host_threads", "bmm_multi_plan", "bmm_release_pools",
    "bmm_collapsed_run_relabel", "bmm_dp_run_relabel", "bmm_sb_run_relabel", "bmm_full_run_relabel",
    "bmm_device_stephens_batch", "bmm_device_stephens_online", "bmm_device_stephens_plan",
    "bmm_chain_set_newdata_host", "bmm_chain_predict_responsibilities", "bmm_chain_predict_state",
    "bmm_chain_sweeps_predict", "bmm_chain_get_predictive", "bmm_chain_predict_reset",
    "bmm_collapsed_run_predict", "bmm_dp_run_predict", "bmm_sb_run_predict", "bmm_full_run_predict",
    "bmm_chain_set_newdata_missing", "bmm_chain_predict_state_cells", "bmm_chain_get_predictive_cells",
    "bmm_set_newdata_missing", "bmm_predict_na_plan",
    "bmm_device_partition_distances", "bmm_device_psm", "bmm_device_partition_plan", "bmm_set_partition_summary",
    "bmm_device_partition_search", "bmm_partition_search_plan", "bmm_set_partition_search",
    "bmm_device_credible_ball", "bmm_credible_ball_plan", "bmm_set_credible_ball",
    "bmm_chain_set_loo", "bmm_chain_loo_state", "bmm_chain_sweeps_loo", "bmm_chain_get_loo", "bmm_chain_loo_reset",
    "bmm_set_loo_summary",
    "bmm_chain_set_split_merge", "bmm_chain_split_merge", "bmm_chain_split_merge_step", "bmm_chain_split_merge_stats",
    "bmm_chain_set_labels", "bmm_set_split_merge", "bmm_last_split_merge_stats",
    "bmm_chain_set_feature_select", "bmm_chain_set_features", "bmm_chain_get_features", "bmm_chain_feature_step",
    "bmm_chain_sweeps_features", "bmm_chain_get_feature_summary", "bmm_chain_feature_reset", "bmm_set_feature_select",
    "bmm_chain_init_labels", "bmm_chain_get_init_centres", "bmm_chain_get_init_rows", "bmm_set_init", "bmm_last_init_info",
    "bmm_chain_set_alloc", "bmm_chain_set_k", "bmm_chain_get_k", "bmm_chain_alloc", "bmm_chain_alloc_step",
    "bmm_chain_alloc_stats", "bmm_alloc_run",
    "bmm_chain_set_alloc_split_merge", "bmm_chain_alloc_split_merge", "bmm_chain_alloc_split_merge_step",
    "bmm_chain_alloc_split_merge_stats", "bmm_set_alloc_split_merge", "bmm_last_alloc_split_merge_stats",
    "bmm_device_ecr", "bmm_device_ecr_plan", "bmm_set_ecr_relabel",
    "bmm_chain_set_logpost", "bmm_chain_logpost_state", "bmm_chain_sweeps_logpost", "bmm_chain_get_best",
    "bmm_chain_logpost_reset", "bmm_set_logpost", "bmm_device_log_joint",
    "bmm_chain_set_temper", "bmm_chain_get_temper", "bmm_ladder_create", "bmm_ladder_destroy", "bmm_ladder_sweeps",
    "bmm_ladder_exchange_step", "bmm_ladder_stats", "bmm_set_temper",
    "bmm_chain_set_pair_check", "bmm_chain_pair_check_state", "bmm_chain_sweeps_pair_check", "bmm_chain_get_pair_check",
    "bmm_chain_pair_check_reset", "bmm_chain_pair_counts", "bmm_set_pair_check", "bmm_device_pair_check", "bmm_pair_check_plan",
    "bmm_chain_set_missing", "bmm_chain_impute_step", "bmm_chain_get_missing_state", "bmm_chain_get_missing_summary",
    "bmm_chain_missing_reset", "bmm_set_missing",
    "bmm_chain_set_constraints", "bmm_chain_constraint_stats", "bmm_set_constraints", "bmm_last_constraint_stats",
    "bmm_set_summary", "bmm_run_bytes", "bmm_summary_plan", "bmm_chain_set_summary", "bmm_chain_summary_state",
    "bmm_chain_sweeps_summary", "bmm_chain_get_summary", "bmm_chain_summary_reset",
    "bmm_chain_set_categorical", "bmm_chain_get_categorical", "bmm_set_categorical", "bmm_categorical_plan",
    "bmm_ensemble_plan", "bmm_ensemble_run", "bmm_ensemble_fold_plan", "bmm_ensemble_run_ex",
]


class BmmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def lib_path():
    """The product library, unless BMM_LIB_PATH names another build of it (the -DBMM_DEBUG_HOOKS test
    variant, a diagnostic or experimental build): alternatives are loaded from their own path, the
    product file is never overwritten."""
    return os.environ.get("BMM_LIB_PATH") or _build.LIB


def load(path):
    """dlopen one build of the library and declare the non-int signatures."""
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc, gfx950). This package has no CPU fallback.")
    L = C.CDLL(path)
    L.bmm_last_error.restype = C.c_char_p
    L.bmm_default_batch.restype = C.c_int64
    L.bmm_default_batch.argtypes = [C.c_int, C.c_int64]
    L.bmm_chain_batch.restype = C.c_int64
    L.bmm_chain_batch.argtypes = [C.c_void_p]
    L.bmm_chain_destroy.restype = None
    L.bmm_chain_destroy.argtypes = [C.c_void_p]
    L.bmm_chain_share_data.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(L, "bmm_chain_set_pair_check"):  # (an older build loaded for a comparison has no pair check)
        L.bmm_chain_set_pair_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.bmm_chain_pair_check_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bmm_chain_sweeps_pair_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.bmm_chain_get_pair_check.argtypes = [C.c_void_p, C.c_void_p]
        L.bmm_chain_pair_check_reset.argtypes = [C.c_void_p]
        L.bmm_chain_pair_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "bmm_chain_set_missing"):  # (an older build loaded for a comparison has no missing data)
        L.bmm_chain_set_missing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        L.bmm_chain_impute_step.argtypes = [C.c_void_p]
        L.bmm_chain_get_missing_state.argtypes = [C.c_void_p, C.c_void_p]
        L.bmm_chain_get_missing_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bmm_chain_missing_reset.argtypes = [C.c_void_p]
        L.bmm_set_missing.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    if hasattr(L, "bmm_chain_set_newdata_missing"):  # (an older build loaded for a comparison has no incomplete new rows)
        L.bmm_chain_set_newdata_missing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        L.bmm_chain_predict_state_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bmm_chain_get_predictive_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bmm_set_newdata_missing.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.bmm_predict_na_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "bmm_chain_set_constraints"):  # (an older build loaded for a comparison has no constraints)
        L.bmm_chain_set_constraints.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.bmm_chain_constraint_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bmm_set_constraints.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
        L.bmm_last_constraint_stats.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(L, "bmm_set_summary"):  # (an older build loaded for a comparison has no summary)
        L.bmm_set_summary.argtypes = [C.c_void_p, C.c_void_p]
        L.bmm_run_bytes.restype = C.c_int64
        L.bmm_run_bytes.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.bmm_summary_plan.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_void_p]
        L.bmm_chain_set_summary.argtypes = [C.c_void_p, C.c_void_p]
        L.bmm_chain_summary_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bmm_chain_sweeps_summary.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.bmm_chain_get_summary.argtypes = [C.c_void_p, C.c_void_p]
        L.bmm_chain_summary_reset.argtypes = [C.c_void_p]
    if hasattr(L, "bmm_chain_set_categorical"):  # (an older build loaded for a comparison has no categorical features)
        L.bmm_chain_set_categorical.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.bmm_chain_get_categorical.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bmm_set_categorical.argtypes = [C.c_void_p, C.c_int]
        L.bmm_categorical_plan.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
    if hasattr(L, "bmm_ensemble_run"):  # (an older build loaded for a comparison has no ensemble)
        L.bmm_ensemble_plan.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.bmm_ensemble_run.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                       C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_uint64, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "bmm_ensemble_run_ex"):  # (an older build loaded for a comparison has no folds on ensemble chains)
        L.bmm_ensemble_fold_plan.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p]
        L.bmm_ensemble_run_ex.argtypes = L.bmm_ensemble_run.argtypes + [C.c_void_p]
    if hasattr(L, "bmm_ladder_create"):  # (an older build loaded for a comparison has no ladder)
        L.bmm_ladder_destroy.restype = None
        L.bmm_ladder_destroy.argtypes = [C.c_void_p]
        L.bmm_ladder_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64]
        L.bmm_ladder_sweeps.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.bmm_ladder_exchange_step.argtypes = [C.c_void_p, C.c_void_p]
        L.bmm_ladder_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def lib():
    global _LIB
    if _LIB is None:
        _LIB = load(lib_path())
    return _LIB


def check(rc):
    if rc != 0:
        raise BmmError(rc, lib().bmm_last_error().decode())


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def device_count():
    n = C.c_int(0)
    lib().bmm_device_count(C.byref(n))
    return n.value


def as_x(data):
    """N x P integer matrix in R's layout (column-major int32).  That the values are 0/1 is checked by the
    library when the matrix is handed over (in the same pass that packs it): a second pass here would cost
    as much as 100 sweeps at the north-star shape."""
    X = np.asarray(data)
    if X.ndim != 2:
        raise ValueError("data must be a matrix with observations in rows")
    if X.dtype.kind == "f":
        if not np.all(X == np.round(X)):
            raise ValueError("data must be integer valued")
    elif X.dtype.kind not in "iub":
        raise ValueError("data must be an integer (0/1) matrix")
    if X.dtype != np.int32 and X.size and (X.min() < 0 or X.max() > 1):
        raise ValueError("data must be binary (0/1)")  # before a narrowing cast could hide it
    return np.asfortranarray(X, dtype=np.int32)


def missing_cells(data, missing):
    """The cells `missing=` names and the matrix without them: (rows int64, cols int32, cleaned data), the cells sorted
    by (row, column).  "na": the NA_INTEGER cells of an integer matrix, the NaN cells of a floating-point one; or a
    boolean N x P mask.  The named cells are zeroed so that the matrix passes as_x, which goes on refusing NA."""
    X = np.asarray(data)
    if X.ndim != 2:
        raise ValueError("data must be a matrix with observations in rows")
    if isinstance(missing, str):
        if missing != "na":
            raise ValueError('missing must be None, "na" or a boolean N x P mask')
        if X.dtype.kind == "f":
            mask = np.isnan(X)
        elif X.dtype.kind == "i" and X.dtype.itemsize >= 4:
            mask = X == NA_INTEGER
        else:
            mask = np.zeros(X.shape, dtype=bool)
    else:
        mask = np.asarray(missing)
        if mask.dtype != np.bool_ or mask.shape != X.shape:
            raise ValueError('missing must be None, "na" or a boolean N x P mask')
    rows, cols = np.nonzero(mask)  # row-major order: sorted by (row, column)
    if rows.size:
        X = X.copy()
        X[mask] = 0
    return np.ascontiguousarray(rows, dtype=np.int64), np.ascontiguousarray(cols, dtype=np.int32), X


def constraint_list(N, K, known=None, allowed=None):
    """The sorted list `known=` and `allowed=` name: (rows int64, masks uint64, n_known).  known: N integers, 0, a negative
    value or NaN marks a free row, any other value is the row's 1-based label.  allowed: an N x K boolean array, a row
    that is all True is free.  Where both constrain a row they must agree: the known label must be allowed, and the row is
    held there.  Labels above 64 cannot be named (the masks are 64 bits wide)."""
    mask = np.zeros(N, dtype=np.uint64)
    listed = np.zeros(N, dtype=bool)
    if allowed is not None:
        A = np.asarray(allowed)
        if A.dtype != np.bool_ or A.shape != (N, K):
            raise ValueError("allowed must be a boolean N x K array")
        if K > 64:
            raise ValueError("allowed= names labels up to 64: K = %d" % K)
        if not A.any(axis=1).all():
            raise ValueError("allowed: row %d has no allowed label" % int(np.flatnonzero(~A.any(axis=1))[0]))
        listed = ~A.all(axis=1)
        mask = (A.astype(np.uint64) << np.arange(K, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    held = np.zeros(N, dtype=bool)
    if known is not None:
        kn = np.asarray(known)
        if kn.shape != (N,) or kn.dtype.kind not in "iuf":
            raise ValueError("known must hold one number per observation")
        if kn.dtype.kind == "f":
            kn = np.where(np.isnan(kn), 0.0, kn)
            if not np.all(kn == np.round(kn)):
                raise ValueError("known must be integer valued")
        kn = kn.astype(np.int64)
        held = kn > 0
        if held.any() and kn[held].max() > min(K, 64):
            raise ValueError("known: label %d lies above %s" % (int(kn[held].max()), "K = %d" % K if K <= 64 else "64, the widest mask"))
        bit = np.zeros(N, dtype=np.uint64)
        bit[held] = np.uint64(1) << (kn[held] - 1).astype(np.uint64)
        clash = held & listed & ((mask & bit) == 0)
        if clash.any():
            raise ValueError("known and allowed disagree on row %d" % int(np.flatnonzero(clash)[0]))
        mask = np.where(held, bit, mask)
        listed = listed | held
    rows = np.flatnonzero(listed).astype(np.int64)
    return np.ascontiguousarray(rows), np.ascontiguousarray(mask[rows], dtype=np.uint64), int(held.sum())
