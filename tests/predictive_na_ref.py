"""NumPy restatement of the predictive of INCOMPLETE new rows (include/bmm_mcmc.h "incomplete new rows", DESIGN.md
section 28), written with np.log and np.logaddexp only -- nothing of the library's arithmetic (no split tables, no
max-shift by hand, no table exponential).  The device kernels (csrc/kernels.hip.h, k_split_tables / k_score_na /
k_score_na_generic / k_predict_cells_finish) compute the same quantities; the tests hold them to each other.

A new row x has observed cells O and missing cells U (`miss`, a boolean M x P mask; the values of X in the missing
cells are ignored).  For a state s the log category terms are those of predictive_ref with the product over d in O:

  terms[m, k]     log w_k + sum_{d in O} log t_kd(x_d)
  logdens[m]      log p(x_O | s) = logaddexp over k of terms[m, k]
  cell joint      log q_md = log p(x_O, x_d = 1 | s) = logaddexp over k of (terms[m, k] + log t_kd(1)), (m, d) missing
  cell_state      q_md / p(x_O | s) = P(x_d = 1 | x_O, s)

and over S folded states lppd = log mean_s p(x_O | s), cell_mean = sum_s q_md(s) / sum_s p(x_O | s) -- the states
weighted by p(x_O | s), not the plain mean of cell_state.

The weights w_k are predictive_ref's own (its family functions called on a row of no features, which leaves the
weights alone); the Bernoulli terms are the same three formulas, restated per feature (`*_parts`).
tests/test_predictive_na_ref.py ties the whole statement back to predictive_ref: the masked density is the sum of
predictive_ref's complete-row densities over all completions of the missing cells.
"""
import numpy as np

import predictive_ref as pref


def _no_features(M=1):
    return np.zeros((M, 0), dtype=np.int32)


def collapsed_parts(Nk, S, alpha, N, beta, gamma):
    """(log w (K,), l1 (K, P), l0 (K, P)) of the finite collapsed sampler's predictive"""
    Nk = np.asarray(Nk, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    w = pref.collapsed_terms(_no_features(), Nk, S[:, :0], alpha, N, beta, gamma)[0]
    den = np.log(beta + gamma + Nk)[:, None]
    return w, np.log(beta + S) - den, np.log(gamma + Nk[:, None] - S) - den


def dp_parts(Nk, S, alpha, N, beta, gamma):
    """... of the DP sampler: the maxK labels (-inf weight for an unused one), then the new-cluster column"""
    Nk = np.asarray(Nk, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    w = pref.dp_terms(_no_features(), Nk, S[:, :0], alpha, N, beta, gamma)[0]
    den = np.log(beta + gamma + Nk)[:, None]
    P = S.shape[1]
    new1 = np.full((1, P), np.log(beta) - np.log(beta + gamma))
    new0 = np.full((1, P), np.log(gamma) - np.log(beta + gamma))
    return (w, np.concatenate([np.log(beta + S) - den, new1], axis=0),
            np.concatenate([np.log(gamma + Nk[:, None] - S) - den, new0], axis=0))


def explicit_parts(pi, theta):
    """... for explicit (pi, theta): stick-breaking and full"""
    theta = np.asarray(theta, dtype=np.float64)
    w = pref.explicit_terms(_no_features(), pi, theta[:, :0])[0]
    with np.errstate(divide="ignore"):
        return w, np.log(theta), np.log(1.0 - theta)


def masked_terms(X, miss, parts):
    """(M, Kc) log category terms over the observed cells only; only terms of observed cells are ever added"""
    w, l1, l0 = parts
    X = np.asarray(X)
    obs = ~np.asarray(miss, dtype=bool)
    one = (obs & (X == 1))[:, None, :]
    zero = (obs & (X == 0))[:, None, :]
    with np.errstate(invalid="ignore"):
        t = np.where(one, l1[None, :, :], 0.0).sum(axis=2) + np.where(zero, l0[None, :, :], 0.0).sum(axis=2)
        return w[None, :] + t


def cells_of(miss):
    """(rows, cols) of the missing cells, sorted by (row, column)"""
    rows, cols = np.nonzero(np.asarray(miss, dtype=bool))
    return rows.astype(np.int64), cols.astype(np.int32)


def cell_logjoint(terms, rows, cols, parts):
    """log q for every missing cell: log sum_k exp(terms[row, k] + l1[k, col])"""
    l1 = parts[1]
    return pref.logdens(terms[rows] + l1[:, cols].T)


def state(X, miss, parts):
    """(logdens (M,), resp (M, Kc), log cell joint (n,), cell_state (n,)) of one state"""
    t = masked_terms(X, miss, parts)
    rows, cols = cells_of(miss)
    ld = pref.logdens(t)
    lj = cell_logjoint(t, rows, cols, parts) if rows.size else np.zeros(0)
    return ld, pref.resp(t), lj, np.exp(lj - ld[rows])


def fold(logdens_trace, logjoint_trace, rows):
    """(lppd (M,), cell_mean (n,)) from the (S, M) and (S, n) per-state traces: the number of states cancels in the ratio"""
    lp = pref.lppd(logdens_trace)
    if logjoint_trace.shape[1] == 0:
        return lp, np.zeros(0)
    return lp, np.exp(pref.lppd(logjoint_trace) - lp[rows])


def completions(x, miss_row):
    """every completion of one row: (2^|U|, P), the missing cells running over all 0/1 patterns"""
    U = np.flatnonzero(miss_row)
    out = np.repeat(np.asarray(x, dtype=np.int32)[None, :], 1 << U.size, axis=0)
    for j, d in enumerate(U):
        out[:, d] = (np.arange(1 << U.size) >> j) & 1
    return out


# ---------------------------------------------------------------- the GPU cases (tests/test_gpu_predict_na.py)
# sampler, K (or maxK), P, beta, gamma, new rows M, share of the cells masked; tests/test_predictive_na_ref.py proves
# from the plan that they reach both forms of the masked scorer
CASES = [
    ("collapsed", 2, 1, 0.5, 0.5, 1300, 0.6),        # smallest shape
    ("collapsed", 3, 5, 0.7, 0.4, 513, 0.1),         # small shape, width-5 groups
    ("collapsed", 3, 33, 0.5, 0.5, 511, 0.6),        # a group straddling the word boundary (bits 30 to 34)
    ("collapsed", 4, 37, 0.6, 0.9, 513, 0.6),        # a short last group, and bit 32
    ("collapsed", 4, 37, 0.6, 0.9, 1, 0.6),          # one new row
    ("collapsed", 20, 50, 0.5, 0.5, 1300, 0.1),      # the north star's table shape
    ("collapsed", 32, 100, 0.7, 0.4, 513, 0.6),      # group width 4
    ("collapsed", 64, 50, 0.5, 0.5, 511, 0.1),       # the global form on a resident shape
    ("collapsed", 20, 120, 0.5, 0.5, 513, 0.1),      # the LDS form in groups of 4
    ("dp", 19, 50, 0.5, 0.5, 1300, 0.6),             # the DP's new-cluster column (the sampler takes beta == gamma only)
    ("dp", 19, 50, 0.5, 0.5, 1, 0.1),                # one new row
    ("stickbreaking", 50, 50, 0.3, 1.1, 513, 0.1),   # explicit parameters
    ("full", 8, 100, 0.7, 0.4, 1300, 0.1),           # explicit parameters
    ("collapsed", 3, 150, 0.5, 0.5, 511, 0.6),       # generic shape (P > 128)
    ("stickbreaking", 70, 10, 0.5, 0.5, 1300, 0.1),  # generic shape (more than 64 categories)
]


def case_mask(rng, M, P, frac):
    """a random mask of that share; from four rows on, row 0 has every cell missing, row 1 none, row 2 only cell 0
    and row 3 only cell P - 1 (one new row: the random mask alone, with at least one cell missing)"""
    miss = rng.random((M, P)) < frac
    if M >= 4:
        miss[0] = True
        miss[1:4] = False
        miss[2, 0] = True
        miss[3, P - 1] = True
    else:
        miss[0, rng.integers(P)] = True
    return miss


def planted():
    """The usefulness case: synth, N = 4096 fitted rows and 512 held-out ones, P = 24, K = 3, 20 % of the held-out cells
    hidden completely at random.  Returns (X, Xnew, miss, the hidden values, each feature's observed rate in X)."""
    import importlib
    synth = importlib.import_module("bmm_mcmc_amd.synth")
    A = np.array(synth.host_matrix(4096 + 512, 24, 3, 100)[0])
    X, Xnew = np.asfortranarray(A[:4096]), A[4096:]
    miss = np.random.default_rng(1000).random(Xnew.shape) < 0.2
    rows, cols = np.nonzero(miss)
    return X, Xnew, miss, Xnew[rows, cols], X.mean(axis=0)


def brier(p, truth):
    return float(np.mean((np.asarray(p, dtype=np.float64) - np.asarray(truth, dtype=np.float64)) ** 2))


# ---------------------------------------------------------------- the plan, restated
# bmm_predict_na_plan (csrc/chain.hip: na_form_of): the split image holds two tables of G x KT x 2^W doubles, the KT
# constants padded to an even count, and the 256-entry exp table; the LDS form needs a resident shape (at most 64
# categories, P <= 128) and the image within the 160 KiB of a gfx950 workgroup.
KT_LIST = (4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 52, 56, 64)
LDS_MAX = 163840


def plan(sampler, K, P, W):
    """{"form", "lds_bytes", "threads", "table_bytes"} for group width W (bmm_spec_group_width_for names it)"""
    Kc = K + 1 if sampler == "dp" else K
    kts = [kt for kt in KT_LIST if kt >= Kc]
    resident = bool(kts) and P <= 128
    G = (P + W - 1) // W
    if resident:  # ... and the head of the sweep's own table image with its histogram must fit too (chain_shape)
        kt = kts[0]
        head = G * kt * (1 << W) + 2 * kt + (kt + 1) // 2 + (((kt + 1) // 2) & 1) + 256
        resident = head * 8 + (K * P + K + 4) * 4 <= LDS_MAX
    KT = kts[0] if resident else (Kc + 3) // 4 * 4
    table = (2 * G * KT * (1 << W) + KT + (KT & 1) + 256) * 8
    lds = resident and table <= LDS_MAX
    return {"form": "lds" if lds else "global", "lds_bytes": table if lds else 0, "threads": 512 if lds else 256,
            "table_bytes": table}
