"""NumPy restatement of the posterior summary (include/bmm_mcmc.h "posterior summary"), written
from the definitions on top of tests/ecr_ref.py; the device fold (csrc/kernels.hip.h, k_sum_*) must match it exactly:
the counts are integers, and the sums are added one sweep at a time in sweep order, as the device adds them.

Labels are 0-based here, -1 is an unassigned label.  z is the kept trace, S x N; theta K x P x S; alpha S.
  folded rows  s >= first_fold and s % stride == 0 (first_fold: 1 in a run without burn-in, whose row 0 is the
               starting state; else 0)
  pivot        "first": the first row whose labels are all assigned (whether or not it is folded); N labels; None
  permutation  one pass of ecr_ref per folded row against the pivot; None: the identity and agree 0; the rows that
               are not folded keep the identity and agree -1
  counts       cnt[i, k] = #{folded s : perm_s[z_s[i]] = k}
  z_hat        argmax_k cnt[i, k], the lowest k on a tie (0-based here); n_max that count
  size_sum     cnt.sum(axis=0)
  profiles     theta_sum[perm_s[l]] += theta[l, :, s] and theta_sq[perm_s[l]] += theta[l, :, s] ** 2 over the cells that
               are not NaN, theta_n[perm_s[l]] += 1 when theta[l, 0, s] is not NaN; alpha_sum += (alpha, alpha ** 2)
"""
import numpy as np

import ecr_ref as E


def folded_rows(S, stride=1, first_fold=0):
    return [s for s in range(S) if s >= first_fold and s % stride == 0]


def first_assigned(z):
    for s in range(z.shape[0]):
        if (z[s] >= 0).all():
            return s
    return None


def row_permutation(zs, c, K):
    """(perm (K,) int32, agree) of one row against the pivot c: the unassigned labels are left out of the table"""
    ok = zs >= 0
    n = E.tables(zs[ok][None, :], c[ok], K)
    perm = E.permutations(n)
    return perm[0], int(E.agreement(n, perm)[0])


def summarise(z, K, theta=None, alpha=None, pivot="first", stride=1, first_fold=0, permutations=None):
    """The whole summary as a dict.  permutations: (S, K), taken as given for the folded rows instead of computed (the
    device tests hand in those of the pinned relabelling, which they have compared first); agree is then recounted."""
    z = np.asarray(z)
    S, N = z.shape
    rows = folded_rows(S, stride, first_fold)
    if pivot is None:
        c = None
    elif isinstance(pivot, str):
        assert pivot == "first"
        f = first_assigned(z)
        c = None if f is None else z[f].astype(np.int32)
    else:
        c = np.asarray(pivot).astype(np.int32)
    perms = np.tile(np.arange(K, dtype=np.int32), (S, 1))
    agree = np.full(S, -1, dtype=np.int64)
    cnt = np.zeros((N, K), dtype=np.uint32)
    P = 0 if theta is None else theta.shape[1]
    theta_sum, theta_sq = np.zeros((K, P)), np.zeros((K, P))
    theta_n = np.zeros(K, dtype=np.int32)
    alpha_sum = np.zeros(2)
    for s in rows:  # one sweep at a time, in sweep order: the device's add order
        if pivot is None:
            agree[s] = 0
        elif permutations is not None:
            perms[s] = permutations[s]
            ok = z[s] >= 0
            agree[s] = int((perms[s][z[s][ok]] == c[ok]).sum())
        else:
            perms[s], agree[s] = row_permutation(z[s], c, K)
        ok = np.flatnonzero(z[s] >= 0)
        np.add.at(cnt, (ok, perms[s][z[s][ok]]), 1)
        if theta is not None:
            for l in range(K):
                t = theta[l, :, s]
                keep = ~np.isnan(t)
                to = perms[s][l]
                theta_sum[to, keep] = theta_sum[to, keep] + t[keep]
                sq = t[keep] * t[keep]
                theta_sq[to, keep] = theta_sq[to, keep] + sq
                if keep[0]:
                    theta_n[to] += 1
        if alpha is not None:
            a = float(np.asarray(alpha).ravel()[s])
            alpha_sum[0] = alpha_sum[0] + a
            sq = a * a
            alpha_sum[1] = alpha_sum[1] + sq
    return {"pivot": c, "folded": rows, "n_folded": len(rows), "permutations": perms, "agree": agree, "counts": cnt,
            "z_hat": np.argmax(cnt, axis=1).astype(np.int32),  # first maximum: the lowest label
            "n_max": cnt.max(axis=1).astype(np.uint32), "size_sum": cnt.sum(axis=0, dtype=np.int64),
            "theta_sum": theta_sum, "theta_sq": theta_sq, "theta_n": theta_n, "alpha_sum": alpha_sum}


def trace_bytes(S, N, K):
    """What the label trace adds to a run's device buffers (include/bmm_mcmc.h, bmm_run_bytes): the S x N int32 trace and
    the two staging blocks of its way out -- a whole number of observations' S labels (one byte each up to K = 254, four
    above), at most 4 MiB and at least 32 observations, in multiples of 32 -- each carved on a 256-byte boundary."""
    el = 1 if K <= 254 else 4
    B = max((4 << 20) // (S * el) // 32 * 32, 32)
    block = min(B, N) * S * el
    return 4 * S * N + 2 * ((block + 255) // 256 * 256)
