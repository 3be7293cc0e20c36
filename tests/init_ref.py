"""The k-modes++ initial allocation (include/bmm_mcmc.h "initial allocation"), restated in NumPy
on the unpacked 0/1 matrix.  Labels are 0-based here.  Everything is integer arithmetic but for one product per centre,
so the device is held to this bit for bit."""
import numpy as np

from split_merge_ref import _M32, philox4x32_10, u01

STREAM_INIT = 10          # bmm_spec.h kStreamInit
MAX_CENTRE_BYTES = 65536  # BMM_INIT_MAX_CENTRE_BYTES
LDS_BUDGET = 131072       # kInitLdsBudget: centres and count histogram of k_init_assign in dynamic LDS up to here


def init_uniform(seed, j):
    """bmm_spec.h init_uniform: the first block of stream 10 at counter (j, 0, 0) under the chain's key"""
    r = philox4x32_10((j, 0, 0, STREAM_INIT), (seed & _M32, (seed >> 32) & _M32))
    return u01(r[0], r[1])


def centre_bytes(Kc, P):
    return Kc * ((P + 31) // 32) * 4


def counts_in_lds(Kc, P):
    """init_counts_in_lds of chain.hip: whether the assign kernel counts its labels itself (else k_count_labels_generic does)"""
    return centre_bytes(Kc, P) + Kc * (P + 1) * 4 <= LDS_BUDGET


def distances(X, C):
    """N x k Hamming distances of the rows of X to the rows of C"""
    return np.stack([(X != c).sum(1) for c in C], 1).astype(np.int64)


def kmodes(X, Kc, seed, iters):
    """Returns labels, rows (the picked rows), centres (k_eff x P), Nk, k_eff, rounds_run, changed_last, cost, and per
    round `changed` (one entry per round run) and `costs` (entry 0 after the seeding, then one per round run); `ties`
    counts the rows of the last assignment whose smallest distance two or more centres share."""
    X = np.asarray(X, dtype=np.int64)
    N, P = X.shape
    assert 1 <= Kc and iters >= 0
    r0 = min(N - 1, int(init_uniform(seed, 0) * float(N)))
    rows, C = [r0], [X[r0].copy()]
    dist = np.full(N, P + 1, dtype=np.int64)
    near = np.zeros(N, dtype=np.int64)

    def fix(m):
        h = (X != C[m]).sum(1)
        better = h < dist  # strict: ties keep the lower label
        dist[better] = h[better]
        near[better] = m

    fix(0)
    k_eff = Kc
    for j in range(1, Kc):
        T = int(dist.sum())
        if T == 0:
            k_eff = j
            break
        t = min(T - 1, int(init_uniform(seed, j) * float(T)))
        r = int(np.searchsorted(np.cumsum(dist), t, side="right"))  # the smallest i whose inclusive prefix sum exceeds t
        rows.append(r)
        C.append(X[r].copy())
        fix(j)
    C = np.array(C, dtype=np.int64)
    z = near.copy()
    D = distances(X, C)
    assert np.array_equal(D.argmin(1), z) and np.array_equal(D.min(1), dist)
    costs, changed = [int(dist.sum())], []
    for _ in range(iters):
        for k in range(k_eff):
            members = z == k
            nk, s = int(members.sum()), X[members].sum(0)
            C[k] = np.where(2 * s > nk, 1, np.where(2 * s < nk, 0, C[k]))
        D = distances(X, C)
        znew = D.argmin(1)  # the first minimum: the lowest label
        changed.append(int((znew != z).sum()))
        z = znew
        costs.append(int(D.min(1).sum()))
        if changed[-1] == 0:
            break
    ties = int(((D == D.min(1, keepdims=True)).sum(1) > 1).sum())
    return {"labels": z, "rows": np.array(rows, dtype=np.int64), "centres": C.astype(np.uint8),
            "Nk": np.bincount(z, minlength=k_eff).astype(np.int32), "k_eff": k_eff, "rounds_run": len(changed),
            "changed_last": changed[-1] if changed else 0, "cost": costs[-1], "changed": changed, "costs": costs, "ties": ties}


def counts(X, z, K):
    """Nk (K) and S (K x P) of 0-based labels"""
    X = np.asarray(X, dtype=np.int64)
    Nk = np.bincount(z, minlength=K).astype(np.int32)
    S = np.zeros((K, X.shape[1]), dtype=np.int32)
    np.add.at(S, z, X.astype(np.int32))
    return Nk, S
