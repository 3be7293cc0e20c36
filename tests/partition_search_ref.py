"""NumPy restatement of the greedy search for the clustering point estimate (include/bmm_mcmc.h "greedy search",
DESIGN.md section 27), on top of partition_ref.  Labels are 1-based as the library's z; slots are 1 .. Ka.  Everything
Binder is in int64 arrays and Python integers (exact); VI uses math.log, the scores summed over t in ascending order
in binary64 and the totals with math.fsum.  It also carries the trace generator and the case list of the tests."""
import math

import numpy as np

import partition_ref as pr


def f(n):
    n = int(n)
    return n * math.log(n) if n else 0.0


def phi(n):
    """f(n + 1) - f(n): what a cell of n gains when a row joins it; phi(0) = 0"""
    return f(n + 1) - f(n)


class State:
    """the candidate c (1-based slots, Ka of them), its sizes n[a] and the S tables T[t][a][b] (0-based indices)"""

    def __init__(self, z, c, Kc, Ka):
        self.z = np.asarray(z, dtype=np.int64) - 1
        self.c = np.asarray(c, dtype=np.int64) - 1
        self.S, self.N = self.z.shape
        self.Kc, self.Ka = Kc, Ka
        self.rebuild()

    def rebuild(self):
        self.n = np.bincount(self.c, minlength=self.Ka).astype(np.int64)
        self.T = np.zeros((self.S, self.Ka, self.Kc), dtype=np.int64)
        for t in range(self.S):
            self.T[t] = np.bincount(self.c * self.Kc + self.z[t], minlength=self.Ka * self.Kc).reshape(self.Ka, self.Kc)

    def labels(self):
        return (self.c + 1).astype(np.int32)

    def binder2(self):
        """S sum n_a^2 + sum_t sum_b n_t,b^2 - 2 sum_t sum_ab T^2, a Python integer"""
        sq = lambda v: int((v * v).sum())  # int64: every sum stays below S N^2 < 2^63
        return self.S * sq(self.n) + sq(self.T.sum(1)) - 2 * sq(self.T)

    def vi_tot(self):
        """S sum f(n_a) + sum_t sum_b f(n_t,b) - 2 sum_t sum_ab f(T), fsum"""
        terms = [self.S * f(x) for x in self.n if x]
        terms += [f(x) for x in self.T.sum(1).ravel() if x]
        terms += [-2.0 * f(x) for x in self.T.ravel() if x]
        return math.fsum(terms)

    def total(self, criterion):
        return self.binder2() if criterion == "binder" else self.vi_tot()

    def scores(self, i, criterion):
        """g_a of row i for every slot, the row taken out of the state"""
        a0 = self.c[i]
        g = []
        for a in range(self.Ka):
            own = 1 if a == a0 else 0
            m = int(self.n[a]) - own
            U = [int(self.T[t, a, self.z[t, i]]) - own for t in range(self.S)]
            if criterion == "binder":
                g.append(self.S * m - 2 * sum(U))
            else:
                acc = 0.0
                for u in U:  # ascending t, binary64
                    acc += phi(u)
                g.append(self.S * phi(m) - 2.0 * acc)
        return g

    def scores_batch_binder(self, rows):
        """the Binder scores of several rows against the state as it stands: (len(rows), Ka) int64"""
        rows = np.asarray(rows)
        tot = np.zeros((len(rows), self.Ka), dtype=np.int64)
        for t in range(self.S):
            tot += self.T[t][:, self.z[t, rows]].T
        own = np.zeros((len(rows), self.Ka), dtype=np.int64)
        own[np.arange(len(rows)), self.c[rows]] = 1
        return self.S * (self.n[None, :] - own) - 2 * (tot - self.S * own)

    def move_delta_vi(self, i, a):
        """vi_tot(c with row i in slot a) - vi_tot(c): the fsum of the terms the move changes, and of nothing else"""
        a0 = self.c[i]
        if a == a0:
            return 0.0
        S = self.S
        m, m0 = int(self.n[a]), int(self.n[a0]) - 1
        terms = [S * f(m + 1), -S * f(m), S * f(m0), -S * f(m0 + 1)]
        for t in range(S):
            b = self.z[t, i]
            u, u0 = int(self.T[t, a, b]), int(self.T[t, a0, b]) - 1
            terms += [-2.0 * f(u + 1), 2.0 * f(u), -2.0 * f(u0), 2.0 * f(u0 + 1)]
        return math.fsum(terms)

    @staticmethod
    def choose(g, a0):
        """the slot with the smallest g; on exact ties the current slot, then the lowest"""
        best = a0
        for a in range(len(g)):
            if g[a] < g[best]:
                best = a
        return best

    def move(self, i, a1):
        a0 = self.c[i]
        if a1 == a0:
            return
        for t in range(self.S):
            b = self.z[t, i]
            self.T[t, a0, b] -= 1
            self.T[t, a1, b] += 1
        self.n[a0] -= 1
        self.n[a1] += 1
        self.c[i] = a1

    def one_pass(self, B, criterion):
        """contiguous batches of B rows, each scored against the tables at the start of its batch; returns the moves"""
        moved = 0
        for i0 in range(0, self.N, B):
            rows = np.arange(i0, min(i0 + B, self.N))
            if criterion == "binder":  # choose() and move(), vectorised over the batch
                G = self.scores_batch_binder(rows)
                k = np.arange(len(rows))
                first = G.argmin(1)  # the lowest slot among the minima
                old = self.c[rows]
                new = np.where(G[k, old] == G[k, first], old, first)
                mv = rows[new != old]
                a0, a1 = self.c[mv], new[new != old]
                for t in range(self.S):
                    np.subtract.at(self.T[t], (a0, self.z[t, mv]), 1)
                    np.add.at(self.T[t], (a1, self.z[t, mv]), 1)
                np.subtract.at(self.n, a0, 1)
                np.add.at(self.n, a1, 1)
                self.c[mv] = a1
                moved += len(mv)
            else:
                new = [self.choose(self.scores(i, criterion), self.c[i]) for i in rows]
                for i, a1 in zip(rows, new):
                    if a1 != self.c[i]:
                        moved += 1
                        self.move(i, a1)
        return moved


def defaults(N, batch=None, min_batch=None):
    batch = -(-N // 8) if batch is None else min(int(batch), N)
    min_batch = -(-N // 256) if min_batch is None else int(min_batch)
    return batch, min(min_batch, batch)


def search(z, Kc, criterion="binder", start=None, batch=None, min_batch=None, max_passes=50, Ka=None):
    """the search of the header's pseudo-code; start None: the draws' minimiser at stride 1"""
    z = np.asarray(z)
    S, N = z.shape
    Ka = Kc if Ka is None else Ka
    if start is None:
        start = z[pr.point_estimate(z, Kc, criterion, 1)]
    B, min_batch = defaults(N, batch, min_batch)
    st = State(z, start, Kc, Ka)
    best = st.c.copy()
    best_tot = st.total(criterion)
    start_tot, start_b2 = best_tot, st.binder2()
    log = {"batch": [], "moved": [], "total": []}
    converged = False
    while len(log["batch"]) < max_passes:
        moved = st.one_pass(B, criterion)
        tot = st.total(criterion)
        log["batch"].append(B)
        log["moved"].append(moved)
        log["total"].append(tot)
        if moved == 0:
            converged = True
            break
        if tot < best_tot:
            best, best_tot = st.c.copy(), tot
        else:
            st.c = best.copy()
            st.rebuild()
            if B == min_batch:
                break
            B = max(min_batch, B // 2)
    st.c = best.copy()
    st.rebuild()
    norm = (2.0 * S) if criterion == "binder" else float(S) * N
    return {"z": st.labels(), "binder2": st.binder2(), "total": best_tot, "loss": best_tot / norm,
            "start_total": start_tot, "start_binder2": start_b2, "start_loss": start_tot / norm,
            "passes": len(log["batch"]), "batch": log["batch"], "moved": log["moved"], "pass_total": log["total"],
            "converged": converged, "n_clusters": int(np.count_nonzero(st.n))}


def expected_vi(c, z, Kc):
    """mean over the draws of partition_ref.vi(c, z_t): the fsum expected VI of a candidate (labels up to Kc)"""
    z = np.asarray(z)
    return math.fsum(pr.vi(c, z[t], Kc) for t in range(z.shape[0])) / z.shape[0]


def make_trace(Kc, N, S, eps, seed):
    """a truth drawn with probabilities proportional to 0.7^k, each label of each draw replaced by a uniform one with
    probability eps, every row renumbered by a random permutation: (z (S, N) int32 column-major 1-based, truth)"""
    rng = np.random.default_rng(seed)
    p = 0.7 ** np.arange(Kc)
    truth = rng.choice(Kc, size=N, p=p / p.sum())
    z = np.empty((S, N), dtype=np.int64)
    for t in range(S):
        row = truth.copy()
        flip = rng.random(N) < eps
        row[flip] = rng.integers(0, Kc, size=int(flip.sum()))
        z[t] = rng.permutation(Kc)[row]
    return np.asfortranarray(z + 1, dtype=np.int32), (truth + 1).astype(np.int32)


EPS = 0.3
# (Kc, N, S, batch, min_batch, start): the shapes the device is held to (tests/test_gpu_partition_search.py);
# batch / min_batch None: the defaults.  start: "best" (the draws' minimiser), "one" (all rows in one cluster), "row0".
CASES = [
    (1, 1, 1, 1, 1, "best"),
    (2, 63, 3, 1, 1, "best"),
    (3, 65, 17, 16, 1, "best"),
    (4, 65, 17, 65, 1, "one"),
    (8, 257, 33, 64, 1, "row0"),
    (5, 1000, 17, 1000, 1, "one"),
    (20, 10007, 17, 1251, 40, "best"),
    (33, 10007, 40, 1251, 40, "best"),
    (64, 4099, 9, 512, 17, "best"),       # every slot in use, none to open
    (6, 10007, 200, 10007, 40, "best"),   # more draws than one LDS block
    (4, 262147, 5, None, None, "best"),   # many workgroups, the default batch
]
# shapes that only the plan sees (no device): the 32-bit sums of a block bound the draws of a block
PLAN_ONLY = [
    (2, 30_000_000, 200, None, None, "best"),
]


def case_id(case):
    return "K%d-N%d-S%d-B%s-%s" % (case[0], case[1], case[2], case[3], case[5])


def start_of(case, z):
    """the start the case names, 1-based labels, or None for the draws' minimiser"""
    Kc, N, S, batch, min_batch, start = case
    if start == "one":
        return np.ones(N, dtype=np.int32)
    if start == "row0":
        return np.ascontiguousarray(z[0], dtype=np.int32)
    return None
