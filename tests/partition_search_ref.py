"""NumPy restatement of the greedy search for the clustering point estimate (include/bmm_mcmc.h "greedy search",
DESIGN.md section 27), on top of partition_ref.  Labels are 1-based as the library's z; slots are 1 .. Ka.  Everything
Binder is in int64 arrays and Python integers (exact); VI uses math.log, the scores summed over t in ascending order
in binary64 and the totals with math.fsum; search_vi_margins restates the VI search once more in np.longdouble and
measures by how much every decision was taken, for the cases (VI_CASES) on which the device must follow it with ==.
It also carries the trace generator and the case lists of the tests."""
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


def f_table(N):
    """f(k) = k log k for k = 0 .. N + 1 in np.longdouble, f(0) = 0"""
    k = np.arange(N + 2, dtype=np.longdouble)
    F = np.zeros(N + 2, dtype=np.longdouble)
    F[1:] = k[1:] * np.log(k[1:])
    return F


def vi_scores(st, rows, PHI):
    """the VI scores of several rows against the state as it stands, every phi and sum in np.longdouble:
    G (R, Ka), the sizes m (R, Ka) and the cells U (S, R, Ka) the scores were made of (the row taken out)"""
    rows = np.asarray(rows)
    R = len(rows)
    own = np.zeros((R, st.Ka), dtype=np.int64)
    own[np.arange(R), st.c[rows]] = 1
    m = st.n[None, :] - own
    U = np.empty((st.S, R, st.Ka), dtype=np.int32)
    acc = np.zeros((R, st.Ka), dtype=np.longdouble)
    for t in range(st.S):  # one elementwise add per draw: equal sequences of cells give equal bits
        U[t] = st.T[t][:, st.z[t, rows]].T - own
        acc += PHI[U[t]]
    return st.S * PHI[m] - 2 * acc, m, U


def search_vi_margins(z, Kc, start, batch, min_batch, max_passes=50, Ka=None, keep_scores=False):
    """search(z, Kc, "vi", ...) with the scores vectorised over a batch and every f, phi and sum in np.longdouble,
    and beside the keys of search():
      score_margin     the smallest g[a] - g[chosen] over every scored row of every pass and every slot a != chosen
                       that is no structural tie (the same m_a and the same cell U_t in every draw t as the chosen
                       slot: bit-equal in any implementation with a fixed order, decided by the tie rule)
      total_margin     the smallest |pass_total - best_total| over the keep-best comparisons (passes that moved a row)
      structural_ties  how many (row, slot) pairs were left out as such
      from_high, into_high, opened_empty   moves out of / into a slot >= 8 (0-based), moves into an empty slot
      stopped          "converged", "min_batch" or "max_passes"
    keep_scores: also "first_scores" (G of the first batch of the first pass), "first_choice" (its choices, 1-based)."""
    z = np.asarray(z)
    S, N = z.shape
    Ka = Kc if Ka is None else Ka
    if start is None:
        start = z[pr.point_estimate(z, Kc, "vi", 1)]
    B, min_batch = defaults(N, batch, min_batch)
    st = State(z, start, Kc, Ka)
    F = f_table(N)
    PHI = F[1:] - F[:-1]
    inf = np.longdouble(np.inf)
    out = {"score_margin": inf, "total_margin": inf, "structural_ties": 0, "from_high": 0, "into_high": 0,
           "opened_empty": 0}

    def total():
        return S * F[st.n].sum() + F[st.T.sum(1)].sum() - 2 * F[st.T].sum()

    def one_pass(B):
        moved = 0
        for i0 in range(0, N, B):
            rows = np.arange(i0, min(i0 + B, N))
            G, m, U = vi_scores(st, rows, PHI)
            k = np.arange(len(rows))
            first = G.argmin(1)  # the lowest slot among the minima
            old = st.c[rows]
            new = np.where(G[k, old] == G[k, first], old, first)
            same = (m == m[k, new][:, None]) & (U == U[:, k, new][:, :, None]).all(0)
            gap = G - G[k, new][:, None]
            assert not (same & (gap != 0)).any()
            out["structural_ties"] += int(same.sum()) - len(rows)
            gap[same] = inf  # the chosen slot itself among them
            out["score_margin"] = min(out["score_margin"], gap.min())
            if keep_scores and "first_scores" not in out:
                out["first_scores"], out["first_choice"] = G, (new + 1).astype(np.int32)
            mv = rows[new != old]
            a0, a1 = old[new != old], new[new != old]
            out["from_high"] += int((a0 >= 8).sum())
            out["into_high"] += int((a1 >= 8).sum())
            out["opened_empty"] += int((st.n[a1] == 0).sum())
            for t in range(S):
                np.subtract.at(st.T[t], (a0, st.z[t, mv]), 1)
                np.add.at(st.T[t], (a1, st.z[t, mv]), 1)
            np.subtract.at(st.n, a0, 1)
            np.add.at(st.n, a1, 1)
            st.c[mv] = a1
            moved += len(mv)
        return moved

    best = st.c.copy()
    best_tot = total()
    start_tot, start_b2 = best_tot, st.binder2()
    log = {"batch": [], "moved": [], "total": []}
    stopped = "max_passes"
    while len(log["batch"]) < max_passes:
        moved = one_pass(B)
        tot = total()
        log["batch"].append(B)
        log["moved"].append(moved)
        log["total"].append(float(tot))
        if moved == 0:
            stopped = "converged"
            break
        out["total_margin"] = min(out["total_margin"], abs(tot - best_tot))
        if tot < best_tot:
            best, best_tot = st.c.copy(), tot
        else:
            st.c = best.copy()
            st.rebuild()
            if B == min_batch:
                stopped = "min_batch"
                break
            B = max(min_batch, B // 2)
    st.c = best.copy()
    st.rebuild()
    norm = float(S) * N
    out.update({"z": st.labels(), "binder2": st.binder2(), "total": float(best_tot), "loss": float(best_tot) / norm,
                "start_total": float(start_tot), "start_binder2": start_b2, "start_loss": float(start_tot) / norm,
                "passes": len(log["batch"]), "batch": log["batch"], "moved": log["moved"], "pass_total": log["total"],
                "converged": stopped == "converged", "n_clusters": int(np.count_nonzero(st.n)), "stopped": stopped,
                "score_margin": float(out["score_margin"]), "total_margin": float(out["total_margin"])})
    return out


def score_error_bound(N, S):
    """E_g, what any binary64 score g_a = S phi(m_a) - 2 sum_t phi(U_t) may be off by: log within 1 ulp, |f| <=
    N log(N + 1), one rounding for the product, one for the difference and S sequential adds"""
    return 16 * S * (N + S) * math.log(N + 1) * 2.0 ** -52


def margins_hold(res, Kc, Ka, N, S):
    """the condition on a case: no correct implementation can flip a decision of this course"""
    return (res["score_margin"] >= 2 ** 10 * 2 * score_error_bound(N, S)
            and res["total_margin"] >= 2 ** 10 * 2 * pr.vi_bound(max(Kc, Ka), N) * S * N)


def expected_vi(c, z, Kc):
    """mean over the draws of partition_ref.vi(c, z_t): the fsum expected VI of a candidate (labels up to Kc)"""
    z = np.asarray(z)
    return math.fsum(pr.vi(c, z[t], Kc) for t in range(z.shape[0])) / z.shape[0]


def make_trace(Kc, N, S, eps, seed, decay=0.7):
    """a truth drawn with probabilities proportional to decay^k, each label of each draw replaced by a uniform one with
    probability eps, every row renumbered by a random permutation: (z (S, N) int32 column-major 1-based, truth)"""
    rng = np.random.default_rng(seed)
    p = decay ** np.arange(Kc)
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


# (Kc, N, S, batch, min_batch, start, Ka, decay, seed): the shapes on which the device's VI search is held to
# search_vi_margins with == (tests/test_gpu_partition_search_vi.py).  Every one meets margins_hold(): no gap between
# two scores or two totals is within 2^11 error bounds of 0, so no correct implementation decides otherwise.  start:
# "best", "row0" as above, "rand" (uniform over the Ka slots), "randKc" (uniform over the first Kc of Ka > Kc slots:
# the others start empty).
VI_CASES = [
    (64, 2053, 11, 512, 17, "best", 64, 0.97, 2),
    (64, 2053, 11, 2053, 17, "row0", 64, 0.97, 1),
    (33, 2053, 13, 700, 20, "row0", 33, 0.95, 1),
    (20, 4099, 23, 4099, 40, "row0", 20, 0.9, 1),
    (12, 1031, 35, 1031, 8, "row0", 16, 0.85, 1),
    (6, 1031, 201, 400, 8, "row0", 6, 0.7, 1),
    (10, 600, 9, 600, 5, "rand", 10, 0.9, 2),
    (4, 300, 5, 300, 2, "rand", 4, 0.7, 3),
    (3, 200, 7, 200, 3, "rand", 9, 0.7, 1),
    (2, 130, 5, 130, 1, "rand", 2, 0.7, 1),
    (12, 1031, 9, 300, 8, "randKc", 16, 0.85, 3),  # rows open empty slots; empty slots tie structurally
    (8, 300, 9, 300, 4, "rand", 5, 0.8, 1),        # a given start inside Ka = 5 < Kc = 8 slots
    (10, 600, 9, 600, 600, "rand", 10, 0.9, 2),    # ends at min_batch: the sixth pass does not improve
    (4, 300, 5, 150, 2, "rand", 4, 0.7, 3),        # ends at max_passes = 4 (11 passes if left alone)
    (20, 1031, 13, 1031, 8, "rand", 20, 0.9, 1),   # blocks of 10 and 3 draws, rows decided by gaps that one draw can turn
]
# the cases that are not given the default 50 passes
VI_MAX_PASSES = {(4, 300, 5, 150, 2, "rand", 4, 0.7, 3): 4}
# the cases of the first-pass test (one pass over one batch of all N rows): those above whose first pass lowers the
# total in the reference, one of each pair that shares a trace and a start
VI_FIRST_PASS = VI_CASES[:12] + VI_CASES[14:]


def vi_case_id(case):
    return "K%d-N%d-S%d-B%d-m%d-%s-Ka%d-d%g-s%d" % case


def vi_trace(case):
    Kc, N, S, _, _, _, _, decay, seed = case
    return make_trace(Kc, N, S, EPS, seed, decay)[0]


def vi_start(case, z):
    """the start the case names, 1-based labels in 1 .. Ka, always explicit"""
    Kc, N, S, _, _, start, Ka, _, seed = case
    if start == "best":
        return np.ascontiguousarray(z[pr.point_estimate(z, Kc, "vi", 1)], dtype=np.int32)
    if start == "row0":
        return np.ascontiguousarray(z[0], dtype=np.int32)
    hi = {"rand": Ka, "randKc": Kc}[start]
    return np.random.default_rng(seed + 50).integers(1, hi + 1, N).astype(np.int32)


def vi_reference(case, **kw):
    """search_vi_margins on a case: (z, start, result)"""
    Kc, N, S, batch, min_batch, _, Ka, _, _ = case
    z = vi_trace(case)
    start = vi_start(case, z)
    kw.setdefault("max_passes", VI_MAX_PASSES.get(case, 50))
    kw.setdefault("batch", batch)
    kw.setdefault("min_batch", min_batch)
    return z, start, search_vi_margins(z, Kc, start, Ka=Ka, **kw)
