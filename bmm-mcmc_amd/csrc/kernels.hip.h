// kernels.hip.h -- gfx950 kernels of the cluster-allocation path.
//
// One observation per lane (wave64).  X is streamed either as bit planes packed once when the
// matrix is handed over (ceil(P/32) 32-bit words per observation; the default) or as the N x P
// int32 column-major matrix R hands over (lane i reads X[i + d*N]: a wave reads 256 contiguous
// bytes per feature, packed to bits in registers as they arrive).  The per-cluster log-predictive
// is K*ceil(P/W) LDS lookups into 2^W-entry group tables (one ds_read_b64 + one v_add_f64 per
// cluster per W features, W = 5, or 4 for big table images: bmm_spec.h; the category's constant term
// sits in group 0) instead of K*P multiply-adds; the observation's own cluster is scored from tables
// of its own with groups of 3.  All entries of a group sit in one 256- (128-) byte run, i.e. on different
// bank pairs, so the per-lane-indexed read is conflict-free.  Work is handed out per wave in chunks of 64
// observations from a counter in LDS.  Sufficient-statistic changes are accumulated as integers in
// LDS (a few movers: one at a time by the whole wave, one feature per lane; many: every mover lane
// walks its own set bits) and flushed with one global integer atomic per touched cell per
// workgroup -- order-independent, hence deterministic.
//
// Reference lines realised here (all /root/reference/src):
//   z | rest, finite K      collapsed_gibbs.cpp:86-182
//   z | rest, CRP           collapsed_gibbs_dp.cpp:108-242
//   z | pi, theta           stickbreaking.cpp:70-125, counts :164-186
//   theta-hat               collapsed_gibbs.cpp:205-219, collapsed_gibbs_dp.cpp:266-281
//   v, pi, theta draws      stickbreaking.cpp:187-229
//   alpha                   utils.cpp:6-14
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bmm_spec.h"

namespace bmm {

typedef __attribute__((address_space(3))) double lds_f64;  // LDS-qualified, keeps ds_read under volatile

constexpr int kMaxP = 128;      // fast path: 4 bit-words per observation
constexpr int lcm_(int a, int b) { int x = a; while (x % b) x += a; return x; }
// features per table-building chunk: whole groups of every width
constexpr int kChunkP = kMaxP / lcm_(lcm_(kGroupW, kGroupWAlt), kGroupWm) * lcm_(lcm_(kGroupW, kGroupWAlt), kGroupWm);
constexpr int kMaxCats = 64;    // fast path: clusters (+ the DP's new-cluster option)
constexpr int kMaxCatsAny = 1024;  // generic path

enum : int { MODE_COLLAPSED = 0, MODE_DP = 1, MODE_SB = 2, MODE_FULL = 3 };
// the two samplers that carry explicit (pi, theta) and resample z | pi, theta in one exact batch
__host__ __device__ inline bool explicit_params(int mode) { return mode == MODE_SB || mode == MODE_FULL; }

// Layout of the table image in global memory, in doubles:
//   Tp  [G][KT][M]    group tables against the full statistics (M = 2^W, W the shape's group width:
//                     ChainParams::W); group 0 carries the category's
//                     prior / weight term Cp, so a score is just the sum of G entries
//   Cp  [KT]          that term on its own (kept for inspection; the kernels do not read it)
//   Cm  [KT]          ... with the scored observation removed from its own cluster
//   Nk  [KT] int32    (two per double slot, padded to an even number of doubles)
//   E   [256]         2^(j/256), the table of the spec's expw_ (read per lane in the draw)
//   Tm  [Gm][KT][Mm]  group tables with the observation's own contribution removed, Cm in group 0
//                     (not SB); narrower groups, Mm = 2^kGroupWm entries each; Gm padded with all-zero
//                     groups to a multiple of kOwnSub
// A workgroup copies the head (Tp..Nk) into LDS, and Tm too when both fit in 160 KiB;
// otherwise Tm is gathered from global memory (L2-resident, 1/K of the lookups).
struct TableLayout {
    int G, KT, Gm, M;  // Gm = 0: no own-cluster tables; M = entries per group of Tp
    __host__ __device__ int tp() const { return 0; }
    __host__ __device__ int cp() const { return G * KT * M; }
    __host__ __device__ int cm() const { return cp() + KT; }
    __host__ __device__ int nk() const { return cm() + KT; }
    __host__ __device__ int et() const { return nk() + (KT + 1) / 2 + (((KT + 1) / 2) & 1); }
    __host__ __device__ int tm() const { return et() + 256; }
    __host__ __device__ int head() const { return tm(); }
    __host__ __device__ int gm_pad() const { return (Gm + kOwnSub - 1) / kOwnSub * kOwnSub; }
    __host__ __device__ int doubles() const { return tm() + gm_pad() * KT * kGroupMm; }
};

// doubles of the packed image Tq behind the table image of a chain that runs k_resample_pk, and of Tm32 behind Tq
__host__ __device__ inline int pk_tq_doubles(const TableLayout& L) { return L.G * (L.KT / 2) * L.M; }

struct ChainParams {
    int mode;           // MODE_*
    int64_t N;          // observations held by this chain object (a shard, or all of them)
    int64_t Ntot;       // observations of the whole chain (= N unless the chain is sharded over ranks)
    int64_t obs0;       // global index of local observation 0 (keys the per-observation Philox counter)
    int P, W, G, Gm;    // features; features per lookup group of the tables (bmm_spec.h); groups of the
                        // tables, of the own-cluster tables
    int K;              // labels (K or maxK)
    int Kc;             // categories = K (+1 for DP)
    int KT;             // Kc rounded up to the kernel's accumulator count
    double beta, gamma, a, b;
    int sample_alpha;
    uint64_t seed;
};
__host__ __device__ inline TableLayout layout_of(const ChainParams& p, bool own_tables) {
    return TableLayout{p.G, p.KT, own_tables ? p.Gm : 0, 1 << p.W};
}

// The integer delta accumulators exist kDeltaReps times (replica r of dS at dS + r*K*P, of dNk at
// dNk + r*K).  Workgroup b of a launch adds into replica b % kDeltaReps: at the end of a short
// launch every workgroup flushes its histogram at the same moment, and device-scope atomics on one
// word serialise (about 12 ns each), so 250 workgroups on the same 1-2 k words cost microseconds;
// eight replicas cut the queue per word eightfold.  Consumers sum (and clear) the replicas.
#ifndef BMM_DELTA_REPS
#define BMM_DELTA_REPS 8
#endif
constexpr int kDeltaReps = BMM_DELTA_REPS;
__device__ __forceinline__ int32_t delta_take(int32_t* d, size_t idx, size_t stride) {
    int32_t v[kDeltaReps];
#pragma unroll
    for (int r = 0; r < kDeltaReps; ++r) v[r] = d[idx + r * stride];  // independent loads, one round trip
    int32_t t = 0;
#pragma unroll
    for (int r = 0; r < kDeltaReps; ++r) t += v[r];
    return t;
}
__device__ __forceinline__ void delta_clear(int32_t* d, size_t idx, size_t stride) {
#pragma unroll
    for (int r = 0; r < kDeltaReps; ++r) d[idx + r * stride] = 0;
}

// update_alpha_ (bmm_spec.h) with its four gamma variates -- independent Philox streams by construction --
// drawn by lanes 0..3 of one wave side by side instead of one after the other (each is a rejection loop
// of logs and square roots: about 1.5 us of latency apiece for a single lane); lane 0 combines them with
// the very operations of the serial form, so the result is bit-identical.  Call with the whole wave;
// the value is valid on lane 0.
__device__ __forceinline__ double update_alpha_wave(double alpha_old, double a, double b, double N, int K,
                                                    uint64_t seed, uint32_t sweep, int lane) {
    double g = 0.0;
    if (lane < 4) {
        const double shape = lane == 0 ? alpha_old + 1.0 : (lane == 1 ? N : (lane == 2 ? a + (double)K : a + (double)K - 1.0));
        Stream st = make_stream(seed, lane == 1 ? 1u : 0u, sweep,
                                lane < 2 ? kStreamAlphaEta : (lane == 2 ? kStreamAlphaG1 : kStreamAlphaG2));
        g = rgamma_(shape, st);
    }
    const double x = __shfl(g, 0), y = __shfl(g, 1), g1 = __shfl(g, 2), g2 = __shfl(g, 3);
    // rbeta_'s quotient.  Its fallback for two gammas that both flushed to 0 cannot be reached here: the shapes are
    // alpha_old + 1 >= 1 and N >= 1, and a gamma of shape >= 1 has no boost to underflow.
    const double eta = div_(x, x + y);
    const double b_eps = b - log_(eta);
    const double pi1 = a + (double)K - 1.0;
    const double pi2 = N * b_eps;
    const double pi = div_(pi1, pi1 + pi2);
    const double scale = div_(1.0, b_eps);
    const double ga = g1 * scale;
    const double gb = g2 * scale;
    return pi * ga + (1.0 - pi) * gb;
}

// ---------------------------------------------------------------------------------
// Table construction: one workgroup per category.  For the counting samplers it first
// folds the pending integer deltas of its cluster into the statistics.
// ---------------------------------------------------------------------------------
// e1/e0 hold the `pc` features of one chunk; its `gc` groups start at global group g0
// `c` is the category's constant term: it goes into the entries of global group 0
// Tq (or null): the packed image behind the table image, Tq[G][KT/2][M] pairs of binary32 -- the very entries
// written to T, narrowed, categories 2j and 2j+1 side by side (k_resample_pk reads a pair in one ds_read_b64)
template <int W>
__device__ __forceinline__ void write_group_tables_w(const double* e1, const double* e0, int pc, int g0, int gc,
                                                   int KT, int k, double c, double* T, float* Tq = nullptr) {
    constexpr int M = 1 << W;
    for (int idx = threadIdx.x; idx < gc * M; idx += blockDim.x) {
        const int g = idx / M;
        const unsigned m = idx % M;
        const double t = group_entry(e1, e0, g, pc, m, W);
        const double v = g0 + g == 0 ? c + t : t;
        T[((size_t)(g0 + g) * KT + k) * M + m] = v;
        if (Tq) Tq[(((size_t)(g0 + g) * (KT / 2) + (k >> 1)) * M + m) * 2 + (k & 1)] = (float)v;
    }
}

// W = the shape's width (kGroupW or kGroupWAlt) or the own-cluster tables' kGroupWm; uniform
__device__ __forceinline__ void write_group_tables(int W, const double* e1, const double* e0, int pc, int c0,
                                                   int KT, int k, double c, double* T, float* Tq = nullptr) {
    const int g0 = c0 / W, gc = (pc + W - 1) / W;
    if (W == kGroupW) write_group_tables_w<kGroupW>(e1, e0, pc, g0, gc, KT, k, c, T, Tq);
    else if (W == kGroupWAlt) write_group_tables_w<kGroupWAlt>(e1, e0, pc, g0, gc, KT, k, c, T, Tq);
    else write_group_tables_w<kGroupWm>(e1, e0, pc, g0, gc, KT, k, c, T);
}

// The own-cluster image of the packed kernel, behind Tq: To[G][KT][M] binary32 -- the "observation removed" terms
// o1/o0 of one chunk grouped at the SHAPE's width W (kGroupW or kGroupWAlt; uniform), the constant c folded into global
// group 0 as Tm folds it, each binary64 sum narrowed once and stored nowhere else (k_resample_pk reads the entry with
// the field that indexes Tq).  A loop of its own: carried through the loop of write_group_tables_w, its arguments
// spilled SGPRs of k_count_tables<TAB_PLAIN>; so did what the compiler computed of it ahead of the chunk loop (the caller).
template <int W>
__device__ __forceinline__ void write_own32_w(const double* o1, const double* o0, int pc, int g0, int gc, int KT, int k,
                                              double c, float* To) {
    constexpr int M = 1 << W;
    for (int idx = threadIdx.x; idx < gc * M; idx += blockDim.x) {
        const int g = idx / M;
        const unsigned m = idx % M;
        const double t = group_entry(o1, o0, g, pc, m, W);
        To[((size_t)(g0 + g) * KT + k) * M + m] = (float)(g0 + g == 0 ? c + t : t);
    }
}
__device__ __forceinline__ void write_own32(int W, const double* o1, const double* o0, int pc, int c0, int KT, int k,
                                            double c, float* To) {
    const int g0 = c0 / W, gc = (pc + W - 1) / W;
    if (W == kGroupW) write_own32_w<kGroupW>(o1, o0, pc, g0, gc, KT, k, c, To);
    else write_own32_w<kGroupWAlt>(o1, o0, pc, g0, gc, KT, k, c, To);
}

constexpr int kCountTablesThreads = 576;
// The table build of every counting chain, one body in five flavours.  A flavour changes expressions only where they
// stand below, behind `if constexpr` or a `?:` on a constant, so that each instantiation is the kernel that was once
// written out for it; the values a flavour alone needs are trailing kernel arguments that exist for it only.
//   TAB_PLAIN   the collapsed and the DP chain.  `packed`: the chain runs k_resample_pk and the packed image goes
//               behind this one.
//   TAB_MASK    feature selection: `mask` holds one inclusion bit per feature (word d / 32, bit
//               d % 32, the bits from P on zero).  An excluded feature's terms are written as 0 in all four roles -- it
//               scores the same for every category, so it drops out of the conditional -- and the DP's new-cluster
//               term counts the included features only.  The statistics are folded for every feature alike.  Never a
//               packed image (plan_kernel).
//   TAB_ALLOC   the allocation sampler (extra: Kact, a): the number of components is part of
//               the state, p.K is maxK and the first *Kact labels are open.  An open label scores with its prior
//               weight a and the prior Bernoulli terms when it is empty (the Dirichlet-multinomial model; the plain
//               build gives an empty label -inf for ever), and a row that sits alone keeps its own label at that
//               weight; a label from *Kact on is closed: -inf, tables zero.  `a` is the Dirichlet parameter per
//               component, the denominator log(N - 1 + K a).  alpha_ptr is not read.
//   TAB_TEMPER  a rung of a replica ladder (extra: b), target p(alpha) p(z | alpha) p(x | z)^b:
//               every per-feature term is multiplied once by the inverse temperature b after its denominator is
//               subtracted, in all four roles.  The category's constant (the allocation prior) is untouched; the DP's
//               new-cluster constant carries b on its P prior Bernoulli terms only.  The multiply sits behind the log_
//               of a term thread, off wave 8's chain of constants.
//   TAB_CAT     categorical features (extra: lev, P bytes): lev[d] = 0 marks a Bernoulli column,
//               computed as TAB_PLAIN computes it, operation for operation; lev[d] = L > 0 a column of a block of L
//               neighbouring one-hot columns, one feature of L levels under a symmetric Dirichlet(beta, ..., beta).  A row
//               has exactly one 1 in a block (k_cat_check), so the block's denominator rides on the x = 1 terms:
//               role 0 is log(beta + s) - log(L beta + n), role 2 log(beta + (s - 1)) - log(L beta + (n - 1)), and the
//               x = 0 terms, roles 1 and 3, are 0.  Their threads are idle and take the column's two denominators, so a
//               thread still has one log_ on its path.  The DP's new cluster counts the Bernoulli columns in the plain
//               expression and adds lb - log(L beta) per block, blocks in ascending column order (1 / L per feature).
//               Every entry stays <= 0, so a packed chain keeps its image (`packed`) and k_resample_pk.  One barrier more
//               than the other flavours, ahead of the chunk loop: behind it the cluster size is folded (Nk and dNk are
//               not carried through the loop) and wave 8 of the new cluster's workgroup adds the blocks.
// Every flavour folds and clears the deltas and writes the same image with the same roles and order of operations, so
// the resample kernels are the ones every chain runs, and these bit-equalities hold against TAB_PLAIN: TAB_MASK with a
// mask of all ones; TAB_TEMPER with b = 1 (x * 1.0 is x); TAB_ALLOC with no label empty or single and K a = alpha;
// TAB_CAT with lev all zero.
// The log terms are written out here; the kernel does not call the count-table rules of bmm_spec.h that
// build_tables_self and k_state_tables share.  One kernel template over those functions wrote the same bits but
// averaged 0.2 us (4 %) more per launch (profiles/r06/README.md), and this launch sits on every batch of every counting
// chain.
enum : int { TAB_PLAIN = 0, TAB_MASK = 1, TAB_ALLOC = 2, TAB_TEMPER = 3, TAB_CAT = 4 };
template <int I, class T, class... R>
__device__ __forceinline__ auto tab_extra(T t, R... r) {  // trailing kernel argument I
    if constexpr (I == 0) return t;
    else return tab_extra<I - 1>(r...);
}
// the LDS that TAB_CAT alone has (the other flavours' kernels hold none of it)
template <bool ON>
__device__ __forceinline__ double* tab_cat_lds() {
    if constexpr (ON) {
        __shared__ double a[256 + 2 * kMaxP];
        return a;
    } else {
        return nullptr;
    }
}
template <int F, class... Extra>
__global__ __launch_bounds__(kCountTablesThreads) void k_count_tables(ChainParams p, int32_t* __restrict__ Nk,
                                                                     int32_t* __restrict__ S,
                                                                     int32_t* __restrict__ dNk,
                                                                     int32_t* __restrict__ dS,
                                                                     const double* __restrict__ alpha_ptr,
                                                                     double* __restrict__ tab,
                                                                     const uint32_t* __restrict__ mask,
                                                                     int packed, Extra... extra) {
    constexpr bool MASK = F == TAB_MASK, ALLOC = F == TAB_ALLOC, TEMPER = F == TAB_TEMPER, CAT = F == TAB_CAT;
    __shared__ double e1[kMaxP], e0[kMaxP], m1[kMaxP], m0[kMaxP], cst[4];  // cst: Cp, Cm, the two denominators
    const int k = blockIdx.x;
    const TableLayout L = layout_of(p, true);
    // the chain runs k_resample_pk: the packed image goes behind this one (uniform)
    float* const Tq = (F == TAB_PLAIN || CAT) && packed ? reinterpret_cast<float*>(tab + L.doubles()) : nullptr;
    const int P = p.P;
    const bool is_label = k < p.K;
    int Ka = 0;            // ALLOC: the number of open labels, and the Dirichlet parameter
    double a = 0.0, b = 1.0;  // TEMPER: the inverse temperature
    if constexpr (ALLOC) { Ka = *tab_extra<0>(extra...); a = tab_extra<1>(extra...); }
    if constexpr (TEMPER) b = tab_extra<0>(extra...);
    const uint8_t* lev = nullptr;  // CAT: the block length of every column
    if constexpr (CAT) lev = tab_extra<0>(extra...);
    const bool open = k < Ka;
    // 576 threads, ONE log_ each on the critical path (a log_ is about 150 dependent instructions).  Waves
    // 0-7: role r = thread / 128 -- the term of feature d for x = 1 and for x = 0 against the full
    // statistics (r = 0, 1) and with the scored observation removed (r = 2, 3).  Wave 8: the cluster's
    // constants, one log per lane (the two denominators, the prior terms), combined by its lane 0 with the
    // operations of the serial form; the term threads subtract the denominators after a barrier.
    const int role = threadIdx.x >> 7;
    const int dl = role < 4 ? (threadIdx.x & 127) : kMaxP;
    // every load this workgroup depends on goes out first, in one round trip: the cluster size
    // (read by every thread: a broadcast, no LDS hand-over), the concentration, the first chunk of counts
    int32_t n_old = 0, n_dl = 0, s_old = 0, s_dl = 0;
    const size_t KP = (size_t)p.K * P;
    if (is_label) { n_old = Nk[k]; n_dl = delta_take(dNk, k, p.K); }
    if (is_label && dl < P) { s_old = S[(size_t)k * P + dl]; s_dl = delta_take(dS, (size_t)k * P + dl, KP); }
    int lv = 0;  // CAT: lev of this thread's column in the first chunk
    if constexpr (CAT) { if (is_label && dl < P) lv = lev[dl]; }
    const double alpha = ALLOC ? 0.0 : *alpha_ptr;
    const int64_t n = (int64_t)n_old + n_dl;
    const double bg = p.beta + p.gamma;
    // CAT, the DP's new cluster (its term threads have no term): log(L beta) for every L a block can have, one per thread
    const bool cat_new = CAT && p.mode == MODE_DP && k == p.K;
    double* const lgl = tab_cat_lds<CAT>();       // CAT: [256], then the columns' denominators dn[2][kMaxP]
    double* const dn = CAT ? lgl + 256 : nullptr;
    if constexpr (CAT) {
        if (cat_new && threadIdx.x >= 2 && threadIdx.x < 256) lgl[threadIdx.x] = log_((double)threadIdx.x * p.beta);
    }
    if (role == 4) {
        const int lane = threadIdx.x & 63;
        const bool dp_new = !ALLOC && p.mode == MODE_DP && k == p.K;
        const double ak = ALLOC ? a : p.mode == MODE_COLLAPSED ? div_(alpha, (double)p.K) : 0.0;
        double arg = 1.0;
        bool need = false;
        switch (lane) {  // (an open label of ALLOC takes its terms down to n = 0 and n - 1 = 0)
            case 0: arg = bg + (double)n; need = ALLOC ? open : is_label && n > 0; break;  // log(beta+gamma+n)
            case 1: arg = bg + (double)(n - 1); need = ALLOC ? open && n > 0 : is_label && n > 1; break;  // ... with one removed
            case 2: arg = (double)n + ak; need = ALLOC ? open : is_label && n > 0; break;  // log(n + alpha/K), log n, log(n + a)
            case 3: arg = (double)(n - 1) + ak; need = ALLOC ? open && n > 0 : is_label && n > 1; break;
            case 4: arg = (double)(p.Ntot - 1) + (ALLOC ? (double)Ka * a : alpha); need = true; break;  // log(N - 1 + alpha), ... + K a)
            case 5: arg = alpha; need = dp_new; break;
            case 6: arg = p.beta; need = dp_new; break;
            case 7: arg = bg; need = dp_new; break;
            default: break;
        }
        const double v = need ? log_(arg) : 0.0;
        int p_in = P;  // features that enter the conditional
        if (MASK) {
            p_in = 0;
            for (int w = lane; w < (P + 31) >> 5; w += 64) p_in += __popc(mask[w]);
            for (int o = 32; o > 0; o >>= 1) p_in += __shfl_xor(p_in, o);
        }
        const double den_p = __shfl(v, 0), den_m = __shfl(v, 1), ln = __shfl(v, 2), lm = __shfl(v, 3);
        const double ldN = __shfl(v, 4), la = __shfl(v, 5), lb = __shfl(v, 6), lbg = __shfl(v, 7);
        if (lane == 0) {
            double cp = neg_inf(), cm = neg_inf();
            if (ALLOC ? open : is_label) {
                if (ALLOC || n > 0) cp = ln - ldN;
                if (n > (ALLOC ? 0 : 1)) cm = lm - ldN;
            } else if (dp_new) {  // the prior of opening a cluster, then its (tempered) likelihood
                if constexpr (TEMPER) cp = (la - ldN) + b * ((double)P * (lb - lbg));
                else if constexpr (CAT) cp = la - ldN;  // the prior alone: the likelihood joins it behind the first barrier below
                else cp = (la - ldN) + (double)p_in * (lb - lbg);
            }
            tab[L.cp() + k] = cp;
            tab[L.cm() + k] = cm;
            cst[0] = cp; cst[1] = cm; cst[2] = den_p; cst[3] = den_m;  // read after the first barrier below
            reinterpret_cast<int32_t*>(tab + L.nk())[k] = (int32_t)n;
            if constexpr (CAT) { lgl[0] = lb; lgl[1] = lbg; }  // (threads 0 and 1 put no log there)
        }
    }
    if constexpr (CAT) {
        __syncthreads();  // lgl and cst are in place; every thread has read the old Nk and dNk
        if (is_label && threadIdx.x == 0) {  // (here, not behind the loop: the two pointers are not carried through it,
            Nk[k] = (int32_t)n;              // and the kernel has no scalar register to spare)
            delta_clear(dNk, k, p.K);
        }
        // the DP's new cluster, the likelihood of its constant: the plain expression over the Bernoulli columns, then
        // lb - log(L beta) per block, blocks in ascending column order.  Wave 8 walks the columns, 64 bytes of lev per
        // load; cst[0] is read behind the chunk loop's barriers.  (vz: a zero the compiler takes for a lane's own, so
        // that the walk's values live in vector registers.)
        if (cat_new && role == 4) {
            const int lane = threadIdx.x & 63;
            const int vz = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) - lane;
            const double lb = lgl[vz], lbg = lgl[vz + 1];
            int p_in = 0;
            for (int d = lane; d < P; d += 64) p_in += lev[d] == 0 ? 1 : 0;
            for (int o = 32; o > 0; o >>= 1) p_in += __shfl_xor(p_in, o);
            double cp = cst[vz] + (double)p_in * (lb - lbg);
            int skip = vz;
            for (int base = 0; base < P; base += 64) {
                const int mine = base + lane < P ? (int)lev[base + lane] : 0;
#pragma unroll 1
                for (int j = 0; j < 64; ++j) {  // (the columns from P on: 0, a step that adds nothing)
                    const int lj = __shfl(mine, j + vz);
                    const bool starts = skip == 0 && lj > 0;
                    cp = cp + (starts ? lb - lgl[lj] : 0.0);
                    skip = starts ? lj - 1 : (skip > 0 ? skip - 1 : 0);
                }
            }
            if (lane == 0) { tab[L.cp() + k] = cp; cst[0] = cp; }
        }
    }
    for (int c0 = 0; c0 < P; c0 += kChunkP) {  // kChunkP features (whole groups) at a time
        const int pc = P - c0 < kChunkP ? P - c0 : kChunkP;
        int32_t s = 0;
        double raw = 0.0;
        bool have = false;
        if (dl < pc && is_label) {
            const int d = c0 + dl;
            s = c0 == 0 ? s_old + s_dl : S[(size_t)k * P + d] + delta_take(dS, (size_t)k * P + d, KP);
            // term_x1 / term_x0 of bmm_spec.h, the denominator subtracted (and the power applied) below
            if constexpr (CAT) {
                // one log_ per thread, its argument picked by role and by the column's kind (no branch inside a branch: the
                // kernel has no scalar register to spare).  A one-hot column (cat_den_arg of bmm_spec.h): roles 1 and 3
                // have no term and take the column's two denominators.
                if (c0 != 0) lv = lev[d];
                const bool oh = lv > 0;
                const double lbeta = (double)lv * p.beta;
                double arg;
                if (role == 0) { have = n > 0; arg = p.beta + (double)s; }
                else if (role == 1) { have = n > 0; arg = oh ? lbeta + (double)n : (p.gamma + (double)n) - (double)s; }
                else if (role == 2) { have = n > 1 && s >= 1; arg = p.beta + (double)((int64_t)s - 1); }
                else { have = n > 1 && (oh || s <= n - 1); arg = oh ? lbeta + (double)(n - 1) : (p.gamma + (double)(n - 1)) - (double)s; }
                const double lg = log_(have ? arg : 1.0);
                raw = have ? lg : 0.0;
                if (oh && (role & 1)) { dn[(role >> 1) * kMaxP + dl] = raw; have = false; }
            } else
            if (role == 0) { have = ALLOC ? open : n > 0; raw = have ? log_(p.beta + (double)s) : 0.0; }
            else if (role == 1) { have = ALLOC ? open : n > 0; raw = have ? log_((p.gamma + (double)n) - (double)s) : 0.0; }
            else if (role == 2) { have = (ALLOC ? open && n > 0 : n > 1) && s >= 1; raw = have ? log_(p.beta + (double)((int64_t)s - 1)) : 0.0; }
            else { have = (ALLOC ? open && n > 0 : n > 1) && s <= n - 1; raw = have ? log_((p.gamma + (double)(n - 1)) - (double)s) : 0.0; }
        }
        __syncthreads();  // the constants are in place; every role has read S + dS before either is rewritten
        if (dl < pc) {
            double t = have ? (TEMPER ? b * (raw - cst[role < 2 ? 2 : 3]) : raw - cst[role < 2 ? 2 : 3]) : 0.0;
            if constexpr (CAT) t = have ? raw - (lv > 0 ? dn[(role >> 1) * kMaxP + dl] : cst[role < 2 ? 2 : 3]) : 0.0;
            if (MASK && !((mask[(c0 + dl) >> 5] >> ((c0 + dl) & 31)) & 1u)) t = 0.0;
            (role == 0 ? e1 : role == 1 ? e0 : role == 2 ? m1 : m0)[dl] = t;
            if (role == 0 && is_label) {
                const int d = c0 + dl;
                S[(size_t)k * P + d] = s;
                delta_clear(dS, (size_t)k * P + d, KP);
            }
        }
        __syncthreads();
        write_group_tables(p.W, e1, e0, pc, c0, p.KT, k, cst[0], tab + L.tp(), Tq);
        write_group_tables(kGroupWm, m1, m0, pc, c0, p.KT, k, cst[1], tab + L.tm());
        if (Tq) {  // Tm32, behind Tq
            int w = p.W, kt = p.KT, g = p.G;
            asm volatile("" : "+s"(w), "+s"(kt), "+s"(g));  // nothing of this block is computed ahead of the loop (SGPRs)
            write_own32(w, m1, m0, pc, c0, kt, k, cst[1], Tq + ((size_t)g * kt << w));  // Tq is G * KT * 2^W floats
        }
        __syncthreads();
    }
    if (!CAT && is_label && threadIdx.x == 0) {  // every thread read the old pair before the barriers above
        Nk[k] = (int32_t)n;
        delta_clear(dNk, k, p.K);
    }
    if (k == 0 && threadIdx.x < 256) tab[L.et() + threadIdx.x] = exp256_table()[threadIdx.x];
}

// Categorical features: every row of the resident bit planes has exactly one bit set in every
// block -- k_count_tables<TAB_CAT> scores a row on that footing, and a row with two bits, or none, would be scored
// without a word.  A thread per row (grid-stride); a block may straddle plane words; the blocks ascend, so a row's first
// bad block is the first one met.  The smallest (row, feature) key over all rows lands in *first_bad (all ones: clean).
struct CatBlock { int32_t col, len, feature; };
constexpr int kCatKeyBits = 20;  // features per key
__global__ __launch_bounds__(256) void k_cat_check(const uint32_t* __restrict__ Xb, int64_t N,
                                                   const CatBlock* __restrict__ blocks, int nb,
                                                   unsigned long long* __restrict__ first_bad) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        for (int q = 0; q < nb; ++q) {
            const CatBlock b = blocks[q];
            const int end = b.col + b.len;  // one past the block's last column
            int ones = 0;
            for (int w = b.col >> 5; w <= (end - 1) >> 5; ++w) {
                const int lo = b.col > 32 * w ? b.col - 32 * w : 0;
                const int hi = end - 32 * w < 32 ? end - 32 * w : 32;  // bits [lo, hi) of word w
                const uint32_t m = (hi - lo == 32 ? ~0u : (1u << (hi - lo)) - 1u) << lo;
                ones += __popc(Xb[(int64_t)w * N + i] & m);
            }
            if (ones != 1) {
                atomicMin(first_bad, ((unsigned long long)i << kCatKeyBits) | (unsigned long long)b.feature);
                break;
            }
        }
    }
}

// One half of a Beta draw split over two threads, as k_sb_theta_tables draws theta: half 0 draws X ~ Gamma(shape) on
// stream kStreamThetaA of counter word c0, half 1 draws Y on kStreamThetaB.  The draws are logged (rgamma_draw_<true>,
// bmm_spec.h), so that rbeta_join_ of the two halves is rbeta_ bit for bit, its underflow fallback included.
__device__ __forceinline__ double sb_theta_half(uint64_t seed, uint32_t c0, uint32_t sweep, int half, double shape) {
    Stream st = make_stream(seed, c0, sweep, half ? kStreamThetaB : kStreamThetaA);
    return rgamma_draw_<true>(shape, st);
}

// Stick-breaking: theta_kd ~ Beta(beta + V_kd, gamma + c_k - V_kd) (stickbreaking.cpp:217-229),
// unless draw == 0 (initial theta is used as given), then the tables of cluster k.
__global__ __launch_bounds__(256) void k_sb_theta_tables(ChainParams p, const int32_t* __restrict__ Nk,
                                                         const int32_t* __restrict__ S,
                                                         const double* __restrict__ pi,
                                                         double* __restrict__ theta, int draw,
                                                         uint32_t sweep, double* __restrict__ theta_trace,
                                                         double* __restrict__ tab,
                                                         double* __restrict__ alpha_ptr,
                                                         double* __restrict__ alpha_trace,
                                                         const int* __restrict__ viable) {
    // 256 threads: a Beta draw is X / (X + Y) of two gammas on their own streams, so threads 0-127 draw
    // X and log theta for feature d while threads 128-255 draw Y and log(1 - theta): half the latency
    __shared__ double e1[kMaxP], e0[kMaxP], gam[2][kMaxP], cst;
    if (blockIdx.x == (unsigned)p.KT) {
        // one workgroup past the clusters' (launched with the draws of a sweep only): the concentration, four
        // gammas side by side (update_alpha_wave; stickbreaking.cpp:233-235, full_gibbs.cpp:228-230), from the count
        // k_sb_params left.  Nothing in this kernel reads alpha; the next sweep's k_sb_params does.
        if (threadIdx.x < 64) {
            const double alpha_prev = *alpha_ptr;
            double alpha_new = alpha_prev;
            if (p.sample_alpha)
                alpha_new = update_alpha_wave(alpha_prev, p.a, p.b, (double)p.Ntot, *viable, p.seed, sweep, threadIdx.x);
            if (threadIdx.x == 0) {
                if (p.sample_alpha) *alpha_ptr = alpha_new;
                if (alpha_trace) *alpha_trace = alpha_new;
            }
        }
        return;
    }
    const int k = blockIdx.x;
    const TableLayout L = layout_of(p, false);
    const int P = p.P, K = p.K;
    const bool is_label = k < K;
    const int half = threadIdx.x >> 7, dl = threadIdx.x & 127;
    if (threadIdx.x == 255) {  // the constants, ahead of its own feature (if P reaches 128)
        cst = is_label ? log_(pi[k]) : neg_inf();  // read after the barriers below
        tab[L.cp() + k] = cst;
        tab[L.cm() + k] = neg_inf();
        reinterpret_cast<int32_t*>(tab + L.nk())[k] = is_label ? Nk[k] : 0;
    }
    for (int c0 = 0; c0 < P; c0 += kChunkP) {
        const int pc = P - c0 < kChunkP ? P - c0 : kChunkP;
        const int d = c0 + dl;
        if (draw && is_label && dl < pc) {
            const int32_t ck = Nk[k], V = S[(size_t)k * P + d];
            const uint32_t c0s = (uint32_t)((size_t)k * P + d);
            gam[half][dl] = sb_theta_half(p.seed, c0s, sweep, half,
                                          half ? (p.gamma + (double)ck) - (double)V : p.beta + (double)V);
        }
        __syncthreads();
        if (dl < pc) {
            double t = 0.0;
            if (is_label) {
                const double th = draw ? rbeta_join_(gam[0][dl], gam[1][dl]) : theta[k + (size_t)d * K];  // rbeta_
                if (half == 0) {
                    if (draw) theta[k + (size_t)d * K] = th;
                    if (theta_trace) theta_trace[k + (size_t)d * K] = th;
                    t = log_(th);
                } else {
                    t = log_(1.0 - th);
                }
            }
            if (half == 0) e1[dl] = t; else e0[dl] = t;
        }
        __syncthreads();
        write_group_tables(p.W, e1, e0, pc, c0, p.KT, k, cst, tab + L.tp());
        __syncthreads();
    }
    if (k == 0) tab[L.et() + threadIdx.x] = exp256_table()[threadIdx.x];  // 256 threads
}

// Stick-breaking: fold deltas, v_k ~ Beta(1 + c_k, alpha + sum_{l>k} c_l), pi by stick
// breaking, K_viable, alpha (stickbreaking.cpp:164-214, 233-235).  One workgroup.
__global__ __launch_bounds__(1024) void k_sb_params(ChainParams p, int32_t* __restrict__ Nk,
                                                   int32_t* __restrict__ S, int32_t* __restrict__ dNk,
                                                   int32_t* __restrict__ dS, const double* __restrict__ alpha_ptr,
                                                   double* __restrict__ pi, uint32_t sweep,
                                                   double* __restrict__ pi_trace, int pi_stride,
                                                   int* __restrict__ viable_out,
                                                   int32_t* __restrict__ nk_trace) {
    __shared__ int32_t ck[kMaxCatsAny];
    __shared__ double v[kMaxCatsAny];
    const int K = p.K, P = p.P;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const int32_t n = Nk[k] + delta_take(dNk, k, K);
        Nk[k] = n; delta_clear(dNk, k, K); ck[k] = n;
        if (nk_trace) nk_trace[k] = n;
    }
    __syncthreads();
    const double alpha_prev = *alpha_ptr;
    // the first wave draws the sticks (they need the cluster sizes only) while the others fold the
    // feature counts, which only the next kernel reads
    const int nfold = blockDim.x > 64 ? blockDim.x - 64 : blockDim.x;
    const int t0 = blockDim.x > 64 ? (int)threadIdx.x - 64 : (int)threadIdx.x;
    for (int idx = t0 < 0 ? K * P : t0; idx < K * P; idx += nfold) {
        S[idx] += delta_take(dS, idx, (size_t)K * P); delta_clear(dS, idx, (size_t)K * P);
    }
    const int ndraw = blockDim.x > 64 ? 64 : blockDim.x;
    for (int k = threadIdx.x < (unsigned)ndraw ? threadIdx.x : K; k < K; k += ndraw) {
        Stream sa = make_stream(p.seed, (uint32_t)k, sweep, kStreamStickA);
        if (p.mode == MODE_FULL) {
            // pi ~ Dirichlet(alpha/K + c_k) through gammas (full_gibbs.cpp:10-27, 203-210)
            v[k] = rgamma_(div_(alpha_prev, (double)K) + (double)ck[k], sa);
        } else {
            int64_t prev = 0;
            for (int l = k + 1; l < K; ++l) prev += ck[l];
            Stream sb = make_stream(p.seed, (uint32_t)k, sweep, kStreamStickB);
            v[k] = rbeta_(1.0 + (double)ck[k], alpha_prev + (double)prev, sa, sb);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int viable = 0;
        if (p.mode == MODE_FULL) {
            double sum_term = 0.0;
            for (int k = 0; k < K; ++k) sum_term = sum_term + v[k];
            for (int k = 0; k < K; ++k) {
                const double pk = div_(v[k], sum_term);
                pi[k] = pk;
                if (pi_trace) pi_trace[(size_t)k * pi_stride] = pk;
            }
            viable = K;  // update_alpha(..., N, K) at full_gibbs.cpp:228-230
        } else {
            v[K - 1] = 1.0;
            double cumprod = 1.0;
            for (int k = 0; k < K; ++k) {
                const double pk = k == 0 ? v[0] : cumprod * v[k];
                if (pk > 0.01) ++viable;
                cumprod = k == 0 ? 1.0 - v[0] : cumprod * (1.0 - v[k]);
                pi[k] = pk;
                if (pi_trace) pi_trace[(size_t)k * pi_stride] = pk;
            }
        }
        // the concentration's update needs this count and nothing else of the sweep: it runs beside the theta
        // draws, in a workgroup of its own of the next kernel (k_sb_theta_tables), off this kernel's critical path
        *viable_out = viable;
    }
}

// Fold replicas 1.. of the delta accumulators into replica 0 and clear them: ahead of anything that
// hands the deltas to the host or to a collective (bmm_chain_get_counts, bmm_chain_shard_deltas).
__global__ __launch_bounds__(256) void k_reduce_deltas(ChainParams p, int32_t* __restrict__ dNk,
                                                       int32_t* __restrict__ dS) {
    const int KP = p.K * p.P;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= KP + p.K) return;
    int32_t* d = idx < KP ? dS : dNk;
    const size_t i = idx < KP ? idx : idx - KP, stride = idx < KP ? KP : p.K;
    const int32_t v = delta_take(d, i, stride);
    delta_clear(d, i, stride);
    d[i] = v;
}

// Counting samplers, end of sweep: fold what the last batch left, theta-hat = S/Nk
// (NaN for an empty cluster in the finite sampler, 0 for an unused DP label), alpha.
__global__ __launch_bounds__(1024) void k_count_sweep_end(ChainParams p, int32_t* __restrict__ Nk,
                                                         int32_t* __restrict__ S,
                                                         int32_t* __restrict__ dNk,
                                                         int32_t* __restrict__ dS,
                                                         double* __restrict__ alpha_ptr, uint32_t sweep,
                                                         double* __restrict__ theta_trace,
                                                         double* __restrict__ alpha_trace,
                                                         int32_t* __restrict__ nk_trace) {
    __shared__ int32_t nk[kMaxCatsAny];
    const int K = p.K, P = p.P;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const int32_t n = Nk[k] + delta_take(dNk, k, K);
        Nk[k] = n; delta_clear(dNk, k, K); nk[k] = n;
        if (nk_trace) nk_trace[k] = n;
    }
    __syncthreads();
    // the first wave draws alpha (below) while the others fold the counts
    const int nfold = blockDim.x > 64 ? blockDim.x - 64 : blockDim.x;
    const int t0 = blockDim.x > 64 ? (int)threadIdx.x - 64 : (int)threadIdx.x;
    for (int idx = t0 < 0 ? K * P : t0; idx < K * P; idx += nfold) {
        const int k = idx / P, d = idx % P;
        const int32_t s = S[idx] + delta_take(dS, idx, (size_t)K * P);
        S[idx] = s; delta_clear(dS, idx, (size_t)K * P);
        if (theta_trace) {
            double t;
            if (p.mode == MODE_DP && nk[k] == 0) t = 0.0;
            else t = div_((double)s, (double)nk[k]);
            theta_trace[k + d * K] = t;
        }
    }
    if (threadIdx.x < 64) {  // the first wave: the concentration, four gammas side by side
        double al = *alpha_ptr;
        if (p.sample_alpha) {
            int Kc = K;
            if (p.mode == MODE_DP) { Kc = 0; for (int k = 0; k < K; ++k) Kc += nk[k] > 0; }
            al = update_alpha_wave(al, p.a, p.b, (double)p.Ntot, Kc, p.seed, sweep, threadIdx.x);
        }
        if (threadIdx.x == 0) {
            if (p.sample_alpha) *alpha_ptr = al;
            if (alpha_trace) *alpha_trace = al;
        }
    }
}

// ---------------------------------------------------------------------------------
// The z-resample kernel.
// ---------------------------------------------------------------------------------
struct ResampleArgs {
    const int32_t* X;
    const uint32_t* Xb;    // bit planes of X: word w of observation i at Xb[w * N + i] (k_pack_bits)
    const int32_t* z_in;   // 0-based labels of the previous sweep, -1 = unassigned
    int32_t* z_out;
    const double* tab;     // table image (TableLayout)
    int32_t* dNk;          // global delta accumulators
    int32_t* dS;
    int64_t lo, hi;        // batch [lo, hi)
    uint32_t sweep;
    int minus_in_lds;      // 1: the Tm tables were sized into LDS too
    double* wts;           // or null: this sweep also emits the draw's weights, wts[k * N + i] for the Kc
    double* wtot;          //   categories in order, and their total wtot[i] (k_probs_finish normalises)
    unsigned long long* diag;  // BMM_DIAG builds: [5] cycle sums (score, pack, draw, movers, prologue)
    int* dbg_flag;         // -DBMM_DEBUG_HOOKS builds: set when a kernel meets a label outside its range
    int dbg_inject;        //   ... and a test's way to make one (BMM_DEBUG_BADLABEL)
    // SELF kernels (workgroups that build their own table image): the folded statistics, the deltas the previous
    // launch left (dNk / dS above are the set this launch flushes into), the concentration, and the count of
    // workgroups that have read all of that (self_fold_prev)
    int32_t* Nk;
    int32_t* S;
    int32_t* dNk_prev;
    int32_t* dS_prev;
    const double* alpha_ptr;
    int* self_done;
    // k_resample_pk, test variant: its counters [draws, deferred, of the deferred those the packed tier left uncertain
    // and BMM_DEBUG_PK_DEFER_EVERY did not select], and BMM_DEBUG_PK_DEFER_EVERY (n > 0: a lane whose observation index
    // is a multiple of n counts as uncertain)
    // then the settle tiers' [runs of the middle tier, of them certain, runs of the definition], and
    // BMM_DEBUG_PK_MID_FAIL_EVERY (n > 0: the middle tier's verdict is dropped for observation indices that are multiples of n)
    unsigned long long* pk_stat;
#ifdef BMM_DEBUG_HOOKS
    int pk_defer_every;
    int pk_mid_fail_every;
#endif
};

// The test variant of the library (-DBMM_DEBUG_HOOKS) checks every label a resample kernel is about to count
// with: 0 <= new < K, -1 <= old < K.  The LDS histogram is indexed by label without a bound, so a wrong
// experimental kernel would otherwise scribble over LDS (round 2 lost a GPU call to exactly that).  A bad
// label raises the chain's flag -- the host turns it into BMM_E_STATE at the next synchronisation -- and the
// observation is left unassigned and uncounted.  The product build carries none of this.
#ifdef BMM_DEBUG_HOOKS
__device__ __forceinline__ void dbg_check_labels(const ResampleArgs& a, bool valid, bool first, int K, int& zn, int& zo) {
    if ((a.dbg_inject & 1) && valid && first) zn = K + 3;
    if (valid && (zn < 0 || zn >= K || zo < -1 || zo >= K)) {
        atomicOr(a.dbg_flag, 1);
        zn = -1; zo = -1;
    }
}
#define BMM_DBG_LABELS(a, valid, first, K, zn, zo) dbg_check_labels(a, valid, first, K, zn, zo)
// The two-tier draw of k_resample under test: BMM_DEBUG_DRAW_FALLBACK (bit 4) sends every wave to the binary64
// definition; BMM_DEBUG_DRAW_NOEPS (bit 8) gives the binary32 tier a band of width zero around the CDF entries, so
// that it answers for draws it cannot prove -- a test then sees that the band is what keeps the labels right.
#define DBG_TIER1_FORCE(a, certain) if ((a).dbg_inject & 4) certain = false
#define DBG_TIER1_EPS(a, eps) if ((a).dbg_inject & 8) eps = 0.0f
#else
#define BMM_DBG_LABELS(a, valid, first, K, zn, zo)
#define DBG_TIER1_FORCE(a, certain)
#define DBG_TIER1_EPS(a, eps)
#endif

// The running maximum of the scores in one v_max_f64 per score.  __builtin_fmax first quiets a signalling NaN in
// either operand (a v_max_f64 x, x apiece: twenty spare binary64 instructions per observation at K = 20), which a
// score, being a sum, never is; on every other operand, quiet NaNs included, the instruction alone is fmax.
__device__ __forceinline__ double max_score(double m, double sc) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(m), "v"(sc));
    return r;
}

// Where a lane sits in a tile of NT consecutive observations.  Lanes past the end of the
// batch re-read its last observation (and never write back).
struct TilePos {
    const char* base;   // wave-uniform byte address of X[wave_base + 0*N]
    uint32_t voff;      // this lane's byte offset from it (>= 0)
    int64_t i, ic;      // own observation, clamped observation
    bool valid;
};
__device__ __forceinline__ TilePos tile_pos(const ResampleArgs& a, int64_t tile, int NT, int tid, int lane) {
    TilePos t;
    const int64_t tile_base = a.lo + tile * NT;
    t.i = tile_base + tid;
    t.valid = t.i < a.hi;
    int64_t wave_base = tile_base + (int64_t)__builtin_amdgcn_readfirstlane(tid & ~63);  // SGPR
    wave_base = wave_base < a.hi ? wave_base : a.hi - 1;
    const int64_t room = a.hi - 1 - wave_base;
    const int lane_off = lane < room ? lane : (int)room;
    t.ic = wave_base + lane_off;
    t.voff = (uint32_t)lane_off * 4u;
    t.base = reinterpret_cast<const char*>(a.X + wave_base);
    return t;
}
// Issue the loads of bit-word wd (features 32*wd ...): 32 coalesced dword loads per lane,
// wave-uniform base + zero-extended 32-bit lane offset (global_load saddr form).
// buffer form: the descriptor (SGPRs) carries the wave-uniform column base and is advanced
// by the column stride between loads; the lane offset is one shared VGPR.  No per-load
// address registers: the STG loads of one stage are in flight from STG + 1 VGPRs.
// STG = features per pipeline stage (16 or 32 = 4 or 8 lookup groups); template parameter below

template <int STG>
__device__ __forceinline__ void issue_stage(const TilePos& t, int64_t N, int P, int h, uint32_t (&st)[STG]) {
    const int d0 = h * STG;
    const int nb = P - d0 < STG ? P - d0 : STG;
    const int64_t stride = N * 4;
    const char* col = t.base + (int64_t)d0 * stride;
    // a partial last stage loads whole groups of four only (the tail re-reads feature P-1: same
    // cache lines; pack_stage masks it off)
#pragma unroll
    for (int u0 = 0; u0 < STG; u0 += 4) {
        if (u0 < nb) {
#pragma unroll
            for (int u = u0; u < u0 + 4; ++u) {
                const __amdgpu_buffer_rsrc_t rsrc =
                    __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(col), 0, 0x7fffffff, 0x00020000);
                st[u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)t.voff, 0, 0);
                col += d0 + u + 1 < P ? stride : 0;
            }
        }
    }
}
template <int STG>
__device__ __forceinline__ uint32_t pack_stage(int P, int h, const uint32_t (&st)[STG]) {
    const int nb = P - h * STG < STG ? P - h * STG : STG;
    uint32_t v = 0;
#pragma unroll
    for (int u = 0; u < STG; ++u) v |= st[u] << u;  // X is validated to be 0/1 when it is set
    return nb >= 32 ? v : (v & ((1u << nb) - 1u));
}
// bits of stage h live in word h*STG/32 at bit (h*STG)%32
template <int STG>
__device__ __forceinline__ void put_stage(uint32_t v, int h, uint32_t& b0, uint32_t& b1, uint32_t& b2, uint32_t& b3) {
    const uint32_t sh = STG == 32 ? v : v << ((h & 1) * 16);
    const int w = STG == 32 ? h : h >> 1;
    b0 |= w == 0 ? sh : 0u;
    b1 |= w == 1 ? sh : 0u;
    b2 |= w == 2 ? sh : 0u;
    b3 |= w == 3 ? sh : 0u;
}
// Word w of the observation's 128-bit pattern (w uniform; past the last word: 0).  The field of lookup
// group g, bits [g*W, (g+1)*W), may straddle two words.
__device__ __forceinline__ uint32_t word_of(int w, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
    return w == 0 ? b0 : (w == 1 ? b1 : (w == 2 ? b2 : (w == 3 ? b3 : 0u)));
}

// Sufficient-statistic deltas of one wave's movers into the workgroup's LDS histogram (integer LDS
// atomics: order-independent, deterministic).  Cluster sizes: every mover lane adds its own +1 / -1.
// Feature counts, two forms chosen per wave by the number of movers:
//   few movers    one mover at a time by the whole wave: its bits broadcast by readlane, one feature
//                 per lane (conflict-free), about 40 instructions per mover;
//   many movers   every mover lane walks the set bits of its own words (LDS atomics resolve lanes that
//                 meet on a cell): about 10 instructions per set bit of the densest mover, whatever the
//                 number of movers -- the first sweeps from a random allocation, where all 64 lanes
//                 move, and samplers whose posteriors keep many observations undecided.
__device__ __forceinline__ void count_movers(bool moves, int zfrom, int zto, uint32_t b0, uint32_t b1,
                                             uint32_t b2, uint32_t b3, int32_t* hist, int K, int P, int lane) {
    unsigned long long movers = __ballot(moves);
    if (!movers) return;
    if (moves) {
        atomicAdd(&hist[K * P + zto], 1);
        if (zfrom >= 0) atomicAdd(&hist[K * P + zfrom], -1);
    }
    const int thr = P >= 16 ? P >> 3 : 2;
    if ((int)__popcll(movers) > thr) {  // uniform
        if (moves) {
            int32_t* const hn = hist + zto * P;
            int32_t* const ho = hist + (zfrom < 0 ? 0 : zfrom) * P;
            const int W = (P + 31) >> 5;
#pragma unroll 1
            for (int w = 0; w < W; ++w) {
                uint32_t bits = w == 0 ? b0 : (w == 1 ? b1 : (w == 2 ? b2 : b3));
                while (bits) {
                    const int d = (w << 5) + __ffs((int)bits) - 1;
                    bits &= bits - 1;
                    atomicAdd(&hn[d], 1);
                    if (zfrom >= 0) atomicAdd(&ho[d], -1);
                }
            }
        }
        return;
    }
    while (movers) {
        const int src = __ffsll((long long)movers) - 1;
        movers &= movers - 1;
        const int mzn = __builtin_amdgcn_readlane(zto, src);
        const int mzo = __builtin_amdgcn_readlane(zfrom, src);
        const uint32_t w0 = __builtin_amdgcn_readlane(b0, src), w1 = __builtin_amdgcn_readlane(b1, src);
        const uint32_t w2 = __builtin_amdgcn_readlane(b2, src), w3 = __builtin_amdgcn_readlane(b3, src);
        const uint32_t lo_w = lane < 32 ? w0 : w1, hi_w = lane < 32 ? w2 : w3;
        const int sh = lane & 31;
        if (lane < P && ((lo_w >> sh) & 1u)) {
            atomicAdd(&hist[mzn * P + lane], 1);
            if (mzo >= 0) atomicAdd(&hist[mzo * P + lane], -1);
        }
        if (lane + 64 < P && ((hi_w >> sh) & 1u)) {
            atomicAdd(&hist[mzn * P + lane + 64], 1);
            if (mzo >= 0) atomicAdd(&hist[mzo * P + lane + 64], -1);
        }
    }
}
__device__ __forceinline__ void flush_hist(const int32_t* hist, int K, int P, int32_t* dS, int32_t* dNk,
                                           int tid, int nt) {
    for (int i = tid; i < K * P + K; i += nt) {
        const int32_t v = hist[i];
        if (v != 0) {
            if (i < K * P) atomicAdd(&dS[i], v);
            else atomicAdd(&dNk[i - K * P], v);
        }
    }
}

// X as bit planes: word w of observation i (features 32w .. 32w+31, feature d at bit d % 32) at
// Xb[w * N + i]; bits past P are zero.  X is constant over the whole chain, so the resample kernel
// streams 4 * ceil(P / 32) bytes per observation and sweep instead of 4 * P.
__global__ __launch_bounds__(256) void k_pack_bits(const int32_t* __restrict__ X, int64_t rows, int64_t ldx,
                                                   int P, uint32_t* __restrict__ Xb, int64_t N) {
    // X: `rows` observations, feature d of observation i at X[i + d * ldx]; Xb already offset to the
    // first of them, planes N words apart
    const int W = (P + 31) / 32;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows; i += (int64_t)gridDim.x * 256) {
        for (int w = 0; w < W; ++w) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int d = w * 32 + j;
                if (d < P) v |= ((uint32_t)X[i + (int64_t)d * ldx] & 1u) << j;
            }
            Xb[(int64_t)w * N + i] = v;
        }
    }
}
// the (up to four) words of observation i; W = ceil(P / 32) is wave-uniform
__device__ __forceinline__ void load_words(const uint32_t* Xb, int64_t N, int W, int64_t i, uint32_t& w0,
                                           uint32_t& w1, uint32_t& w2, uint32_t& w3) {
    w0 = Xb[i];
    w1 = W > 1 ? Xb[N + i] : 0u;
    w2 = W > 2 ? Xb[2 * N + i] : 0u;
    w3 = W > 3 ? Xb[3 * N + i] : 0u;
}

// One pass over X when it is handed over: every cell must be 0 or 1 (the packing above
// shifts the loaded words without masking).  flag[0] is set when one is not.
__global__ __launch_bounds__(256) void k_validate_binary(const uint4* __restrict__ X4, int64_t n16,
                                                         const uint32_t* __restrict__ X, int64_t n,
                                                         int* __restrict__ flag) {
    uint32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
        const uint4 v = X4[i];
        bad |= (v.x | v.y | v.z | v.w) & ~1u;
    }
    for (int64_t i = n16 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        bad |= X[i] & ~1u;
    if (__any(bad != 0) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// Statistics of a given allocation (the collapsed sampler's initial labels,
// collapsed_gibbs.cpp:60-63): every labelled observation counts as arriving.
__global__ __launch_bounds__(256) void k_count_labels(ChainParams p, const int32_t* __restrict__ X,
                                                      const uint32_t* __restrict__ Xb,
                                                      const int32_t* __restrict__ z, int32_t* dNk,
                                                      int32_t* dS) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int32_t* const hist = reinterpret_cast<int32_t*>(smem);
    const int P = p.P, K = p.K, tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < K * P + K; i += 256) hist[i] = 0;
    __syncthreads();
    ResampleArgs a{};
    a.X = X; a.lo = 0; a.hi = p.N;
    const int64_t ntiles = (p.N + 255) / 256;
    const int nstages = (P + 15) / 16;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const TilePos pos = tile_pos(a, tile, 256, tid, lane);
        uint32_t st[16], b0 = 0, b1 = 0, b2 = 0, b3 = 0;
#pragma unroll
        for (int u = 0; u < 16; ++u) st[u] = 0;
        if (Xb) {  // bit planes (uniform)
            load_words(Xb, p.N, (P + 31) / 32, pos.ic, b0, b1, b2, b3);
        } else {
#pragma unroll 1
            for (int h = 0; h < nstages; ++h) {
                issue_stage<16>(pos, p.N, P, h, st);
                put_stage<16>(pack_stage<16>(P, h, st), h, b0, b1, b2, b3);
            }
        }
        const int zl = z[pos.ic];
        count_movers(pos.valid && zl >= 0, -1, zl, b0, b1, b2, b3, hist, K, P, lane);
    }
    __syncthreads();
    flush_hist(hist, K, P, dS + (size_t)(blockIdx.x % kDeltaReps) * K * P, dNk + (blockIdx.x % kDeltaReps) * K, tid, 256);
}

// Diagnostic build only (-DBMM_DIAG, never shipped): per-wave cycle stamps of the phases.
#ifdef BMM_DIAG
__device__ __forceinline__ unsigned long long diag_stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define DIAG(...) __VA_ARGS__
#else
#define DIAG(...)
#endif

// The z-resample kernel.  Software pipeline per wave, two levels:
//  * HBM: while tile t is scored, the STG loads of feature stage h of tile t+1 are in
//    flight; they are issued at the top of outer iteration h and packed at its bottom, after the
//    stage's own STG/4 lookup groups of tile t (nothing in flight is ever loop-carried);
//  * LDS: the K lookups of a group are issued together and added as they return (volatile:
//    one ds_read_b64 each -- the compiler would otherwise pair them into ds_read2_b64,
//    which moves half the bytes per clock).
// MINUS says where the own-cluster ("minus self") tables are: 0 none (stick-breaking),
// 1 in LDS, 2 in global memory.  It is a template parameter because a possible VMEM load in
// the lookup loop makes the compiler wait vmcnt(0) there, which would drain the HBM prefetch.
// SPLIT = 2 (bit planes only, for more than 32 accumulators): an observation is shared by lanes l
// and l + 32 of a wave, each scoring half of the categories -- half the accumulator registers per
// lane, so twice the waves per SIMD; the halves meet through three lane exchanges (maximum, running
// sum, count), all in the order the one-lane form uses, so the draw is bit-identical.
#ifndef BMM_LOOKUP_PRIO
#define BMM_LOOKUP_PRIO 2
#endif

// SELF: k_count_tables' work done by every resample workgroup for itself, straight into its LDS image -- for the
// finite sampler on shapes so small that the whole table build is at most two logs per thread (K (4P + 5) <= 2 NT:
// BASELINE config 2, K = 3, P = 20, is 255 logs: one per thread of a 256-thread workgroup; each further round of
// logs costs a launch about 2 us, and from the third on the table launch it replaces was cheaper).  Such shapes are bound by launches, not by work: a sweep of config 2
// is 8 table launches + 8 resample launches + 1, each a few microseconds, and this form drops the 8 table launches
// (every workgroup of a launch building the image of a bigger shape itself was measured in round 2: 8 000 logs per
// workgroup cost six times what the launch did).  The statistics are then folded by one of the launch's own
// workgroups (self_fold_prev, below).  The terms and constants are those of the count-table rules (bmm_spec.h) that
// k_count_tables evaluates, the entries those of write_group_tables: the image is bit-identical.
// scratch (LDS, doubles): terms [K][4][P] (x=1 / x=0 against the full statistics, then with the scored
// observation removed), logs [K][8], consts [KT][2] (Cp, Cm).
__host__ __device__ inline size_t self_scratch_doubles(int K, int KT, int P) { return (size_t)K * 4 * P + (size_t)K * 8 + (size_t)KT * 2; }
__host__ __device__ inline bool self_tables_fit(int mode, int K, int P, int threads) {
    return mode == MODE_COLLAPSED && P <= kChunkP && (long)K * (4 * P + 5) <= 2L * threads;
}
// SELF kernels read the statistics themselves when a workgroup starts -- Nk, S and the deltas of the previous
// launch -- so all three must stay as the previous launch left them until every workgroup of THIS launch has
// read them: a workgroup may start late (another chain's kernels on the device, another process), after others
// of its launch have already finished and flushed.  Two sets of delta accumulators therefore take turns: a
// launch flushes into the one that is empty and reads the other; each workgroup takes a ticket (a counter in
// global memory) once its reads are done, and the one that draws the last ticket -- nobody will read the old
// values again -- folds the previous launch's deltas into Nk and S and clears them, while the others are already
// scoring.  The host swaps the two sets after every such launch, so that to every other kernel (k_count_tables
// in a sweep that emits probabilities, k_count_sweep_end, the accessors) "the deltas" are the pending set as
// before and the other set is zero.  Integer sums: the result does not depend on who folds or when.
template <int NT>
__device__ __forceinline__ void self_fold_prev(const ResampleArgs& a, int K, int P, int tid) {
    const int KP = K * P;
    for (int i = tid; i < KP + K; i += NT) {
        if (i < KP) {
            const int32_t v = delta_take(a.dS_prev, (size_t)i, (size_t)KP);
            if (v != 0) a.S[i] += v;
            delta_clear(a.dS_prev, (size_t)i, (size_t)KP);
        } else {
            const int32_t v = delta_take(a.dNk_prev, (size_t)(i - KP), (size_t)K);
            if (v != 0) a.Nk[i - KP] += v;
            delta_clear(a.dNk_prev, (size_t)(i - KP), (size_t)K);
        }
    }
    if (tid == 0) *a.self_done = 0;  // every ticket of this launch has been drawn
}

template <int KT, int NT, int GW>
__device__ __forceinline__ void build_tables_self(const ChainParams& p, const ResampleArgs& a, const TableLayout& L,
                                                  double* lds, double* scratch, int tid, int* is_last) {
    constexpr int GM = 1 << GW;
    const int K = p.K, P = p.P;
    const size_t KP = (size_t)K * P;
    double* const terms = scratch;
    double* const logs = scratch + (size_t)K * 4 * P;
    double* const consts = logs + (size_t)K * 8;
    const CountRule r{BUILD_SELF, false, K, p.Ntot, p.beta, p.gamma, *a.alpha_ptr};  // the finite sampler's sweep
    const double ak = rule_ak(r);
    constexpr int kLogs = 5;  // the logs of const_arg a finite label needs (log 5 belongs to the DP's new cluster)
    const int nterm = K * 4 * P, nitem = nterm + K * kLogs;
    // phase A: every raw log, at most two per thread, held in registers across the barrier
    constexpr int R = 2;
    double raw[R];
    bool have[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int t = tid + q * NT;
        raw[q] = 0.0; have[q] = false;
        double arg;
        if (t < nterm) {
            const int k = t / (4 * P), role = (t / P) & 3, d = t % P;
            const int64_t n = (int64_t)a.Nk[k] + delta_take(a.dNk_prev, k, K);
            const int32_t sd = a.S[(size_t)k * P + d] + delta_take(a.dS_prev, (size_t)k * P + d, KP);
            have[q] = term_arg(r, k, role, n, sd, arg);
            raw[q] = have[q] ? log_(arg) : 0.0;  // the denominator is subtracted below
        } else if (t < nitem) {
            const int k = (t - nterm) / kLogs, lane = (t - nterm) % kLogs;
            const int64_t n = (int64_t)a.Nk[k] + delta_take(a.dNk_prev, k, K);
            logs[(size_t)k * 8 + lane] = const_arg(r, ak, k, n, lane, arg) ? log_(arg) : 0.0;
        }
    }
    __syncthreads();
    // phase B: the terms (denominator subtracted), the constants, the cluster sizes
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int t = tid + q * NT;
        if (t < nterm) {
            const int k = t / (4 * P), role = (t / P) & 3;
            terms[t] = term_of(have[q], raw[q], logs[(size_t)k * 8 + term_den(role)]);
        }
    }
    for (int k = tid; k < KT; k += NT) {
        double cp = neg_inf(), cm = neg_inf();
        int32_t n32 = 0;
        if (k < K) {
            const int64_t n = (int64_t)a.Nk[k] + delta_take(a.dNk_prev, k, K);
            const CatConsts c = cat_consts(r, k, n, logs + (size_t)k * 8);
            cp = c.cp; cm = c.cm;
            n32 = (int32_t)n;
        }
        consts[2 * k] = cp; consts[2 * k + 1] = cm;
        lds[L.cp() + k] = cp;
        lds[L.cm() + k] = cm;
        reinterpret_cast<int32_t*>(lds + L.nk())[k] = n32;
    }
    __syncthreads();
    // every read of the statistics is done: the ticket (self_fold_prev); its answer is needed only after phase C
    int ticket = 0;
    if (tid == 0) ticket = atomicAdd(a.self_done, 1);
    // phase C: the group tables, laid out as write_group_tables lays them out (constant folded into group 0;
    // accumulators past K score -inf; the own-cluster tables padded with zero groups)
    for (int idx = tid; idx < L.G * KT * GM; idx += NT) {
        const int g = idx / (KT * GM), k = (idx / GM) % KT;
        const unsigned m = idx % GM;
        const double t = k < K ? group_entry(terms + (size_t)(k * 4 + 0) * P, terms + (size_t)(k * 4 + 1) * P, g, P, m, GW) : 0.0;
        lds[L.tp() + ((size_t)g * KT + k) * GM + m] = g == 0 ? consts[2 * k] + t : t;
    }
    const int gm_used = (P + kGroupWm - 1) / kGroupWm;
    for (int idx = tid; idx < L.gm_pad() * KT * kGroupMm; idx += NT) {
        const int g = idx / (KT * kGroupMm), k = (idx / kGroupMm) % KT;
        const unsigned m = idx % kGroupMm;
        double v = 0.0;
        if (g < gm_used) {
            const double t = k < K ? group_entry(terms + (size_t)(k * 4 + 2) * P, terms + (size_t)(k * 4 + 3) * P, g, P, m, kGroupWm) : 0.0;
            v = g == 0 ? consts[2 * k + 1] + t : t;
        }
        lds[L.tm() + ((size_t)g * KT + k) * kGroupMm + m] = v;
    }
    if (tid == 0) *is_last = ticket == (int)gridDim.x - 1;
    for (int i = tid; i < 256; i += NT) lds[L.et() + i] = exp256_table()[i];
}

// EMIT: the launch also writes the draw's weights and their total (a.wts, a.wtot) for the probability
// hand-off to the host's relabelling; a twin instantiation, so that the plain kernel carries no branch.
// GW: features per lookup group of the tables (the shape's width, ChainParams::W).
template <int KT, int NT, int MINUS, int STG, bool BITS = false, int SPLIT = 1, bool EMIT = false, int GW = kGroupW, bool SELF = false>
__global__ __launch_bounds__(NT) void k_resample(ChainParams p, ResampleArgs a) {
    static_assert(!SELF || (MINUS == 1 && BITS && SPLIT == 1 && !EMIT), "self-built tables: the finite sampler's plain bit-plane kernel");
    constexpr int GM = 1 << GW;  // entries per group table
    // Bit planes, one lane per observation: a wave runs its scoring loop at raised priority.  Scoring is
    // bound by the CU's LDS pipe, the draw by the SIMD's VALU; with only four waves per SIMD the VALU
    // starves whenever all four sit in their scoring loops, so a scoring wave gets its few instructions in
    // ahead of the drawing waves (it stalls on LDS most of the time anyway) and leaves the loop sooner:
    // C5 +3.5 %, c3 +2.6 % over raising the priority for the issue of the reads only (which was +2 % over
    // none); the int32 pipeline and the two-lane form lose 1-3 % with it (profiles/r02/README.md).
    constexpr bool kPrioKernel = BITS && SPLIT == 1;
    // the draw tries binary32 first (below): the plain kernels with an observation's categories all in one lane
    constexpr bool kTier1 = SPLIT == 1 && !EMIT;
    static_assert(SPLIT == 1 || (SPLIT == 2 && BITS && MINUS != 2 && KT % 2 == 0), "split form");
    constexpr int SB = BITS ? 32 : STG;  // start bits of the lookup groups one stage scores
    constexpr int KH = KT / SPLIT;      // accumulators per lane
    constexpr int OT = NT / SPLIT;      // observations per tile
    constexpr int CH = SPLIT == 2 ? (KH <= 20 ? KH : KH / 2)
                                  : (KT <= 24 ? KT : (KT <= 48 ? KT / 2 : KT / 4));  // lookups issued together
    static_assert(KH % CH == 0, "chunking");
    DIAG(const unsigned long long d_entry = diag_stamp();)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool has_minus = MINUS != 0;
    const TableLayout L{p.G, KT, has_minus ? p.Gm : 0, GM};
    double* const lds = reinterpret_cast<double*>(smem);
    const int lds_doubles = MINUS == 1 ? L.doubles() : L.head();
    const volatile lds_f64* const Tp = (const volatile lds_f64*)(lds + L.tp());
    const lds_f64* const TmL = (const lds_f64*)(lds + L.tm());
    const double* const TmG = a.tab + L.tm();
    const int32_t* const NkT = reinterpret_cast<const int32_t*>(lds + L.nk());
    const lds_f64* const ET = (const lds_f64*)(lds + L.et());
    int32_t* const hist = reinterpret_cast<int32_t*>(lds + lds_doubles);  // [K*P] then [K]
    const int P = p.P, G = p.G, K = p.K;
    const int tid = threadIdx.x, lane = tid & 63;
    const int half = SPLIT == 2 ? lane >> 5 : 0;  // which half of the categories this lane scores
    const int kb = half * KH;
    // Work is handed out per wave, in chunks of OW consecutive observations: workgroup b owns the chunks
    // [b * cpw, (b + 1) * cpw) of the batch; a wave's first chunk is fixed (its loads go out before the
    // tables are staged), every further one comes from a counter in LDS -- the waves of a workgroup then
    // finish within one chunk of each other whatever order the SIMDs served them in.  The statistics are
    // integer sums and every label is stored by observation index, so results do not depend on who took what.
    constexpr int OW = 64 / SPLIT;
    constexpr int NW = NT / 64;  // waves per workgroup
    const int64_t nchunks = (a.hi - a.lo + OW - 1) / OW;
    const int64_t cpw = (nchunks + gridDim.x - 1) / gridDim.x;
    const int64_t wg_c0 = (int64_t)blockIdx.x * cpw;
    const int64_t wg_cn = nchunks - wg_c0 < cpw ? nchunks - wg_c0 : cpw;  // chunks of this workgroup (may be <= 0)
    (void)OT;
    auto tpos = [&](int64_t t) -> TilePos {
        if (SPLIT == 1) return tile_pos(a, t, 64, lane, lane);
        TilePos q;  // lanes l and l + 32 of a wave stand on the same observation
        q.i = a.lo + t * OW + (lane & 31);
        q.valid = q.i < a.hi;
        q.ic = q.valid ? q.i : a.hi - 1;
        q.voff = 0; q.base = nullptr;
        return q;
    };
    // BITS: X comes as bit planes; a "stage" is then one 32-bit word = eight lookup groups, all
    // (up to four) words of the next tile being loaded with the first stage
    const int W = (P + 31) / 32;
    const int nstages = BITS ? W : (P + STG - 1) / STG;

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int64_t tile = wg_c0 + wave;  // chunk index within the batch
    const bool has_tile = wave < wg_cn;
    int* const next_chunk = hist + K * P + K;  // LDS counter behind the histogram
    uint32_t st[STG];
#pragma unroll
    for (int u = 0; u < STG; ++u) st[u] = 0;
    TilePos pos = tpos(has_tile ? tile : 0);
    // first loads of the first tile go out before the tables are staged
    uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    if (has_tile) {
        if (BITS) load_words(a.Xb, p.N, W, pos.ic, b0, b1, b2, b3);
        else issue_stage<STG>(pos, p.N, P, 0, st);
    }
    if (SELF) {
#ifdef BMM_DEBUG_HOOKS
        // test variant, BMM_DEBUG_STRAGGLER: workgroup 0 starts about 100 us late, as it may on a device that other
        // work shares -- the others have flushed by then (tests/test_gpu_layouts.py)
        if ((a.dbg_inject & 2) && blockIdx.x == 0)
            for (int i = 0; i < 30; ++i) __builtin_amdgcn_s_sleep(127);
#endif
        // behind the histogram (and its chunk counter), on an 8-byte boundary
        double* const scratch = lds + lds_doubles + ((size_t)(K * P + K + 4) * sizeof(int32_t) + 7) / 8;
        build_tables_self<KT, NT, GW>(p, a, L, lds, scratch, tid, next_chunk + 1);  // (a spare word behind the counter)
    } else {
        // stage the table image: eight 16-byte loads in flight per lane (one L2 round trip per
        // eight, not per one)
        const double2* src = reinterpret_cast<const double2*>(a.tab);
        double2* dst = reinterpret_cast<double2*>(smem);
        const int n2 = lds_doubles / 2;
        for (int i0 = tid; i0 < n2; i0 += NT * 8) {
            double2 t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * NT;
                t[u] = src[i < n2 ? i : n2 - 1];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * NT;
                if (i < n2) dst[i] = t[u];
            }
        }
    }
    for (int i = tid; i < K * P + K; i += NT) hist[i] = 0;
    if (tid == 0) *next_chunk = NW;  // chunks 0 .. NW-1 of the workgroup are the waves' first ones
    __syncthreads();
    if (SELF && next_chunk[1]) self_fold_prev<NT>(a, K, P, tid);  // this workgroup was the last to read the statistics

    // DP bookkeeping shared by the whole batch (collapsed_gibbs_dp.cpp:166-171,212-231)
    int Kused = 0, new_label = -1;
    if (p.mode == MODE_DP) {
        for (int k = 0; k < K; ++k) {
            if (NkT[k] > 0) ++Kused;
            else if (new_label < 0) new_label = k;
        }
    }

    DIAG(unsigned long long d_ndraw = 0, d_nfall = 0;)
    DIAG(unsigned long long d_nmov = 0, d_ntile = 0; unsigned long long d_score = 0, d_pack = 0, d_draw = 0, d_mov = 0, d_pro = 0; unsigned long long d_t = diag_stamp(); const unsigned long long d_staged = d_t;)
    if (has_tile) {
        // prologue: the rest of the first tile's features, nothing to overlap with yet
        if (!BITS) put_stage<STG>(pack_stage<STG>(P, 0, st), 0, b0, b1, b2, b3);
        // no accumulators are live yet, so 64 loads share one round trip
#pragma unroll 1
        for (int h0 = 1; !BITS && h0 < nstages; h0 += 64 / STG) {
            uint32_t s0[STG], s1[STG], s2[STG], s3[STG];
#pragma unroll
            for (int u = 0; u < STG; ++u) { s0[u] = 0; s1[u] = 0; s2[u] = 0; s3[u] = 0; }
            issue_stage<STG>(pos, p.N, P, h0, s0);
            if (h0 + 1 < nstages) issue_stage<STG>(pos, p.N, P, h0 + 1, s1);
            if (STG == 16 && h0 + 2 < nstages) issue_stage<STG>(pos, p.N, P, h0 + 2, s2);
            if (STG == 16 && h0 + 3 < nstages) issue_stage<STG>(pos, p.N, P, h0 + 3, s3);
            put_stage<STG>(pack_stage<STG>(P, h0, s0), h0, b0, b1, b2, b3);
            if (h0 + 1 < nstages) put_stage<STG>(pack_stage<STG>(P, h0 + 1, s1), h0 + 1, b0, b1, b2, b3);
            if (STG == 16 && h0 + 2 < nstages) put_stage<STG>(pack_stage<STG>(P, h0 + 2, s2), h0 + 2, b0, b1, b2, b3);
            if (STG == 16 && h0 + 3 < nstages) put_stage<STG>(pack_stage<STG>(P, h0 + 3, s3), h0 + 3, b0, b1, b2, b3);
        }
        int zo = a.z_in ? a.z_in[pos.ic] : -1;
        asm volatile("" : "+v"(zo));  // land it before the pipeline starts: no load may be
                                      // pending at a loop header (the compiler would drain
                                      // vmcnt(0) at the first register reuse inside the loop)
        DIAG({ const unsigned long long n_ = diag_stamp(); d_pro += n_ - d_t; d_t = n_; })

        int zn_prev = 0;
        int64_t i_prev = -1;  // < 0: nothing to store yet
        for (;;) {
            const int zoc = zo < 0 ? 0 : zo;
            double acc_own = 0.0;
            if (MINUS != 0) {
                // the observation's own cluster is scored from the "minus self" tables: one entry per (narrow)
                // group, a per-lane gather -- from LDS (MINUS = 1), or from global memory when they are too big
                // to sit there beside Tp (MINUS = 2: L2-resident) -- before the accumulators are live, kOwnSub
                // groups per round: their fields are the low bits of a copy of the pattern that is shifted
                // down between rounds, their gathers are in flight together and summed in group order.  The
                // table image is padded with zero groups to whole rounds (bits past P are zero, so a padding
                // group adds its entry 0 = 0.0).
                uint32_t r0 = b0, r1 = b1, r2 = b2, r3 = b3;
                constexpr int RB = kOwnSub * kGroupWm;  // bits per round
                static_assert(RB < 32, "a round's fields come out of one word");
                const int rounds = (p.Gm + kOwnSub - 1) / kOwnSub;
                size_t at0 = (size_t)zoc * kGroupMm;
#pragma unroll 1
                for (int it = 0; it < rounds; ++it) {
                    double ow[kOwnSub];
#pragma unroll
                    for (int v = 0; v < kOwnSub; ++v) {
                        // v_bfe_u32 by hand: the compiler turns the bit-field extract into shift + and + add
                        // (three instructions where bfe + shift-add are two)
                        unsigned f;
                        asm("v_bfe_u32 %0, %1, %2, %3" : "=v"(f) : "v"(r0), "n"(v * kGroupWm), "n"(kGroupWm));
                        const size_t at = at0 + (size_t)v * KT * kGroupMm + f;
                        ow[v] = MINUS == 1 ? TmL[at] : TmG[at];
                    }
                    r0 = __builtin_amdgcn_alignbit(r1, r0, RB);
                    r1 = __builtin_amdgcn_alignbit(r2, r1, RB);
                    r2 = __builtin_amdgcn_alignbit(r3, r2, RB);
                    r3 >>= RB;
                    at0 += (size_t)kOwnSub * KT * kGroupMm;
#pragma unroll
                    for (int v = 0; v < kOwnSub; ++v) acc_own = acc_own + ow[v];
                }
            }
            // the previous tile's labels go out here, ahead of this iteration's stage loads in
            // the in-order VMEM stream (and behind the gathers above, whose wait would otherwise cover
            // a write round trip): a store still pending at the loop latch would make the compiler
            // wait vmcnt(0) there
            if (i_prev >= 0) a.z_out[i_prev] = zn_prev;
            int nc = 0;
            if (lane == 0) nc = atomicAdd(next_chunk, 1);
            nc = __builtin_amdgcn_readfirstlane(nc);
            const int64_t next = wg_c0 + nc;
            const bool has_next = nc < wg_cn;  // uniform
            const TilePos npos = tpos(has_next ? next : tile);
            uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
            int zo_next = -1;

            // ---- scoring: K * G conflict-free LDS lookups.  One outer iteration = one feature
            // stage: its loads for the NEXT tile are issued first, fly during the four lookup
            // groups of THIS tile, and are packed last -- nothing in flight is loop-carried.
            double acc[KH];
#pragma unroll
            for (int k = 0; k < KH; ++k) acc[k] = 0.0;
            if (kPrioKernel) __builtin_amdgcn_s_setprio(BMM_LOOKUP_PRIO);
#pragma unroll 1
            for (int h = 0; h < nstages; ++h) {
                if (has_next) {
                    if (BITS) { if (h == 0) load_words(a.Xb, p.N, W, npos.ic, n0, n1, n2, n3); }
                    else issue_stage<STG>(npos, p.N, P, h, st);
                }
                // the lookup groups whose first bit lies in this stage's span [SB*h, SB*(h+1)): one word
                // `cur` holds it, a field may run on into `nxt`
                const int wd = (SB * h) >> 5;
                const uint32_t cur = word_of(wd, b0, b1, b2, b3), nxt = word_of(wd + 1, b0, b1, b2, b3);
                // the next tile's previous labels ride along with its first stage
                if (has_next && h == 0 && a.z_in) zo_next = a.z_in[npos.ic];
                const int g_lo = (SB * h + GW - 1) / GW;
                int g_hi = (SB * (h + 1) + GW - 1) / GW;
                g_hi = g_hi < G ? g_hi : G;
#pragma unroll 1
                for (int g = g_lo; g < g_hi; ++g) {
                    const unsigned nib = __builtin_amdgcn_alignbit(nxt, cur, (unsigned)(g * GW - 32 * wd)) &
                                         (unsigned)(GM - 1);
                    const volatile lds_f64* row = Tp + (((size_t)g * KT + kb) * GM + nib);
#pragma unroll
                    for (int c0 = 0; c0 < KH; c0 += CH) {
                        double tv[CH];
#pragma unroll
                        for (int j = 0; j < CH; ++j) tv[j] = row[(c0 + j) * GM];
#pragma unroll
                        for (int j = 0; j < CH; ++j) acc[c0 + j] = acc[c0 + j] + tv[j];
                        if (CH < KH) __builtin_amdgcn_sched_barrier(0);  // keep the chunks apart
                    }
                }
                DIAG({ const unsigned long long n_ = diag_stamp(); d_score += n_ - d_t; d_t = n_; })
                if (!BITS && has_next) put_stage<STG>(pack_stage<STG>(P, h, st), h, n0, n1, n2, n3);
                DIAG({ const unsigned long long n_ = diag_stamp(); d_pack += n_ - d_t; d_t = n_; })
            }
            if (kPrioKernel) __builtin_amdgcn_s_setprio(0);
            // scores (the constant terms sit in group 0 of the tables); the observation's own
            // cluster is scored without itself
            double m = neg_inf();
#pragma unroll
            for (int k = 0; k < KH; ++k) {
                double sc = acc[k];
                if (has_minus && kb + k == zo) sc = acc_own;
                acc[k] = sc;
                m = max_score(m, sc);
            }
            if (SPLIT == 2) m = __builtin_fmax(m, __shfl_xor(m, 32));
            // u <= 1 - 2^-52, so u * tot < tot: the walk always ends on a category with weight
            const double u = z_uniform(p.seed, (uint64_t)(p.obs0 + pos.ic), a.sweep);
            // The draw is one integer, the count of CDF entries at or below u * tot.  The plain one-lane kernels
            // first take it from binary32 weights (draw_tier1, bmm_spec.h: hardware exp2, no table read), which also
            // says per lane whether that count is proven to be the definition's; when it is for every lane of the
            // wave the twenty binary64 exponentials below are not run at all.  Otherwise -- some lane's u * tot
            // within 2^-16 tot of a CDF entry, an impossible observation, a NaN -- the whole wave runs the
            // definition as before and every lane takes its result: a uniform branch, nothing per lane.
            bool tier1 = false;
            int cnt = 0;
            if constexpr (kTier1) {
                float eps = kTier1Eps;
                DBG_TIER1_EPS(a, eps);
                bool certain = draw_tier1<KH>(acc, m, u, eps, cnt);
                DBG_TIER1_FORCE(a, certain);
                tier1 = __ballot(!certain) == 0;
                DIAG(++d_ndraw; d_nfall += tier1 ? 0 : 1;)
            }
            if (!tier1) {
                // weights exp(score - max) and their running sum in label order; acc[k] becomes the CDF
                double run = 0.0;
#pragma unroll
                for (int k = 0; k < KH; ++k) {
                    const double w = expw_tab(acc[k] - m, ET);
                    if (EMIT && kb + k < p.Kc && pos.valid) a.wts[(int64_t)(kb + k) * p.N + pos.i] = w;
                    if (SPLIT == 1) { run = run + w; acc[k] = run; }
                    else acc[k] = w;
                    if ((k & 1) == 1) __builtin_amdgcn_sched_barrier(0);  // two at a time: bounds the temporaries
                }
                if (SPLIT == 2) {
                    // the running sum goes through the categories in label order: the upper half continues
                    // from the lower half's total
#pragma unroll
                    for (int k = 0; k < KH; ++k) run = run + acc[k];
                    const double lower = __shfl(run, lane & 31);
                    run = half ? lower : 0.0;
#pragma unroll
                    for (int k = 0; k < KH; ++k) { run = run + acc[k]; acc[k] = run; }
                    run = __shfl(run, (lane & 31) + 32);
                }
                const double tot = run;
                if (EMIT && half == 0 && pos.valid) a.wtot[pos.i] = tot;
                const double t = u * tot;
                cnt = 0;
#pragma unroll
                for (int k = 0; k < KH; ++k) cnt += t >= acc[k] ? 1 : 0;
                if (SPLIT == 2) cnt += __shfl_xor(cnt, 32);
            }
            int zn = cnt;
            if (!(m > neg_inf())) zn = zoc;  // every category impossible: keep (or 0)
            if (p.mode == MODE_DP && zn == K) {
                const int own_single = (zo >= 0 && NkT[zoc] == 1) ? 1 : 0;
                if (Kused - own_single < K - 1) {
                    zn = new_label;
                    if (own_single && (zn < 0 || zo < zn)) zn = zo;
                } else {
                    int best = -1, bs = 0;
                    for (int k = 0; k < K; ++k) {
                        const int sz = NkT[k] - (k == zo ? 1 : 0);
                        if (sz > 0 && (best < 0 || sz < bs)) { best = k; bs = sz; }
                    }
                    zn = best >= 0 ? best : zoc;
                }
            }
            DIAG({ const unsigned long long n_ = diag_stamp(); d_draw += n_ - d_t; d_t = n_; })

            BMM_DBG_LABELS(a, pos.valid, pos.i == a.lo, K, zn, zo);
            DIAG(d_nmov += __popcll(__ballot(pos.valid && zn >= 0 && zn != zo));)
            count_movers(pos.valid && half == 0 && zn >= 0 && zn != zo, zo, zn, b0, b1, b2, b3, hist, K, P, lane);
            DIAG({ const unsigned long long n_ = diag_stamp(); d_mov += n_ - d_t; d_t = n_; })

            zn_prev = zn;
            i_prev = pos.valid && half == 0 ? pos.i : -1;
            if (!has_next) break;
            b0 = n0; b1 = n1; b2 = n2; b3 = n3;
            zo = zo_next;
            pos = npos;
            tile = next;
        }
        if (i_prev >= 0) a.z_out[i_prev] = zn_prev;
    }

    DIAG(const unsigned long long d_loop = diag_stamp();)
    __syncthreads();
    DIAG(const unsigned long long d_sync = diag_stamp();)
    flush_hist(hist, K, P, a.dS + (size_t)(blockIdx.x % kDeltaReps) * K * P, a.dNk + (blockIdx.x % kDeltaReps) * K, tid, NT);
    DIAG(asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); const unsigned long long d_flush = diag_stamp();)
    DIAG(if (a.diag && lane == 0) {
        atomicAdd(&a.diag[0], d_score); atomicAdd(&a.diag[1], d_pack); atomicAdd(&a.diag[2], d_draw);
        atomicAdd(&a.diag[3], d_mov); atomicAdd(&a.diag[4], d_pro); atomicAdd(&a.diag[5], 1ull);
        atomicAdd(&a.diag[6], d_nmov);
        // per-launch phases of a wave: table staging, tile loop, wait for the workgroup, flush
        atomicAdd(&a.diag[8], d_staged - d_entry); atomicAdd(&a.diag[9], d_loop - d_staged);
        atomicAdd(&a.diag[10], d_sync - d_loop); atomicAdd(&a.diag[11], d_flush - d_sync);
        // the two-tier draw: draws of 64 observations a wave made, and how many of them ran the binary64 definition
        atomicAdd(&a.diag[12], d_ndraw); atomicAdd(&a.diag[13], d_nfall);
    })
}

// ---------------------------------------------------------------------------------
// k_resample_pk: the plain bit-plane kernel (one lane per observation) with every score summed in binary32.  The
// other categories come from the packed image Tq -- one ds_read_b64 and one v_pk_add_f32 per PAIR of categories and
// lookup group, half of k_resample's LDS and scoring VALU instructions -- and the observation's own cluster from
// Tm32, the "observation removed" entries at the same group width: one ds_read_b32 and one v_add_f32 per group, at
// the field the group step has already extracted for Tq.  The draw is draw_pk (bmm_spec.h), which says per lane
// whether its count is proven to be the definition's.  The lanes that are not certain are settled where they arise:
// right behind the draw the wave takes them one at a time and runs the binary64 definition on each (pk_exact_count:
// one lane per category, Tp and the width-3 Tm read from the global image, every load in flight at once), and the
// count goes into that lane, so the labels are k_resample's bit for bit.  From there on certain and settled lanes
// are the same: one count_movers, one pipelined store.  No phase follows the tile loop but the flush of the histogram.
// Since round 12 a middle tier stands ahead of the definition: pk_mid_count sums the lane's binary32 entries, which are
// in LDS, in binary64 (draw_mid, bmm_spec.h) and settles about six uncertain lanes in seven at C5 for 1 600 ticks
// instead of 8 900, at priority 3; the definition runs, unchanged, for the rest (profiles/r12/README.md).
// Settling is not free: measured at C5 (profiles/r08/README.md) a settled lane lengthens its wave's loop by about
// 8 800 cycles -- the definition is a chain of dependent binary64 steps; the SIMD's other waves take the issue slots
// meanwhile, but the workgroup's barrier waits for the wave that settled most -- and about half of the 12 us the pass
// behind the loop took per launch came back.
// The loop's steady state -- a chunk without an uncertain lane and without a mover -- moves no spilled scalar: the
// blocks beside it (pk_exact_count, pk_dp_label and its books, count_movers, the flush) take their arguments from the
// kernel argument segment where they run (pk_args_view: scalar loads behind an opaque pointer) and rebuild layout and
// LDS places from them, so none of that is held in scalar registers across the loop; their branches are marked
// unlikely, which keeps the register allocator's spills inside them.  An observation is a 32-bit offset from the
// launch's first (PkPos), the draw works on pairs (pk_draw2), and the Philox key is a scalar wherever the launch's
// indices allow (pk_uniform).  Instruction counts before and after: profiles/r09/README.md.
// PIPE: the second loop body, which the 1024-thread forms of up to 20 accumulators run (pk_pipelined; the name is
// round 10's, whose second body drew chunk i - 1 among the lookups of chunk i -- that measured as nothing and is
// gone).  It is the present body's trip in the present body's order with the lookups in unrolled steps at
// compile-time groups (pk_score: the field one v_bfe_u32, the rows instruction offsets) and the next chunk's place, its
// loads and this chunk's Philox rounds behind group 0's reads.  The
// present body is the other branch, unchanged, and every other form's.  profiles/r10/README.md, profiles/r11/README.md.
// LDS, in doubles: Tq [G][KT/2][M] pairs | Tm32 [G][KT][M] binary32 (the two as they lie behind the table image in
// global memory) | Nk, E (as they lie in the image) | histogram, chunk counter | kPkQueue words that nothing uses
// (pk_image_bytes, chain.hip).  The binary64 Tm is not staged.
// ---------------------------------------------------------------------------------
constexpr int kPkQueue = 4096;  // words reserved behind the counters and unused (pk_image_bytes, chain.hip)
typedef float pk_f2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) pk_f2 lds_pk_f2;
typedef __attribute__((address_space(3))) float lds_f32;
// the own-cluster tables' groups at the largest P, padded: one lane each in pk_exact_count
constexpr int kOwnPadMax = ((kMaxP + kGroupWm - 1) / kGroupWm + kOwnSub - 1) / kOwnSub * kOwnSub;
static_assert(kOwnPadMax <= 64, "pk_exact_count loads the own-cluster entries one per lane");

// the DP's bookkeeping for a draw of the new-cluster option (collapsed_gibbs_dp.cpp:212-231).  A second copy of the
// block under `if (p.mode == MODE_DP && zn == K)` in k_resample, which stays inline there so that its 370
// instantiations compile as they did: a fix to either belongs in both.
__device__ __forceinline__ int pk_dp_label(const int32_t* NkT, int K, int Kused, int new_label, int zo, int zoc) {
    const int own_single = (zo >= 0 && NkT[zoc] == 1) ? 1 : 0;
    if (Kused - own_single < K - 1) {
        int zn = new_label;
        if (own_single && (zn < 0 || zo < zn)) zn = zo;
        return zn;
    }
    int best = -1, bs = 0;
    for (int k = 0; k < K; ++k) {
        const int sz = NkT[k] - (k == zo ? 1 : 0);
        if (sz > 0 && (best < 0 || sz < bs)) { best = k; bs = sz; }
    }
    return best >= 0 ? best : zoc;
}
// bits [bit, bit + width) of the observation's 128-bit pattern (bit uniform)
__device__ __forceinline__ unsigned pk_field(int bit, unsigned mask, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
    const int wd = bit >> 5;
    return __builtin_amdgcn_alignbit(word_of(wd + 1, b0, b1, b2, b3), word_of(wd, b0, b1, b2, b3), (unsigned)(bit & 31)) & mask;
}

// lane j's binary64 value in every lane (j uniform): two v_readlane_b32, no trip through the LDS crossbar
__device__ __forceinline__ double pk_bcast(double x, int j) {
    const long long b = __double_as_longlong(x);
    const uint64_t e = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, j) |
                       ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), j) << 32);
    return __longlong_as_double((long long)e);
}

// The definition for one observation, by the whole wave; everything about the observation is wave-uniform and comes
// from the lane that holds it: its words w0..w3, its label zo, its uniform u.  Lane k scores category k -- the G
// entries of Tp from the global image (L2), added in group order; the own cluster from Tm in the global image too:
// lane l loads the entry of group l (gm_pad() <= kOwnPadMax lanes), and the entries are added in group order, padding
// groups included, lane by lane.  The loads of GR groups and the one of Tm are issued before the first is used: one
// round trip up to GR groups (twenty from 12 accumulators on: P <= 100 at groups of five), ceil(G / GR) beyond (a
// round's loads past G repeat the last group's and are not added).  Then the maximum, expw_ and the binary64 running sum walk the lanes in label order,
// each lane's value broadcast by v_readlane (pk_bcast).
// Every operation and its order are k_resample's.  Returns the count of the draw (the DP's new-cluster option is K:
// the caller keeps the books), or the label to keep where every category is impossible.
template <int KT, int GW>
__device__ __forceinline__ int pk_exact_count(const ChainParams& p, const ResampleArgs& a, const TableLayout& L,
                                              uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int zo, double u,
                                              const lds_f64* ET, int lane) {
    constexpr int GM = 1 << GW;
    // loads in flight, two VGPRs each, sized so that no form holds fewer waves per SIMD by registers than it did with
    // the pass behind the loop: the forms of up to 8 accumulators have few registers to spare (profiles/r08/README.md)
    constexpr int GR = KT <= 4 ? 6 : KT <= 8 ? 10 : 20;
    static_assert((kMaxP + GW - 1) / GW <= 64, "lane g holds the field of group g");
    const int G = p.G;
    const int zoc = zo < 0 ? 0 : zo;
    const int k = lane < KT ? lane : KT - 1;
    const double* const tp = a.tab + L.tp();
    const int gmp = L.gm_pad();
    const int go = lane < gmp ? lane : gmp - 1;
    const double oe = a.tab[L.tm() + ((size_t)go * KT + zoc) * kGroupMm + pk_field(go * kGroupWm, kGroupMm - 1, w0, w1, w2, w3)];
    // (the row of a group is uniform and the lane adds its category; lane g extracts the field of group g from the
    // uniform words with selects, and the groups read theirs from it: no scalar code that branches on the word)
    const unsigned koff = (unsigned)k * GM;
    const int gl = lane < G ? lane : G - 1;
    const int fld = (int)pk_field(gl * GW, GM - 1, w0, w1, w2, w3);
    double sc = 0.0;
#pragma unroll 1
    for (int g0 = 0; g0 < G; g0 += GR) {
        double tv[GR];
#pragma unroll
        for (int v = 0; v < GR; ++v) {
            const int g = g0 + v < G ? g0 + v : G - 1;
            const double* const row = tp + ((size_t)g * KT * GM + (unsigned)__builtin_amdgcn_readlane(fld, g));
            tv[v] = row[koff];
        }
#pragma unroll
        for (int v = 0; v < GR; ++v)
            if (g0 + v < G) sc = sc + tv[v];
    }
    double own = 0.0;
#pragma unroll 1
    for (int g = 0; g < gmp; ++g) own = own + pk_bcast(oe, g);  // (a loop, not kOwnPadMax tests: the path is rare and cold)
    if (k == zo) sc = own;
    double m = neg_inf();
#pragma unroll
    for (int j = 0; j < KT; ++j) m = max_score(m, pk_bcast(sc, j));
    const double w = expw_tab(sc - m, ET);
    double run = 0.0, cdf = 0.0;
#pragma unroll
    for (int j = 0; j < KT; ++j) {
        run = run + pk_bcast(w, j);
        cdf = lane == j ? run : cdf;
    }
    const double t = u * run;
    int zn = (int)__popcll(__ballot(lane < KT && t >= cdf));
    if (!(m > neg_inf())) zn = zoc;  // every category impossible: keep (or 0)
    return zn;
}

// One step of a walk over the lanes of a wave in DPP moves (two v_mov_b32 with a DPP control, no LDS crossbar and no
// s_waitcnt): x as the lanes CTRL names hold it, `old` where CTRL names no lane or ROWS leaves the row out.
// CTRL: 0x110 + n is row_shr:n (lane i - n of the same row of 16), 0x142 row_bcast:15 (lane 15 of the row below).
template <int CTRL, int ROWS>
__device__ __forceinline__ double pk_dpp(double old, double x) {
    const long long o = __double_as_longlong(old), b = __double_as_longlong(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)o, (int)(uint32_t)b, CTRL, ROWS, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(o >> 32), (int)(uint32_t)(b >> 32), CTRL, ROWS, 0xf, false);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// bits [g GW, g GW + GW) of a pattern whose words are uniform, g known at compile time: scalar shifts, no lane involved
template <int GW, int g>
__device__ __forceinline__ unsigned pk_field_at(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    constexpr int bit = g * GW, wd = bit >> 5, sh = bit & 31;
    static_assert(bit + GW <= kMaxP, "a group of the pattern");
    const uint32_t lo = wd == 0 ? w0 : (wd == 1 ? w1 : (wd == 2 ? w2 : w3));
    const uint32_t hi = wd == 0 ? w1 : (wd == 1 ? w2 : (wd == 2 ? w3 : 0u));
    const uint32_t f = sh + GW <= 32 ? lo >> sh : (lo >> sh) | (hi << ((32 - sh) & 31));
    return f & (unsigned)((1 << GW) - 1);
}

// The middle tier for one observation, by the whole wave, ahead of the definition: draw_mid (bmm_spec.h) on the
// binary32 entries the packed loop read for it, which are all in LDS.  As in pk_exact_count everything about the
// observation is wave-uniform and lane k takes category k: the G entries of its column (a whole first round at
// compile-time groups, the field a scalar extract; behind it the field of group g from lane g by v_readlane), up to
// MR reads issued before the first is used, each widened and added in binary64 (four partial
// sums: any order is within draw_mid's band).  The lane of the observation's own label reads its column of Tm32 where
// the others read theirs of Tq -- the two images have the same stride from group to group, so that is another base
// and the field taken once, not twice -- and nothing is added across lanes.  The maximum and the running sum are
// log-step walks in DPP moves over the 32 lanes that can hold a category (four steps inside a row of 16, one from row
// to row), the total and the maximum come from lane 31 by v_readlane, expw_tab reads E in LDS, the count and the
// verdict are ballots.  No global load, and two waits for LDS in all.  `certain` is uniform; where it comes back false
// the caller runs pk_exact_count as before.
// A first form walked the lanes with ds_bpermute_b32 (17 round trips through the LDS pipeline, which the scoring waves
// keep busy) and added the own entries across lanes: 6 200 ticks per observation where the definition takes 8 900;
// a second took every field by v_readlane and ran at priority 0: 3 300 (profiles/r12/README.md).
template <int KT, int GW>
__device__ __forceinline__ int pk_mid_count(const TableLayout& L, int G, const char* smem, uint32_t w0, uint32_t w1,
                                            uint32_t w2, uint32_t w3, int zo, double u, const lds_f64* ET, int lane,
                                            bool& certain) {
    constexpr int GM = 1 << GW;
    // reads in flight, one VGPR each: as many as pk_exact_count has loads in flight at two VGPRs each, so that this
    // block, not that one, never decides a form's registers (C5's twenty groups are one round)
    constexpr int MR = KT <= 4 ? 6 : KT <= 8 ? 10 : 20;
    static_assert(KT <= 32, "the walks cover two rows of 16 lanes");
    static_assert((kMaxP + GW - 1) / GW <= 64, "lane g holds the field of group g");
    const lds_f32* const img = (const lds_f32*)smem;  // Tq as single entries (pair j of a row at 2 j and 2 j + 1), Tm32 behind it
    const int k = lane < KT ? lane : KT - 1;
    const bool is_own = lane == zo;  // (zo < KT; -1: no lane)
    // entry of group g at field f: Tq[g * KT * GM + (k / 2) * 2 GM + 2 f + (k & 1)], Tm32[g * KT * GM + zo * GM + f]
    const unsigned base = is_own ? 2u * (unsigned)pk_tq_doubles(L) + (unsigned)k * GM : (unsigned)(k >> 1) * (2 * GM) + (unsigned)(k & 1);
    const unsigned fsh = is_own ? 0u : 1u;
    double part[4] = {0.0, 0.0, 0.0, 0.0};
    int g_from = 0;
    if (G >= MR) {
        // a whole first round (C5's twenty groups): groups known at compile time, so a field is a scalar extract of the
        // uniform words and a row an instruction offset -- one VALU instruction and the read per group
        static_assert(MR * GW <= kMaxP, "the first round's groups exist");
        float tv[MR];
        pk_static_for<0, MR>([&](auto J) {
            constexpr int g = decltype(J)::value;
            tv[g] = img[(unsigned)g * (KT * GM) + (base + (pk_field_at<GW, g>(w0, w1, w2, w3) << fsh))];
        });
        pk_static_for<0, MR>([&](auto J) {
            constexpr int g = decltype(J)::value;
            part[g & 3] = part[g & 3] + (double)tv[g];
        });
        g_from = MR;
    }
    // the groups behind it, and every group of a shape with fewer than MR: lane g extracts the field of group g with
    // selects and the groups read theirs from it by v_readlane, as pk_exact_count does
    int fld = 0;
    if (g_from < G) {
        const int gl = lane < G ? lane : G - 1;
        fld = (int)pk_field(gl * GW, GM - 1, w0, w1, w2, w3);
    }
#pragma unroll 1
    for (int g0 = g_from; g0 < G; g0 += MR) {
        float tv[MR];
#pragma unroll
        for (int v = 0; v < MR; ++v) {
            const int g = g0 + v < G ? g0 + v : G - 1;
            tv[v] = img[(unsigned)g * (KT * GM) + base + ((unsigned)__builtin_amdgcn_readlane(fld, g) << fsh)];
        }
#pragma unroll
        for (int v = 0; v < MR; ++v)
            if (g0 + v < G) part[v & 3] = part[v & 3] + (double)tv[v];
    }
    double sc = (part[0] + part[1]) + (part[2] + part[3]);
    if (lane >= KT) sc = neg_inf();
    const bool nan = __ballot(sc != sc) != 0;
    // the maximum of lanes 0 .. 31 in lane 31: row_shr 1, 2, 4, 8 leave a row's maximum in its lane 15, row_bcast:15
    // brings row 0's to row 1 (a lane without a source keeps its own value)
    double m = sc;
    m = __builtin_fmax(m, pk_dpp<0x111, 0xf>(m, m));
    m = __builtin_fmax(m, pk_dpp<0x112, 0xf>(m, m));
    m = __builtin_fmax(m, pk_dpp<0x114, 0xf>(m, m));
    m = __builtin_fmax(m, pk_dpp<0x118, 0xf>(m, m));
    m = __builtin_fmax(m, pk_dpp<0x142, 0xa>(m, m));
    m = pk_bcast(m, 31);
    // the running sum in label order, the same walk with 0 where there is no source (lanes from KT on weigh 0)
    double cdf = lane < KT ? expw_tab(sc - m, ET) : 0.0;
    cdf = cdf + pk_dpp<0x111, 0xf>(0.0, cdf);
    cdf = cdf + pk_dpp<0x112, 0xf>(0.0, cdf);
    cdf = cdf + pk_dpp<0x114, 0xf>(0.0, cdf);
    cdf = cdf + pk_dpp<0x118, 0xf>(0.0, cdf);
    cdf = cdf + pk_dpp<0x142, 0xa>(0.0, cdf);
    const double tot = pk_bcast(cdf, 31);
    const double t = u * tot;
    const double band = mid_band(m, kMidEpsUnit) * tot;
    const int cnt = (int)__popcll(__ballot(lane < KT && t >= cdf));
    const bool close = __ballot(lane < KT && !(__builtin_fabs(t - cdf) > band)) != 0;  // a NaN is close
    certain = !close && !nan && m > neg_inf() && m < pos_inf();
    return cnt;
}

// The kernel's arguments as the blocks outside the loop's steady state read them: from the kernel argument segment,
// through a pointer the compiler cannot see behind, where they run.  Everything those blocks need -- the definition's
// table pointers and layout, the histogram's place and shape for the movers, the DP's books, the flush -- would
// otherwise be computed ahead of the tile loop and held in scalar registers across it: more than the register file
// has, so the loop's steady state moved them to and from VGPR lanes on every trip (profiles/r09/README.md).  Scalar
// loads from the segment cost those rare blocks a round trip to the scalar cache and the loop nothing.
struct PkArgsView {
    const ChainParams* p;
    const ResampleArgs* a;
};
static_assert(alignof(ChainParams) == 8 && alignof(ResampleArgs) == 8 && sizeof(ChainParams) % 8 == 0,
              "k_resample_pk(ChainParams, ResampleArgs): the second argument lies right behind the first");
__device__ __forceinline__ PkArgsView pk_args_view() {
    const __attribute__((address_space(4))) char* ka =
        (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));  // not the pointer the kernel's own argument loads come from, as far as the compiler knows
    PkArgsView v;
    v.p = (const ChainParams*)ka;
    v.a = (const ResampleArgs*)(ka + sizeof(ChainParams));
    return v;
}
// the LDS places behind the two binary32 images, from the layout (k_resample_pk's comment)
struct PkLds {
    const int32_t* NkT;
    const lds_f64* ET;
    int32_t* hist;
};
__device__ __forceinline__ PkLds pk_lds(char* smem, const TableLayout& L) {
    double* const tail = reinterpret_cast<double*>(smem) + 2 * pk_tq_doubles(L);
    PkLds r;
    r.NkT = reinterpret_cast<const int32_t*>(tail);
    r.ET = (const lds_f64*)(tail + (L.et() - L.nk()));
    r.hist = reinterpret_cast<int32_t*>(tail + (L.tm() - L.nk()));
    return r;
}

// Where a lane sits in a chunk of 64 consecutive observations of a launch of n < 2^31: the chunk's first observation
// as an offset from the launch's first (uniform), and the lane's own offset from there, clamped to the last
// observation of the launch (lanes past the end re-read it and never write back).  The launch's base pointers have the
// batch's first observation folded in (launch_resample), so an observation's words and labels are at
// base + s0 (scalar) + voff (a zero-extended 32-bit lane offset): no 64-bit lane arithmetic.
struct PkPos {
    uint32_t s0;    // uniform
    uint32_t loff;  // lane offset in observations, clamped
    bool valid;
};
__device__ __forceinline__ PkPos pk_pos(uint32_t n, int chunk, int lane) {
    PkPos t;
    t.s0 = (uint32_t)chunk << 6;
    const uint32_t room = n - 1u - t.s0;
    t.valid = (uint32_t)lane <= room;
    t.loff = (uint32_t)lane < room ? (uint32_t)lane : room;
    return t;
}
template <class T>
__device__ __forceinline__ T* pk_at(T* sbase, uint32_t loff) {
    static_assert(sizeof(T) == 4, "words and labels");
    return (T*)((const char*)sbase + (loff * 4u));  // uniform base + zero-extended 32-bit lane offset (saddr form)
}
// load_words at a PkPos; W is tested where it is used (a flag computed ahead of the loop is a lane mask held across it)
__device__ __forceinline__ void pk_load_words(const uint32_t* Xb, int64_t N, int W, const PkPos& t, uint32_t& w0,
                                              uint32_t& w1, uint32_t& w2, uint32_t& w3) {
    const uint32_t* const b = Xb + t.s0;
    w0 = *pk_at(b, t.loff);
    if (W > 1) w1 = *pk_at(b + N, t.loff);
    if (W > 2) w2 = *pk_at(b + 2 * N, t.loff);
    if (W > 3) w3 = *pk_at(b + 3 * N, t.loff);
}

// draw_pk (bmm_spec.h) on scores held in pairs: s - m, the scaling by log2(e) and t - c[k] as packed binary32
// operations, each component rounded as the scalar instruction rounds it (same mode register), the running sum in the
// same order: cnt and the verdict are draw_pk's bit for bit (tests/test_gpu_pk_lean.py runs the two side by side).
// bmm_spec.h's function remains the statement of the draw.
template <int KT>
__device__ __forceinline__ bool pk_draw2(const pk_f2 (&s2)[KT / 2], float m, double u, int G, float unit, int& cnt) {
    static_assert(KT % 2 == 0 && KT <= kTier1MaxCats, "the band is derived for at most kTier1MaxCats categories");
    constexpr int KP = KT / 2;
    const pk_f2 mm{m, m}, l2e{0x1.715476p+0f, 0x1.715476p+0f};
    pk_f2 c[KP];
    float run = 0.0f;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const pk_f2 x = (s2[j] - mm) * l2e;  // sub, then mul: no fma (-ffp-contract=off, and the band's derivation)
        run = run + __builtin_amdgcn_exp2f(x.x);
        c[j].x = run;
        run = run + __builtin_amdgcn_exp2f(x.y);
        c[j].y = run;
    }
    const float t = (float)u * run;
    const pk_f2 tt{t, t};
    float nearest = __builtin_inff();
    int n = 0;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const pk_f2 diff = tt - c[j];
        n += diff.x >= 0.0f ? 1 : 0;
        nearest = __builtin_fminf(nearest, __builtin_fabsf(diff.x));
        n += diff.y >= 0.0f ? 1 : 0;
        nearest = __builtin_fminf(nearest, __builtin_fabsf(diff.y));
    }
    cnt = n;
    return nearest > pk_band(m, G, unit) * run && m > -__builtin_inff() && m < __builtin_inff();
}
// z_uniform (bmm_spec.h) of the observation whose global index is i0 + loff, i0 = obs0 + the launch's first.  While
// obs0 + hi <= 2^32 the high word z_key folds in is zero for every lane of the launch (key_uniform, a scalar): key
// and the ten round keys are scalars then, computed by the scalar unit.  The same bits by construction.  (gfx950 has
// no three-operand xor: a round's hi ^ k ^ c1 stays two instructions in either form.)
__device__ __forceinline__ double pk_uniform(uint64_t seed, uint64_t i0, uint32_t s0, uint32_t loff, uint32_t sweep,
                                             bool key_uniform) {
    uint32_t ra, rb;
    if (key_uniform) {
        uint32_t k = z_key(seed, 0);
        asm volatile("" : "+s"(k));  // a scalar, and this form is not folded into the general one below
        philox2x32_10((uint32_t)i0 + s0 + loff, sweep, k, ra, rb);
        asm volatile("" : "+v"(ra), "+v"(rb));
    } else {
        const uint64_t i = i0 + s0 + loff;
        philox2x32_10((uint32_t)i, sweep, z_key(seed, i), ra, rb);
    }
    return u52(ra, rb);
}

// ---- the second body's pieces (k_resample_pk<.., PIPE = true>): one group step at a compile-time group, and the
// scoring of a chunk written over it (pk_score)
template <int I>
struct PkIdx { static constexpr int value = I; };
template <int I, int N, class F>
__device__ __forceinline__ void pk_static_for(F&& f) {
    if constexpr (I < N) {
        f(PkIdx<I>{});
        pk_static_for<I + 1, N>(f);
    }
}
// The lookups of group g, g known at compile time: the field is one v_bfe_u32 (or one v_alignbit_b32 and a mask
// where it crosses a word), the group's rows are instruction offsets.  `fill` runs behind the first reads and ahead
// of the adds that need them: work that does not depend on the reads, placed in the shadow of their round trip.
template <int KT, int GW, int g, class Fill>
__device__ __forceinline__ void pk_step(const volatile lds_pk_f2* Tq, const volatile lds_f32* orow0, uint32_t b0,
                                        uint32_t b1, uint32_t b2, uint32_t b3, pk_f2 (&acc)[KT / 2], float& own32,
                                        Fill&& fill) {
    constexpr int GM = 1 << GW, KP = KT / 2, CH = KP <= 12 ? KP : KP / 2;
    constexpr int bit = g * GW, wd = bit >> 5, sh = bit & 31;
    static_assert(bit < kMaxP, "a group of the pattern");
    const uint32_t lo = wd == 0 ? b0 : (wd == 1 ? b1 : (wd == 2 ? b2 : b3));
    const uint32_t hi = wd == 0 ? b1 : (wd == 1 ? b2 : (wd == 2 ? b3 : 0u));
    const unsigned nib = (sh + GW <= 32 ? lo >> sh : __builtin_amdgcn_alignbit(hi, lo, (unsigned)sh)) & (unsigned)(GM - 1);
    const volatile lds_pk_f2* row = Tq + ((size_t)g * KP * GM + nib);
    const volatile lds_f32* orow = orow0 + ((size_t)g * KT * GM + nib);
#pragma unroll
    for (int c0 = 0; c0 < KP; c0 += CH) {
        pk_f2 tv[CH];
        float ov = 0.0f;
#pragma unroll
        for (int j = 0; j < CH; ++j) tv[j] = row[(c0 + j) * GM];
        if (c0 == 0) ov = *orow;
        if (c0 == 0) fill();
#pragma unroll
        for (int j = 0; j < CH; ++j) acc[c0 + j] = acc[c0 + j] + tv[j];
        if (c0 == 0) own32 = own32 + ov;
        if (CH < KP) __builtin_amdgcn_sched_barrier(0);
    }
}

// Behind an unrolled step: its sums exist here (the optimiser otherwise sinks the adds of several steps below the reads
// of the steps behind them and holds every read value until then), and the next step's reads stay behind them.  One
// statement for all the sums of a step (an inline asm takes up to 30 operands: 14 in-out pairs), so that the adds ahead
// of it are placed freely among themselves and the step's slice.
#define BMM_PK_PIN2(a, i) "+v"(a[i]), "+v"(a[(i) + 1])
template <int KT>
__device__ __forceinline__ void pk_step_end(pk_f2 (&acc)[KT / 2]) {
    constexpr int KP = KT / 2;
    static_assert(KP % 2 == 0 && KP <= 16, "pairs of sums");
    if constexpr (KP == 2) asm volatile("" : BMM_PK_PIN2(acc, 0));
    if constexpr (KP == 4) asm volatile("" : BMM_PK_PIN2(acc, 0), BMM_PK_PIN2(acc, 2));
    if constexpr (KP == 6) asm volatile("" : BMM_PK_PIN2(acc, 0), BMM_PK_PIN2(acc, 2), BMM_PK_PIN2(acc, 4));
    if constexpr (KP >= 8) asm volatile("" : BMM_PK_PIN2(acc, 0), BMM_PK_PIN2(acc, 2), BMM_PK_PIN2(acc, 4), BMM_PK_PIN2(acc, 6));
    if constexpr (KP == 10) asm volatile("" : BMM_PK_PIN2(acc, 8));
    if constexpr (KP == 12) asm volatile("" : BMM_PK_PIN2(acc, 8), BMM_PK_PIN2(acc, 10));
    if constexpr (KP == 14) asm volatile("" : BMM_PK_PIN2(acc, 8), BMM_PK_PIN2(acc, 10), BMM_PK_PIN2(acc, 12));
    if constexpr (KP == 16) asm volatile("" : BMM_PK_PIN2(acc, 8), BMM_PK_PIN2(acc, 10), BMM_PK_PIN2(acc, 12), BMM_PK_PIN2(acc, 14));
    __builtin_amdgcn_sched_barrier(0);
}
#undef BMM_PK_PIN2
// Groups [g_from, g_to) of a chunk in the rolled form of the present body: the word loop, the field by a runtime shift.
// A second copy of the group loop in k_resample_pk's present body (the `for (int h = 0; h < W; ++h)` under "scoring"),
// which stays inline there because calling this one cost that body four more spilled scalars at C5's form: a change to
// either belongs in both.
template <int KT, int GW>
__device__ __forceinline__ void pk_groups(const volatile lds_pk_f2* Tq, const volatile lds_f32* orow0, int g_from, int g_to,
                                          int W, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, pk_f2 (&acc)[KT / 2],
                                          float& own32) {
    constexpr int GM = 1 << GW, KP = KT / 2, CH = KP <= 12 ? KP : KP / 2;
#pragma unroll 1
    for (int h = (g_from * GW) >> 5; h < W; ++h) {
        const uint32_t cur = word_of(h, b0, b1, b2, b3), nxt = word_of(h + 1, b0, b1, b2, b3);
        int g_lo = (32 * h + GW - 1) / GW;
        g_lo = g_lo > g_from ? g_lo : g_from;
        int g_hi = (32 * (h + 1) + GW - 1) / GW;
        g_hi = g_hi < g_to ? g_hi : g_to;
#pragma unroll 1
        for (int g = g_lo; g < g_hi; ++g) {
            const unsigned nib = __builtin_amdgcn_alignbit(nxt, cur, (unsigned)(g * GW - 32 * h)) & (unsigned)(GM - 1);
            const volatile lds_pk_f2* row = Tq + ((size_t)g * KP * GM + nib);
            const volatile lds_f32* orow = orow0 + ((size_t)g * KT * GM + nib);
#pragma unroll
            for (int c0 = 0; c0 < KP; c0 += CH) {
                pk_f2 tv[CH];
                float ov = 0.0f;
#pragma unroll
                for (int j = 0; j < CH; ++j) tv[j] = row[(c0 + j) * GM];
                if (c0 == 0) ov = *orow;
#pragma unroll
                for (int j = 0; j < CH; ++j) acc[c0 + j] = acc[c0 + j] + tv[j];
                if (c0 == 0) own32 = own32 + ov;
                if (CH < KP) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}
// The scoring of one chunk in the second body, from cleared sums.  Group 0 is a step of its own, whatever G, with
// `head` in the shadow of its reads.  The groups behind it are taken in rounds of KT/2: a round that is whole (G >= KT/2, G >= KT)
// is straight-line code, its groups known at compile time; a round that is not whole runs the rolled loop, and so do
// the groups from the third round on.  (A guard per step was tried first: the compiler either held a mask per step in
// scalar registers across the tile loop or, with early exits, gave the accumulators new registers at every step and
// spilled them -- profiles/r10/README.md.)  G is tested on an opaque copy, where it is used.
template <int KT, int GW, class Head>
__device__ __forceinline__ void pk_score(const volatile lds_pk_f2* Tq, const volatile lds_f32* orow0, int G, int W,
                                         uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, pk_f2 (&acc)[KT / 2],
                                         float& own32, Head&& head) {
    constexpr int KP = KT / 2;
    constexpr bool kRound0 = (KP - 1) * GW < kMaxP, kRound1 = (2 * KP - 1) * GW < kMaxP;  // such a G exists
    asm volatile("" : "+s"(G));
#pragma unroll
    for (int j = 0; j < KP; ++j) acc[j] = pk_f2{0.0f, 0.0f};
    own32 = 0.0f;
    pk_step<KT, GW, 0>(Tq, orow0, b0, b1, b2, b3, acc, own32, head);
    pk_step_end<KT>(acc);
    bool whole = false;
    if constexpr (kRound0) whole = G >= KP;
    if (whole) {
        if constexpr (kRound0)
            pk_static_for<1, KP>([&](auto J) {
                pk_step<KT, GW, decltype(J)::value>(Tq, orow0, b0, b1, b2, b3, acc, own32, [] {});
                pk_step_end<KT>(acc);
            });
    } else if (G > 1) {
        pk_groups<KT, GW>(Tq, orow0, 1, G, W, b0, b1, b2, b3, acc, own32);  // (G < KT/2 here)
    }
    whole = false;
    if constexpr (kRound1) whole = G >= 2 * KP;
    if (whole) {
        if constexpr (kRound1)
            pk_static_for<0, KP>([&](auto J) {
                pk_step<KT, GW, KP + decltype(J)::value>(Tq, orow0, b0, b1, b2, b3, acc, own32, [] {});
                pk_step_end<KT>(acc);
            });
        if (G > 2 * KP) pk_groups<KT, GW>(Tq, orow0, 2 * KP, G, W, b0, b1, b2, b3, acc, own32);
    } else if (G > KP) {
        pk_groups<KT, GW>(Tq, orow0, KP, G, W, b0, b1, b2, b3, acc, own32);
    }
}

// Which forms run the second body: the 1024-thread forms of up to 20 accumulators, as round 10 chose them for its
// pipelined body (the predicate and its name are kept: KernelForm::pipe and bmm_dbg_kernel_pk_pipelined mean "this
// chain runs the second body").  They compile without scratch at 57, 65, 84, 86 and 98 VGPRs at 4, 8, 12, 16 and 20
// accumulators, within one VGPR of the present body up to 16.  The plain trip would also fit the forms of up to 28
// accumulators at every workgroup size (109 VGPRs at most, no scratch; 32 accumulators spill at 1024 threads); giving
// it to them is a change of its own, with its own timings.  Both bodies of every form: profiles/r11/README.md.
constexpr bool pk_pipelined(int kt, int nt, int /*gw*/) { return nt == 1024 && kt <= 20; }

// What a wave counts about its uncertain lanes: the test variant's counters (bmm_dbg_pk_counts, bmm_dbg_pk_unselected,
// bmm_dbg_pk_tier_counts) and the stamped build's ticks inside the two settle tiers.  In the product nothing writes or
// reads any of it.
struct PkTally {
    unsigned deferred = 0, unselected = 0;                // valid lanes handed to pk_settle's rare block; of them not selected
    unsigned mid_tried = 0, mid_settled = 0, exact = 0;   // runs of pk_mid_count, of them certain; runs of pk_exact_count
    DIAG(unsigned long long t_mid = 0, t_exact = 0;)      // ticks inside the runs of either
    DIAG(unsigned n_mid = 0, n_exact = 0;)
};

// What follows the packed draw of a chunk, the same in both bodies: the lanes the packed tier cannot prove, the DP's
// books, the movers.  pos, zo, u and the words b0..b3 are those of the chunk that was drawn.  Returns the label to store.
template <int KT, int GW>
__device__ __forceinline__ int pk_settle(const ResampleArgs& a, char* smem, const PkPos& pos, int lane, bool certain,
                                         int cnt, double u, int zo, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3,
                                         int dp_K, int K, PkTally& tally) {
    constexpr int GM = 1 << GW;
    const int zoc = zo < 0 ? 0 : zo;
    DBG_TIER1_FORCE(a, certain);
    bool defer = pos.valid && !certain;
#ifdef BMM_DEBUG_HOOKS
    const bool selected = a.pk_defer_every > 0 && pos.valid &&
                          (a.lo + (int64_t)pos.s0 + lane) % a.pk_defer_every == 0;
    tally.unselected += (unsigned)__popcll(__ballot(defer && !selected));
    defer = defer || selected;
#endif
    int zn = cnt;
    // ---- the lanes the packed tier cannot prove (uniform, rare), one lane at a time: the middle tier on the LDS
    // image first (pk_mid_count), the definition where that is not certain either, the count into that lane.  (A
    // certain lane of either tier has a finite maximum: the "every category impossible" case is always settled by the
    // definition.)  Arguments, layout and the lane number are taken here, not ahead of the loop.
    unsigned long long o = __ballot(defer);
#ifdef BMM_DEBUG_HOOKS
    tally.deferred += (unsigned)__popcll(o);
#endif
    if (__builtin_expect(o != 0, 0)) {
        const PkArgsView v = pk_args_view();
        const TableLayout Lc{v.p->G, KT, v.p->Gm, GM};
        const PkLds lc = pk_lds(smem, Lc);
        int ln = lane;
        asm volatile("" : "+v"(ln));
        // above the scoring waves' priority while it settles: this wave is the one its workgroup's barrier waits for
        __builtin_amdgcn_s_setprio(3);
        do {
            const int src = __ffsll((long long)o) - 1;
            o &= o - 1;
            const uint32_t w0 = __builtin_amdgcn_readlane(b0, src), w1 = __builtin_amdgcn_readlane(b1, src);
            const uint32_t w2 = __builtin_amdgcn_readlane(b2, src), w3 = __builtin_amdgcn_readlane(b3, src);
            const int zs = __builtin_amdgcn_readlane(zo, src);
            const double us = pk_bcast(u, src);
            bool settled = false;
            int e = 0;
            bool try_mid = true;
#ifdef BMM_DEBUG_HOOKS
            if (v.a->dbg_inject & 32) try_mid = false;  // BMM_DEBUG_PK_NOMID
#endif
            if (try_mid) {
                DIAG(const unsigned long long d_m0 = diag_stamp();)
                e = pk_mid_count<KT, GW>(Lc, v.p->G, smem, w0, w1, w2, w3, zs, us, lc.ET, ln, settled);
                DIAG(tally.t_mid += diag_stamp() - d_m0; ++tally.n_mid;)
#ifdef BMM_DEBUG_HOOKS
                // BMM_DEBUG_PK_MID_FAIL_EVERY: the middle tier's verdict dropped for every n-th observation
                if (v.a->pk_mid_fail_every > 0 && (v.a->lo + (int64_t)pos.s0 + src) % v.a->pk_mid_fail_every == 0) settled = false;
                ++tally.mid_tried;
                tally.mid_settled += settled ? 1u : 0u;
#endif
            }
            if (!settled) {
                DIAG(const unsigned long long d_e0 = diag_stamp();)
                e = pk_exact_count<KT, GW>(*v.p, *v.a, Lc, w0, w1, w2, w3, zs, us, lc.ET, ln);
                DIAG(tally.t_exact += diag_stamp() - d_e0; ++tally.n_exact;)
#ifdef BMM_DEBUG_HOOKS
                ++tally.exact;
#endif
            }
            if (ln == src) zn = e;
        } while (o);
        __builtin_amdgcn_s_setprio(0);
    }
    if (__builtin_expect(__ballot(zn == dp_K) != 0, 0)) {  // the DP's new cluster was drawn (rare): its books, from the staged sizes
        const PkArgsView v = pk_args_view();
        const int Kc = v.p->K;
        const TableLayout Lc{v.p->G, KT, v.p->Gm, GM};
        const int32_t* const Nkc = pk_lds(smem, Lc).NkT;
        int Kused = 0, new_label = -1;
        for (int k = 0; k < Kc; ++k) {
            if (Nkc[k] > 0) ++Kused;
            else if (new_label < 0) new_label = k;
        }
        if (zn == Kc) zn = pk_dp_label(Nkc, Kc, Kused, new_label, zo, zoc);
    }
    const bool keep = pos.valid;
#ifdef BMM_DEBUG_HOOKS
    BMM_DBG_LABELS(a, keep, pos.s0 + (uint32_t)lane == 0u, K, zn, zo);
#endif
    const bool moves = keep && zn >= 0 && zn != zo;
    if (__builtin_expect(__ballot(moves) != 0, 0)) {
        const PkArgsView v = pk_args_view();
        const int Kc = v.p->K, Pc = v.p->P;
        const TableLayout Lc{v.p->G, KT, v.p->Gm, GM};
        int ln = lane;
        asm volatile("" : "+v"(ln));
        count_movers(moves, zo, zn, b0, b1, b2, b3, pk_lds(smem, Lc).hist, Kc, Pc, ln);
    }
    return zn;
}

template <int KT, int NT, int GW, bool PIPE>
__global__ __launch_bounds__(NT) void k_resample_pk(ChainParams p, ResampleArgs a) {
    static_assert(KT % 2 == 0 && KT <= 32, "pairs of categories, one lane per category in pk_exact_count");
    constexpr int GM = 1 << GW;
    constexpr int KP = KT / 2;                      // pairs = accumulators (two binary32 each)
    constexpr int CH = KP <= 12 ? KP : KP / 2;      // lookups issued together
    static_assert(KP % CH == 0, "chunking");
    constexpr int NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const TableLayout L{p.G, KT, p.Gm, GM};
    double* const lds = reinterpret_cast<double*>(smem);
    const int nq_d = pk_tq_doubles(L), tail_d = L.tm() - L.nk();  // Tq, and Tm32 of as many bytes; Nk and E
    const volatile lds_pk_f2* const Tq = (const volatile lds_pk_f2*)lds;
    const volatile lds_f32* const Tm32 = (const volatile lds_f32*)(lds + nq_d);
    double* const tail = lds + 2 * nq_d;
    int32_t* const hist = reinterpret_cast<int32_t*>(tail + tail_d);  // [K*P] then [K]
    const int P = p.P, G = p.G, K = p.K;
    const int tid = threadIdx.x, lane = tid & 63;
    int* const next_chunk = hist + K * P + K;  // LDS counter behind the histogram
    DIAG(const unsigned long long d_entry = diag_stamp();)
    // work per wave in chunks of 64 observations, as in k_resample; plan_kernel offers this kernel for launches of
    // fewer than 2^31 observations only, and launch_resample has folded the launch's first observation into Xb, z_in
    // and z_out: an observation is a 32-bit offset from there
    const uint32_t n = (uint32_t)(a.hi - a.lo);
    const int nchunks = (int)((n + 63u) >> 6);
    const int cpw = (nchunks + (int)gridDim.x - 1) / (int)gridDim.x;
    const int wg_c0 = (int)blockIdx.x * cpw;
    const int wg_cn = nchunks - wg_c0 < cpw ? nchunks - wg_c0 : cpw;  // chunks of this workgroup (may be <= 0)
    const int W = (P + 31) / 32;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool has_tile = wave < wg_cn;
    PkPos pos = pk_pos(n, has_tile ? wg_c0 + wave : 0, lane);
    uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    if (has_tile) pk_load_words(a.Xb, p.N, W, pos, b0, b1, b2, b3);  // before the tables are staged
    {
        // stage the two binary32 images and Nk, E of the table image: eight 16-byte loads in flight per lane
        auto stage = [&](const double* from, double* to, int n2) {
            const double2* src = reinterpret_cast<const double2*>(from);
            double2* dst = reinterpret_cast<double2*>(to);
            for (int i0 = tid; i0 < n2; i0 += NT * 8) {
                double2 t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = i0 + u * NT;
                    t[u] = src[i < n2 ? i : n2 - 1];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = i0 + u * NT;
                    if (i < n2) dst[i] = t[u];
                }
            }
        };
        stage(a.tab + L.doubles(), lds, nq_d);
        stage(a.tab + L.nk(), tail, tail_d / 2);
    }
    for (int i = tid; i < K * P + K; i += NT) hist[i] = 0;
    if (tid == 0) *next_chunk = NW;
    __syncthreads();
    DIAG(const unsigned long long d_staged = diag_stamp();)
    DIAG(unsigned long long d_score = 0, d_trips = 0;)  // ticks of this wave's trips between the first and the last lookup, trips

    float unit = kPkEpsUnit;
#ifdef BMM_DEBUG_HOOKS
    if (a.dbg_inject & 8) unit = 0.0f;
#endif
    // valid lanes this wave has settled by the definition: counted and reported by the test variant only
    // (bmm_dbg_pk_counts); in the product nothing writes or reads them, nor the K that pk_settle hands to its label check
    PkTally tally;

    // What the loop's steady state -- a chunk without an uncertain lane and without a mover -- holds in scalar
    // registers is named here: three base pointers, the plane stride, the launch's length and this workgroup's chunks,
    // G, W, K, the draw's key and counter base, the two LDS places.  The blocks beside it (the definition for an
    // uncertain lane, the DP's books, the movers, the flush) take their arguments from the kernel argument segment
    // where they run (pk_args_view), and a uniform flag is tested on the value it comes from, behind an opaque copy,
    // so that no lane mask of it is carried around the loop.
    if (has_tile) {
        const uint32_t* const Xb = a.Xb;
        const int32_t* const z_in = a.z_in;
        int32_t* const z_out = a.z_out;
        const int64_t N = p.N;
        const uint64_t seed = p.seed, i0 = (uint64_t)(p.obs0 + a.lo);
        const uint32_t sweep = a.sweep;
        // every observation of the launch below 2^32: the key of z_uniform is one scalar (pk_uniform)
        int key_general = (int)(uint32_t)(((uint64_t)(p.obs0 + a.hi) - 1u) >> 32);  // != 0: some index is >= 2^32
#ifdef BMM_DEBUG_HOOKS
        if (a.dbg_inject & 16) key_general = 1;  // BMM_DEBUG_PK_GENKEY: the general form whatever the launch
#endif
        key_general = __builtin_amdgcn_readfirstlane(key_general);
        const int dp_K = p.mode == MODE_DP ? K : -1;  // the count that stands for the DP's new cluster, or none
        const int has_zin = (int)((uint32_t)((uintptr_t)z_in >> 32) | (uint32_t)(uintptr_t)z_in);  // != 0: there are labels
        int zo = -1;
        if (z_in) zo = *pk_at(z_in + pos.s0, pos.loff);
        asm volatile("" : "+v"(zo));  // landed before the pipeline starts (k_resample)
        if constexpr (!PIPE) {
        int zn_prev = 0;
        uint32_t st_s0 = 0, st_loff = 0;  // the chunk whose labels are still to be stored
        bool st_on = false;               //   ... and the lanes of it that store
        for (;;) {
            const int zoc = zo < 0 ? 0 : zo;
            if (st_on) *pk_at(z_out + st_s0, st_loff) = zn_prev;
            int nc = 0;
            if (lane == 0) nc = atomicAdd(next_chunk, 1);
            nc = __builtin_amdgcn_readfirstlane(nc);
            const bool has_next = nc < wg_cn;  // uniform
            const PkPos npos = pk_pos(n, has_next ? wg_c0 + nc : 0, lane);
            uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
            int zo_next = -1;
            int Wl = W, zl = has_zin;
            asm volatile("" : "+s"(Wl), "+s"(zl));  // (tested below, on the values)

            // ---- scoring: (K / 2) * G conflict-free 64-bit LDS lookups, one packed add each; per group one 32-bit
            // gather of the own cluster's "observation removed" entry at the same field, one add.  (pk_groups is a
            // second copy of this loop, for the second body's rolled groups: a change to either belongs in both.)
            pk_f2 acc[KP];
#pragma unroll
            for (int j = 0; j < KP; ++j) acc[j] = pk_f2{0.0f, 0.0f};
            float own32 = 0.0f;
            const volatile lds_f32* const orow0 = Tm32 + zoc * GM;
            DIAG(const unsigned long long d_s0 = diag_stamp();)
            __builtin_amdgcn_s_setprio(BMM_LOOKUP_PRIO);
#pragma unroll 1
            for (int h = 0; h < W; ++h) {
                if (has_next && h == 0) {
                    pk_load_words(Xb, N, Wl, npos, n0, n1, n2, n3);
                    if (zl) zo_next = *pk_at(z_in + npos.s0, npos.loff);
                }
                const uint32_t cur = word_of(h, b0, b1, b2, b3), nxt = word_of(h + 1, b0, b1, b2, b3);
                const int g_lo = (32 * h + GW - 1) / GW;
                int g_hi = (32 * (h + 1) + GW - 1) / GW;
                g_hi = g_hi < G ? g_hi : G;
#pragma unroll 1
                for (int g = g_lo; g < g_hi; ++g) {
                    const unsigned nib = __builtin_amdgcn_alignbit(nxt, cur, (unsigned)(g * GW - 32 * h)) & (unsigned)(GM - 1);
                    const volatile lds_pk_f2* row = Tq + ((size_t)g * KP * GM + nib);
                    const volatile lds_f32* orow = orow0 + ((size_t)g * KT * GM + nib);
#pragma unroll
                    for (int c0 = 0; c0 < KP; c0 += CH) {
                        pk_f2 tv[CH];
                        float ov = 0.0f;
#pragma unroll
                        for (int j = 0; j < CH; ++j) tv[j] = row[(c0 + j) * GM];
                        if (c0 == 0) ov = *orow;  // with the first chunk of Tq reads
#pragma unroll
                        for (int j = 0; j < CH; ++j) acc[c0 + j] = acc[c0 + j] + tv[j];
                        if (c0 == 0) own32 = own32 + ov;
                        if (CH < KP) __builtin_amdgcn_sched_barrier(0);  // keep the chunks apart
                    }
                }
            }
            __builtin_amdgcn_s_setprio(0);
            DIAG(d_score += diag_stamp() - d_s0; ++d_trips;)
            // the binary32 scores, the observation's own cluster from its own image
            pk_f2 s2[KP];
            float m = -__builtin_inff();
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                float x = acc[j].x, y = acc[j].y;
                if (2 * j == zo) x = own32;
                if (2 * j + 1 == zo) y = own32;
                s2[j] = pk_f2{x, y};
                m = __builtin_fmaxf(m, x);
                m = __builtin_fmaxf(m, y);
            }
            int kg = key_general;
            asm volatile("" : "+s"(kg));
            const double u = pk_uniform(seed, i0, pos.s0, pos.loff, sweep, kg == 0);
            int cnt = 0;
            const bool certain = pk_draw2<KT>(s2, m, u, G, unit, cnt);
            const int zn = pk_settle<KT, GW>(a, smem, pos, lane, certain, cnt, u, zo, b0, b1, b2, b3, dp_K, K, tally);
            const bool keep = pos.valid;
            zn_prev = zn;
            st_s0 = pos.s0; st_loff = pos.loff; st_on = keep;
            if (!has_next) break;
            b0 = n0; b1 = n1; b2 = n2; b3 = n3;
            zo = zo_next;
            pos = npos;
        }
        if (st_on) *pk_at(z_out + st_s0, st_loff) = zn_prev;
        } else {
        // ---- the second body: the present body's trip, in its order, with the lookups in unrolled steps at
        // compile-time groups (pk_score).  The chunk counter's atomic stays at the head of the trip (the compiler turns
        // it into a wave reduction whose result it waits for and broadcasts on the spot), and what follows from its
        // index -- the next chunk's place and loads -- and the Philox rounds of this chunk's uniform are issued in the
        // shadow of group 0's reads.  Nothing of a chunk is carried into the next trip but the labels to store.
        int zn_prev = 0;
        uint32_t st_s0 = 0, st_loff = 0;  // the chunk whose labels are still to be stored
        bool st_on = false;               //   ... and the lanes of it that store
        for (;;) {
            const int zoc = zo < 0 ? 0 : zo;
            if (st_on) *pk_at(z_out + st_s0, st_loff) = zn_prev;
            int nc = 0;
            if (lane == 0) nc = atomicAdd(next_chunk, 1);
            bool has_next = false;  // uniform
            PkPos npos;  // (places are copied member by member: a whole-struct copy of a PkPos set in a lambda goes through memory)
            npos.s0 = pos.s0; npos.loff = pos.loff; npos.valid = pos.valid;
            uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
            int zo_next = -1;
            double u = 0.0;
            int Wl = W, zl = has_zin, kg = key_general;
            asm volatile("" : "+s"(Wl), "+s"(zl), "+s"(kg));  // (tested below, on the values)
            pk_f2 acc[KP];
            float own32;
            const volatile lds_f32* const orow0 = Tm32 + zoc * GM;
            DIAG(const unsigned long long d_s0 = diag_stamp();)
            __builtin_amdgcn_s_setprio(BMM_LOOKUP_PRIO);
            pk_score<KT, GW>(Tq, orow0, G, W, b0, b1, b2, b3, acc, own32, [&] {
                __builtin_amdgcn_sched_barrier(0);  // group 0's reads are issued ahead of this, not behind it
                nc = __builtin_amdgcn_readfirstlane(nc);
                has_next = nc < wg_cn;
                const PkPos t = pk_pos(n, has_next ? wg_c0 + nc : 0, lane);
                npos.s0 = t.s0; npos.loff = t.loff; npos.valid = t.valid;
                if (has_next) {
                    pk_load_words(Xb, N, Wl, npos, n0, n1, n2, n3);
                    if (zl) zo_next = *pk_at(z_in + npos.s0, npos.loff);
                }
                u = pk_uniform(seed, i0, pos.s0, pos.loff, sweep, kg == 0);
            });
            __builtin_amdgcn_s_setprio(0);
            DIAG(d_score += diag_stamp() - d_s0; ++d_trips;)
            // the binary32 scores, the observation's own cluster from its own image
            pk_f2 s2[KP];
            float m = -__builtin_inff();
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                float x = acc[j].x, y = acc[j].y;
                if (2 * j == zo) x = own32;
                if (2 * j + 1 == zo) y = own32;
                s2[j] = pk_f2{x, y};
                m = __builtin_fmaxf(m, x);
                m = __builtin_fmaxf(m, y);
            }
            int cnt = 0;
            const bool certain = pk_draw2<KT>(s2, m, u, G, unit, cnt);
            const int zn = pk_settle<KT, GW>(a, smem, pos, lane, certain, cnt, u, zo, b0, b1, b2, b3, dp_K, K, tally);
            zn_prev = zn;
            st_s0 = pos.s0; st_loff = pos.loff; st_on = pos.valid;
            if (!has_next) break;
            b0 = n0; b1 = n1; b2 = n2; b3 = n3;
            zo = zo_next;
            pos.s0 = npos.s0; pos.loff = npos.loff; pos.valid = npos.valid;
        }
        if (st_on) *pk_at(z_out + st_s0, st_loff) = zn_prev;
        }
    }

    DIAG(const unsigned long long d_loop = diag_stamp();)
    __syncthreads();
    DIAG(const unsigned long long d_sync = diag_stamp();)
    {
        const PkArgsView v = pk_args_view();
        const int Kc = v.p->K, Pc = v.p->P;
        const TableLayout Lc{v.p->G, KT, v.p->Gm, GM};
        const int rep = blockIdx.x % kDeltaReps;
        flush_hist(pk_lds(smem, Lc).hist, Kc, Pc, v.a->dS + (size_t)rep * Kc * Pc, v.a->dNk + rep * Kc, tid, NT);
    }
    // diagnostic build: per-launch phases in the slots k_resample reports them in; workgroup-launches and entry to
    // flushed in [7] and [14], which k_resample leaves alone, the per-trip split in [16] and [17]; from wave 0 of the workgroup only (every wave's atomics
    // on one line, as k_resample has them, take longer than this launch and hold up the global loads of workgroups
    // still at work)
    DIAG(asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); const unsigned long long d_flush = diag_stamp();)
    DIAG(if (a.diag && tid == 0) {
        atomicAdd(&a.diag[5], 1ull); atomicAdd(&a.diag[7], 1ull); atomicAdd(&a.diag[14], d_flush - d_entry);
        atomicAdd(&a.diag[8], d_staged - d_entry); atomicAdd(&a.diag[9], d_loop - d_staged);
        atomicAdd(&a.diag[10], d_sync - d_loop); atomicAdd(&a.diag[11], d_flush - d_sync);
        atomicAdd(&a.diag[16], d_score); atomicAdd(&a.diag[17], d_trips);  // wave 0's trips: the lookups, and how many
        // wave 0's settled lanes: ticks inside the middle tier and inside the definition, and the runs of either
        if (tally.n_mid) { atomicAdd(&a.diag[18], tally.t_mid); atomicAdd(&a.diag[19], (unsigned long long)tally.n_mid); }
        if (tally.n_exact) { atomicAdd(&a.diag[20], tally.t_exact); atomicAdd(&a.diag[21], (unsigned long long)tally.n_exact); }
    })
#ifdef BMM_DEBUG_HOOKS
    if (a.pk_stat) {  // test variant: draws made and valid lanes settled by the definition (bmm_dbg_pk_counts)
        if (tid == 0) {
            int64_t first = a.lo + (int64_t)wg_c0 * 64, last = a.lo + ((int64_t)wg_c0 + (wg_cn > 0 ? wg_cn : 0)) * 64;
            last = last < a.hi ? last : a.hi;
            if (last > first) atomicAdd(&a.pk_stat[0], (unsigned long long)(last - first));
        }
        if (lane == 0 && tally.deferred) atomicAdd(&a.pk_stat[1], (unsigned long long)tally.deferred);
        if (lane == 0 && tally.unselected) atomicAdd(&a.pk_stat[2], (unsigned long long)tally.unselected);
        // the settle tiers (bmm_dbg_pk_tier_counts): runs of the middle tier, of them certain, runs of the definition
        if (lane == 0 && tally.mid_tried) atomicAdd(&a.pk_stat[3], (unsigned long long)tally.mid_tried);
        if (lane == 0 && tally.mid_settled) atomicAdd(&a.pk_stat[4], (unsigned long long)tally.mid_settled);
        if (lane == 0 && tally.exact) atomicAdd(&a.pk_stat[5], (unsigned long long)tally.exact);
    }
#endif
}

// ---------------------------------------------------------------------------------
// Generic path: any P, up to kMaxCatsAny categories, no LDS residency.  Same arithmetic as
// k_resample (group lookups in g order, expw_, running sum and count in label order), with the
// tables gathered from global memory (L2) and the scores kept in a per-thread scratch column
// scr[k * stride + thread].  Clusters are accumulated sixteen at a time, X is re-read per chunk.
// Slow next to the resident kernel; it exists so that every shape the reference accepts runs.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ unsigned field_from_x(const int32_t* X, const uint32_t* Xb, int64_t N, int P,
                                                  int64_t i, int g, int GW) {
    if (Xb) {  // bit planes, any number of words: the field may straddle two of them
        const int o = g * GW, w = o >> 5, sh = o & 31, W = (P + 31) >> 5;
        uint32_t v = Xb[(int64_t)w * N + i] >> sh;
        if (sh + GW > 32 && w + 1 < W) v |= Xb[(int64_t)(w + 1) * N + i] << (32 - sh);
        return v & (unsigned)((1 << GW) - 1);
    }
    unsigned nib = 0;
    for (int j = 0; j < GW; ++j) {
        const int d = g * GW + j;
        if (d < P) nib |= ((unsigned)X[i + (int64_t)d * N] & 1u) << j;
    }
    return nib;
}

__global__ __launch_bounds__(256) void k_resample_generic(ChainParams p, ResampleArgs a, double* scr,
                                                          int64_t stride) {
    const bool has_minus = !explicit_params(p.mode);
    const TableLayout L = layout_of(p, has_minus);
    const int GM = L.M;
    const double* const Tp = a.tab + L.tp();
    const double* const Tm = a.tab + L.tm();
    const int32_t* const NkT = reinterpret_cast<const int32_t*>(a.tab + L.nk());
    const double* const ET = a.tab + L.et();
    const int P = p.P, G = p.G, K = p.K, Kc = p.Kc, KT = p.KT;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double* const my = scr + gid;

    int Kused = 0, new_label = -1;
    if (p.mode == MODE_DP) {
        for (int k = 0; k < K; ++k) {
            if (NkT[k] > 0) ++Kused;
            else if (new_label < 0) new_label = k;
        }
    }
    for (int64_t i = a.lo + gid; i < a.hi; i += (int64_t)gridDim.x * blockDim.x) {
        int zo = a.z_in ? a.z_in[i] : -1;
        const int zoc = zo < 0 ? 0 : zo;
        double acc_own = 0.0;
        if (has_minus)
            for (int g = 0; g < p.Gm; ++g)
                acc_own = acc_own + Tm[((size_t)g * KT + zoc) * kGroupMm + field_from_x(a.X, a.Xb, p.N, P, i, g, kGroupWm)];
        double m = neg_inf();
        for (int k0 = 0; k0 < Kc; k0 += 16) {
            double acc[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = 0.0;
            for (int g = 0; g < G; ++g) {
                const double* row = Tp + ((size_t)g * KT + k0) * GM + field_from_x(a.X, a.Xb, p.N, P, i, g, p.W);
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (k0 + j < Kc) acc[j] = acc[j] + row[j * GM];
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k = k0 + j;
                if (k < Kc) {
                    double sc = acc[j];
                    if (has_minus && k == zo) sc = acc_own;
                    my[(int64_t)k * stride] = sc;
                    m = __builtin_fmax(m, sc);
                }
            }
        }
        double run = 0.0;
        for (int k = 0; k < Kc; ++k) {
            const double w = expw_tab(my[(int64_t)k * stride] - m, ET);
            if (a.wts) a.wts[(int64_t)k * p.N + i] = w;
            run = run + w;
            my[(int64_t)k * stride] = run;
        }
        const double tot = run;
        if (a.wts) a.wtot[i] = tot;
        const double t = z_uniform(p.seed, (uint64_t)(p.obs0 + i), a.sweep) * tot;
        int zn = 0;
        for (int k = 0; k < Kc; ++k) zn += t >= my[(int64_t)k * stride] ? 1 : 0;
        if (!(m > neg_inf())) zn = zoc;
        if (p.mode == MODE_DP && zn == K) {
            const int own_single = (zo >= 0 && NkT[zoc] == 1) ? 1 : 0;
            if (Kused - own_single < K - 1) {
                zn = new_label;
                if (own_single && (zn < 0 || zo < zn)) zn = zo;
            } else {
                int best = -1, bs = 0;
                for (int k = 0; k < K; ++k) {
                    const int sz = NkT[k] - (k == zo ? 1 : 0);
                    if (sz > 0 && (best < 0 || sz < bs)) { best = k; bs = sz; }
                }
                zn = best >= 0 ? best : zoc;
            }
        }
        BMM_DBG_LABELS(a, true, i == a.lo, K, zn, zo);
        a.z_out[i] = zn;
        if (zn >= 0 && zn != zo) {
            int32_t* const rNk = a.dNk + (blockIdx.x % kDeltaReps) * K;
            int32_t* const rS = a.dS + (size_t)(blockIdx.x % kDeltaReps) * K * P;
            atomicAdd(&rNk[zn], 1);
            if (zo >= 0) atomicAdd(&rNk[zo], -1);
            for (int d = 0; d < P; ++d)
                if (a.Xb ? (a.Xb[(int64_t)(d >> 5) * p.N + i] >> (d & 31)) & 1u : (uint32_t)a.X[i + (int64_t)d * p.N] & 1u) {
                    atomicAdd(&rS[(size_t)zn * P + d], 1);
                    if (zo >= 0) atomicAdd(&rS[(size_t)zo * P + d], -1);
                }
        }
    }
}

__global__ __launch_bounds__(256) void k_count_labels_generic(ChainParams p, const int32_t* __restrict__ X,
                                                              const uint32_t* __restrict__ Xb,
                                                              const int32_t* __restrict__ z, int32_t* dNk,
                                                              int32_t* dS) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.N; i += (int64_t)gridDim.x * blockDim.x) {
        const int zl = z[i];
        if (zl < 0) continue;
        atomicAdd(&dNk[zl], 1);
        for (int d = 0; d < p.P; ++d)
            if (Xb ? (Xb[(int64_t)(d >> 5) * p.N + i] >> (d & 31)) & 1u : (uint32_t)X[i + (int64_t)d * p.N] & 1u)
                atomicAdd(&dS[(size_t)zl * p.P + d], 1);
    }
}

// ---- constrained allocations: known labels and allowed-label sets (include/bmm_mcmc.h "constraints"; DESIGN.md
// section 25) ----
// Behind a resample launch over [lo, hi): every listed row of that range whose drawn label lies outside its set goes
// back to the label it had (z_in; the lowest allowed label where it had none), and the move the resample launch has
// just flushed for it is undone in the same delta set: -1 at the drawn label, +1 at the restored one, for Nk and for
// every set feature of the row.  The next consumer of the deltas (a table build, k_sb_params, k_count_sweep_end) sums
// them, so the row never appears moved.  One lane per listed row; integer LDS and global atomics and plain stores only:
// the result does not depend on any order.
// project: the other use, outside a sweep -- a listed row whose label lies outside its set takes its
// (label mod |set|)-th allowed label (the rule of the starting labels); dNk = null where nothing has counted the labels
// yet, stats = null.
struct ConstrainArgs {
    const int64_t* rows;    // the listed rows of the range, ascending
    const uint64_t* masks;  // bit k of masks[q]: rows[q] may take label k
    int64_t n;
    const int32_t* z_in;    // null: the rows had no labels (the first sweep of a DP or explicit chain)
    int32_t* z_out;
    const int32_t* X;       // the chain's matrix: int32 (the generic twin) ...
    const uint32_t* Xb;     // ... or bit planes
    int32_t *dNk, *dS;      // the pending delta set, kDeltaReps replicas of each
    unsigned long long* stats;  // [0] listed rows drawn, [1] reverted
    int project;
};
__device__ __forceinline__ int constrain_nth_allowed(uint64_t mask, int n) {
    for (int t = 0; t < n; ++t) mask &= mask - 1;
    return __ffsll((long long)mask) - 1;
}
// the label a listed row is to hold given the one it holds now (zd); `moves`: whether that is another one
__device__ __forceinline__ int constrain_target(const ConstrainArgs& a, int64_t i, uint64_t mask, int zd, bool& moves) {
    const bool inside = zd >= 0 && zd < 64 && ((mask >> zd) & 1ull);
    moves = !inside && !(a.project && zd < 0);
    if (!moves) return zd;
    if (a.project) return constrain_nth_allowed(mask, zd % __popcll(mask));
    const int zp = a.z_in ? a.z_in[i] : -1;
    return zp >= 0 ? zp : __ffsll((long long)mask) - 1;
}
__device__ __forceinline__ void constrain_stats(const ConstrainArgs& a, unsigned long long reverted, int tid) {
    if (!a.stats) return;
    if ((tid & 63) == 0 && reverted) atomicAdd(&a.stats[1], reverted);
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&a.stats[0], (unsigned long long)a.n);
}
__global__ __launch_bounds__(256) void k_constrain(ChainParams p, ConstrainArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int32_t* const hist = reinterpret_cast<int32_t*>(smem);
    const int P = p.P, K = p.K, tid = threadIdx.x, lane = tid & 63;
    if (a.dNk) {
        for (int i = tid; i < K * P + K; i += 256) hist[i] = 0;
        __syncthreads();
    }
    unsigned long long reverted = 0;  // of this wave (uniform)
    const int64_t ntiles = (a.n + 255) / 256;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t q = tile * 256 + tid;
        const bool valid = q < a.n;
        const int64_t qc = valid ? q : a.n - 1;
        const int64_t i = a.rows[qc];
        const uint64_t mask = a.masks[qc];
        const int zd = a.z_out[i];
        bool moves;
        const int zr = constrain_target(a, i, mask, zd, moves);
        moves = moves && valid;
        uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
        if (moves) {
            a.z_out[i] = zr;
            if (a.dNk) load_words(a.Xb, p.N, (P + 31) / 32, i, b0, b1, b2, b3);
        }
        if (a.dNk) count_movers(moves, zd, zr, b0, b1, b2, b3, hist, K, P, lane);  // (uniform)
        reverted += (unsigned long long)__popcll(__ballot(moves));
    }
    if (a.dNk) {
        __syncthreads();
        flush_hist(hist, K, P, a.dS + (size_t)(blockIdx.x % kDeltaReps) * K * P, a.dNk + (blockIdx.x % kDeltaReps) * K, tid, 256);
    }
    constrain_stats(a, reverted, tid);
}
// ... for a chain on the generic path or the int32 layout: the adds go straight to the replica, as k_resample_generic's do
__global__ __launch_bounds__(256) void k_constrain_generic(ChainParams p, ConstrainArgs a) {
    const int P = p.P, K = p.K, tid = threadIdx.x;
    unsigned long long reverted = 0;
    const int64_t ntiles = (a.n + 255) / 256;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t q = tile * 256 + tid;
        const bool valid = q < a.n;
        const int64_t qc = valid ? q : a.n - 1;
        const int64_t i = a.rows[qc];
        const uint64_t mask = a.masks[qc];
        const int zd = a.z_out[i];
        bool moves;
        const int zr = constrain_target(a, i, mask, zd, moves);
        moves = moves && valid;
        if (moves) {
            a.z_out[i] = zr;
            if (a.dNk) {
                int32_t* const rNk = a.dNk + (blockIdx.x % kDeltaReps) * K;
                int32_t* const rS = a.dS + (size_t)(blockIdx.x % kDeltaReps) * K * P;
                atomicAdd(&rNk[zr], 1);
                if (zd >= 0) atomicAdd(&rNk[zd], -1);
                for (int d = 0; d < P; ++d)
                    if (a.Xb ? (a.Xb[(int64_t)(d >> 5) * p.N + i] >> (d & 31)) & 1u : (uint32_t)a.X[i + (int64_t)d * p.N] & 1u) {
                        atomicAdd(&rS[(size_t)zr * P + d], 1);
                        if (zd >= 0) atomicAdd(&rS[(size_t)zd * P + d], -1);
                    }
            }
        }
        reverted += (unsigned long long)__popcll(__ballot(moves));
    }
    constrain_stats(a, reverted, tid);
}

// The allocation probabilities of one batch, normalised and filed by label: the matrix the reference
// stores for Stephens' relabelling (collapsed_gibbs.cpp:162-172, collapsed_gibbs_dp.cpp:190-200,
// stickbreaking.cpp:129-139).  wts/wtot are what the resample kernel of this batch emitted;
// probs is N x K column-major.  The DP's new-cluster mass goes under the label a new cluster would take
// for THIS observation (choices(K) = unused_clusters.top(), collapsed_gibbs_dp.cpp:169-170,193): the
// smallest free label of the batch (from the table image's cluster sizes) -- or the observation's own
// label when it sat alone in its cluster and that label is smaller, because removing it (:113-128) has
// just returned that label to the heap.  The draw itself (k_resample) opens the same label.
__global__ __launch_bounds__(256) void k_probs_finish(ChainParams p, const double* __restrict__ tab,
                                                      const double* __restrict__ wts,
                                                      const double* __restrict__ wtot,
                                                      const int32_t* __restrict__ z_in, int64_t lo, int64_t hi,
                                                      double* __restrict__ probs) {
    const TableLayout L = layout_of(p, !explicit_params(p.mode));
    const int32_t* const NkT = reinterpret_cast<const int32_t*>(tab + L.nk());
    int new_label = -1;
    if (p.mode == MODE_DP)
        for (int k = 0; k < p.K && new_label < 0; ++k)
            if (NkT[k] <= 0) new_label = k;
    for (int64_t i = lo + (int64_t)blockIdx.x * 256 + threadIdx.x; i < hi; i += (int64_t)gridDim.x * 256) {
        const double tot = wtot[i];
        int own_new = new_label;
        if (p.mode == MODE_DP && z_in) {
            const int zo = z_in[i];
            if (zo >= 0 && NkT[zo] == 1 && (new_label < 0 || zo < new_label)) own_new = zo;
        }
        for (int k = 0; k < p.Kc; ++k) {
            const int lbl = k < p.K ? k : own_new;  // in label order: the new-cluster mass lands last
            if (lbl >= 0) probs[i + (int64_t)lbl * p.N] = div_(wts[(int64_t)k * p.N + i], tot);
        }
    }
}

// The label trace on its way out: observations [i0, i0 + rows) of the [S][N] 0-based device trace as the
// rows x S block of R's S x N column-major matrix they occupy (out[(i - i0) * S + s]: that block is
// contiguous in the caller's buffer), labels 1-based.  T = int32_t: unassigned -> NA_integer_;
// T = uint8_t (at most 254 labels): unassigned -> 0, widened on the host, a quarter of the bytes over PCIe.
// perm (relabel = TRUE, Stephens on the device): label v of kept sweep s leaves as perm(s, v) + 1, perm the
// S x K column-major permutation table (collapsed_gibbs.cpp:197-199); nullptr: as sampled.
template <typename T>
__global__ __launch_bounds__(256) void k_trace_block(const int32_t* __restrict__ trace, int64_t N, int S,
                                                     int64_t i0, int64_t rows, T* __restrict__ out,
                                                     const int32_t* __restrict__ perm = nullptr) {
    __shared__ int32_t tile[32][33];
    const int64_t b0 = (int64_t)blockIdx.x * 32;  // within the block of observations
    const int s0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int s = s0 + r;
        const int64_t li = b0 + tx;
        tile[r][tx] = (s < S && li < rows) ? trace[(size_t)s * N + i0 + li] : 0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t li = b0 + r;
        const int s = s0 + tx;
        if (s < S && li < rows) {
            int32_t v = tile[tx][r];
            if (perm && v >= 0) v = perm[s + (int64_t)v * S];
            if (sizeof(T) == 1) out[(size_t)li * S + s] = (T)(v < 0 ? 0 : v + 1);
            else out[(size_t)li * S + s] = (T)(v < 0 ? (int32_t)0x80000000 : v + 1);
        }
    }
}

// initialK as R hands it over (1-based) -> the chain's 0-based label row; bad[0] receives the smallest
// index whose label lies outside 1..K (or stays at its initial all-ones value)
__global__ __launch_bounds__(256) void k_labels_from_r(const int32_t* __restrict__ z1, int64_t N, int K,
                                                       int32_t* __restrict__ z0, unsigned long long* bad) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const int32_t v = z1[i];
        if (v < 1 || v > K) atomicMin(bad, (unsigned long long)i);
        z0[i] = v - 1;
    }
}

// ---- Stephens' relabelling (src/stephens.cpp as it executes) -------------------
// Matrices are N x K column-major (p[n + k*N]); a cost matrix is K x K column-major (C[k + l*K]); a
// permutation table is rows x K column-major (perm(r, k) at perm[r + k*ld]), 0-based.
constexpr int kStephensMaxK = 128;  // = BMM_STEPHENS_MAX_K
// rows of p / log q staged in LDS per step of the cost kernel: 64 up to 32 categories (48 KiB), 16 above
__host__ __device__ inline int st_tile_rows(int K) { return (K + 3) / 4 * 4 <= 32 ? 64 : 16; }

// The shape of the cost pass for K categories -- the kernel, its launch and bmm_device_stephens_plan all read it
// here: nb 4 x 4 blocks of C; below 256 blocks, ng groups of nb threads share a tile's rows (256 - ng * nb threads
// idle); above, every thread owns B blocks (the template argument of k_st_cost_partial)
__host__ __device__ inline int st_cost_nb(int K) { return ((K + 3) / 4) * ((K + 3) / 4); }
__host__ __device__ inline int st_cost_ng(int K) { return st_cost_nb(K) >= 256 ? 1 : 256 / st_cost_nb(K); }
__host__ __device__ inline int st_cost_b(int K) { return st_cost_nb(K) <= 256 ? 1 : (st_cost_nb(K) + 255) / 256; }

// LDS bytes of k_st_cost_partial for K categories: three T x K4 tiles, or the cross-group reduction (ng x nb x 16)
__host__ __device__ inline size_t st_cost_lds(int K) {
    const int K4 = (K + 3) / 4 * 4, nb = st_cost_nb(K);
    const int ng = st_cost_ng(K);
    const size_t tiles = (size_t)3 * st_tile_rows(K) * K4 * sizeof(double);
    const size_t red = ng > 1 ? (size_t)ng * nb * 16 * sizeof(double) : 0;
    return tiles > red ? tiles : red;
}

// Per-workgroup partial cost matrices over rows [wg*rows, (wg+1)*rows) of slice blockIdx.y:
//   C[k,l] = sum_n p(n,l) * (a(n,l) - log q(n,k)),  a = log p (batch, stephens.cpp:50) or p (online, :79),
// a term with p(n,l) == 0 counting exactly 0 (an all-zero column costs 0 against every row).  q is read as
// log q (lq_is_log) or as q; rows are staged st_tile_rows(K) at a time.  Each thread owns 4 x 4 blocks of C (B of them when there are more than 256
// blocks); with fewer blocks, ng groups of threads take every ng-th row of a tile and are summed in group
// order at the end.  partial[(slice * G + wg) * K*K + k + l*K]; no atomics: a fixed shape sums in a fixed order.
template <int B>
__global__ __launch_bounds__(256) void k_st_cost_partial(const double* __restrict__ p, int64_t N, int K,
                                                         int64_t slice_stride, const double* __restrict__ q,
                                                         int lq_is_log, int batch_form, int64_t rows,
                                                         double* __restrict__ partial) {
    extern __shared__ double st_lds[];
    const int K4 = (K + 3) / 4 * 4, nbk = K4 / 4, nb = st_cost_nb(K);
    const int ng = st_cost_ng(K);
    const int tid = threadIdx.x;
    const int g = nb >= 256 ? 0 : tid / nb;
    const bool active = g < ng;
    const int T = st_tile_rows(K);
    double* sP = st_lds;
    double* sA = st_lds + T * K4;
    double* sL = st_lds + 2 * T * K4;
    const double* ps = p + (int64_t)blockIdx.y * slice_stride;
    const int64_t n0 = (int64_t)blockIdx.x * rows;
    const int64_t n1 = n0 + rows < N ? n0 + rows : N;
    double acc[B][16];
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[b][e] = 0.0;
    for (int64_t r0 = n0; r0 < n1; r0 += T) {
        for (int idx = tid; idx < T * K4; idx += 256) {
            const int t = idx % T, col = idx / T;
            const int64_t n = r0 + t;
            const bool ok = n < n1 && col < K;
            const double pv = ok ? ps[n + (int64_t)col * N] : 0.0;
            const double qv = ok ? q[n + (int64_t)col * N] : 1.0;
            sP[t * K4 + col] = pv;
            sA[t * K4 + col] = batch_form ? (pv > 0.0 ? log(pv) : 0.0) : pv;
            sL[t * K4 + col] = lq_is_log ? qv : log(qv);
        }
        __syncthreads();
        if (active) {
            for (int t = g; t < T; t += ng) {
#pragma unroll
                for (int b = 0; b < B; ++b) {
                    const int blk = nb >= 256 ? tid + 256 * b : tid % nb;
                    if (blk >= nb) continue;
                    const int kb = blk % nbk, lb = blk / nbk;
                    double lq[4], pp[4], aa[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        lq[u] = sL[t * K4 + 4 * kb + u];
                        pp[u] = sP[t * K4 + 4 * lb + u];
                        aa[u] = sA[t * K4 + 4 * lb + u];
                    }
#pragma unroll
                    for (int l = 0; l < 4; ++l)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const double term = pp[l] * (aa[l] - lq[k]);
                            acc[b][k + 4 * l] += pp[l] != 0.0 ? term : 0.0;
                        }
                }
            }
        }
        __syncthreads();
    }
    const int KK = K * K;
    double* out = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * KK;
    if (ng == 1) {
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int blk = tid + 256 * b;
            if (blk >= nb) continue;
            const int kb = blk % nbk, lb = blk / nbk;
#pragma unroll
            for (int l = 0; l < 4; ++l)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int kk = 4 * kb + k, ll = 4 * lb + l;
                    if (kk < K && ll < K) out[kk + ll * K] = acc[b][k + 4 * l];
                }
        }
        return;
    }
    // ng > 1: one block per thread (B == 1); sum the groups in order
    double* red = st_lds;  // [ng][nb][16]
    if (active)
#pragma unroll
        for (int e = 0; e < 16; ++e) red[((size_t)g * nb + (tid % nb)) * 16 + e] = acc[0][e];
    __syncthreads();
    for (int e = tid; e < KK; e += 256) {
        const int kk = e % K, ll = e / K;
        const int blk = kk / 4 + (ll / 4) * nbk, sub = (kk % 4) + 4 * (ll % 4);
        double s = 0.0;
        for (int gg = 0; gg < ng; ++gg) s += red[((size_t)gg * nb + blk) * 16 + sub];
        out[e] = s;
    }
}

// cost[slice][e] = sum over the G partials of that slice, in a fixed order (four quarters, then the quarters
// in order).  Grid (ceil(KK / 64), slices), 256 threads.
__global__ __launch_bounds__(256) void k_st_cost_reduce(const double* __restrict__ partial, int G, int KK,
                                                        double* __restrict__ cost) {
    __shared__ double part[4][64];
    const int lane = threadIdx.x & 63, quarter = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    const int per = (G + 3) / 4, g0 = quarter * per, g1 = g0 + per < G ? g0 + per : G;
    const double* base = partial + (int64_t)blockIdx.y * G * KK;
    double s = 0.0;
    if (e < KK)
        for (int g = g0; g < g1; ++g) s += base[(int64_t)g * KK + e];
    part[quarter][lane] = s;
    __syncthreads();
    if (quarter == 0 && e < KK)
        cost[(int64_t)blockIdx.y * KK + e] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// The assignment (lp_solve's integer program in my_lpsolve): min sum_k C[k, sigma(k)] over permutations, by the
// O(K^3) shortest-augmenting-path Hungarian method with potentials u (rows), v (columns), rows added in index
// order.  In each scan the free column with the smallest slack wins under strict <, i.e. the lowest index wins a
// tie; potentials are updated elementwise.  tests/stephens_ref.py restates exactly these steps.  One wave per
// cost matrix (blockIdx.x = slice), lane j handling columns j, j + 64, j + 128 (index 0 is the virtual column).
// perm(slice, l) = the row assigned to column l (stephens.cpp:54-55, 83-84; not inverted: :56, :85).
constexpr int kStAssignCols = 3;  // columns per lane: 1 + kStephensMaxK <= 64 * 3
inline int st_assign_cols(int K) { return (K + 1 + 63) / 64; }  // columns 0 .. K over 64 lanes: registers in use
// the cost matrix is staged in LDS when it fits beside u, v, minv, pr, way, used (K <= 88)
inline bool st_assign_in_lds(int K) {
    return (size_t)K * K * sizeof(double) + (size_t)(K + 1) * (3 * sizeof(double) + 3 * sizeof(int)) <= 65536;
}
inline size_t st_assign_lds(int K) {
    const size_t cm = (size_t)K * K * sizeof(double);
    const size_t rest = (size_t)(K + 1) * (3 * sizeof(double) + 3 * sizeof(int));
    return (st_assign_in_lds(K) ? cm : 0) + rest;
}
__global__ __launch_bounds__(64) void k_st_assign(const double* __restrict__ cost, int K, int32_t* __restrict__ perm,
                                                  int64_t ld, int cost_in_lds) {
    extern __shared__ double st_lds[];
    const int lane = threadIdx.x;
    const int KK = K * K;
    const double* Cg = cost + (int64_t)blockIdx.x * KK;
    double* sC = st_lds;
    double* u = st_lds + (cost_in_lds ? KK : 0);
    double* v = u + (K + 1);
    double* minv = v + (K + 1);
    int* pr = reinterpret_cast<int*>(minv + (K + 1));
    int* way = pr + (K + 1);
    int* used = way + (K + 1);
    if (cost_in_lds)
        for (int e = lane; e < KK; e += 64) sC[e] = Cg[e];
    const double* C = cost_in_lds ? sC : Cg;
    for (int j = lane; j <= K; j += 64) { u[j] = 0.0; v[j] = 0.0; pr[j] = 0; way[j] = 0; }
    __syncthreads();
    const double INF = __builtin_huge_val();
    for (int i = 1; i <= K; ++i) {
        for (int j = lane; j <= K; j += 64) { minv[j] = INF; used[j] = 0; }
        if (lane == 0) pr[0] = i;
        __syncthreads();
        int j0 = 0;
        for (;;) {
            if (lane == 0) used[j0] = 1;
            __syncthreads();
            const int i0 = pr[j0];
            const double ui0 = u[i0];
            double best = INF;
            int bj = 0x7fffffff;
#pragma unroll
            for (int r = 0; r < kStAssignCols; ++r) {
                const int j = lane + 64 * r;
                if (j < 1 || j > K || used[j]) continue;
                const double cur = (C[(i0 - 1) + (int64_t)(j - 1) * K] - ui0) - v[j];
                if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
                if (minv[j] < best) { best = minv[j]; bj = j; }
            }
            for (int off = 32; off >= 1; off >>= 1) {  // (value, index) minimum: the lowest index wins a tie
                const double ob = __shfl_xor(best, off);
                const int oj = __shfl_xor(bj, off);
                if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
            }
            const double delta = best;
            const int j1 = bj;
            __syncthreads();
            for (int j = lane; j <= K; j += 64) {
                if (used[j]) { u[pr[j]] += delta; v[j] -= delta; }
                else minv[j] -= delta;
            }
            __syncthreads();
            j0 = j1;
            if (j0 > K || pr[j0] == 0) break;  // j0 > K: no finite slack left (non-finite costs)
        }
        if (lane == 0 && j0 <= K) {
            do { const int j1 = way[j0]; pr[j0] = pr[j1]; j0 = j1; } while (j0);
        }
        __syncthreads();
    }
    for (int l = lane; l < K; l += 64) perm[blockIdx.x + (int64_t)l * ld] = pr[l + 1] - 1;
}

// p.replace(0, 1e-6) over the whole batch window (stephens.cpp:30-31)
__global__ __launch_bounds__(256) void k_st_replace_zeros(double* __restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        if (p[i] == 0.0) p[i] = 0.000001;
}

// Q of one batch iteration (stephens.cpp:36-43): q(n,k) = (sum over slices m, in order, of p_m(n, perm(m,k))) / M,
// and log q for that iteration's costs
__global__ __launch_bounds__(256) void k_st_q_batch(const double* __restrict__ p, int64_t N, int K, int M,
                                                    const int32_t* __restrict__ perm, double* __restrict__ Q,
                                                    double* __restrict__ LQ) {
    const int64_t NK = N * K;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < NK; i += (int64_t)gridDim.x * 256) {
        const int64_t n = i % N;
        const int k = (int)(i / N);
        double s = 0.0;
        for (int m = 0; m < M; ++m) {
            const int pk = min(max(perm[m + (int64_t)k * M], 0), K - 1);  // in range whatever the costs were
            s += p[(int64_t)m * NK + n + (int64_t)pk * N];
        }
        const double qv = s / (double)M;
        Q[i] = qv;
        LQ[i] = log(qv);
    }
}

// The online update (stephens.cpp:86-92): Q = (j * (Q + p[:, perm])) / (j + 1) -- add, multiply, correctly rounded
// divide, no contraction (the library is built with -ffp-contract=off)
__global__ __launch_bounds__(256) void k_st_q_online(double* __restrict__ Q, const double* __restrict__ p, int64_t N,
                                                     int K, const int32_t* __restrict__ perm, int64_t ld, double j,
                                                     double j1) {
    const int64_t NK = N * K;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < NK; i += (int64_t)gridDim.x * 256) {
        const int64_t n = i % N;
        const int k = (int)(i / N);
        const int pk = min(max(perm[(int64_t)k * ld], 0), K - 1);
        const double sum = Q[i] + p[n + (int64_t)pk * N];
        Q[i] = (j * sum) / j1;
    }
}

__global__ __launch_bounds__(256) void k_st_perm_identity(int32_t* __restrict__ perm, int M, int K) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < M * K) perm[i] = i / M;
}

// ---- posterior predictive density of new observations -------------------------
// The z-step for an (N+1)-th observation that is not in the data: no own-cluster pass, no uniform, no draw,
// no histogram -- the Kc category scores from the group tables, max-shift, expw, total, and then
//   logdens = max + log(total) = log p(x | state).
// New rows are always held as bit planes (k_pack_bits: word w of row m at Xb[w * M + m]).  A row is owned by one
// lane, so the accumulators that live in global memory across sweeps are updated without atomics and in a
// fixed order: the streaming log-sum-exp pair (run_max, run_sum) with
//   sum_s p(x | s) = exp(run_max) * run_sum,
// and, when asked for, the Kc running sums of the normalised category weights.
// Leave-one-out scores the fitted rows the same way, the row's own label from the minus-self
// tables; its arguments ride in the same struct.
struct ScoreArgs {
    const uint32_t* Xb;  // bit planes of the scored rows: the new rows, or the fitted rows (null on the int32 layout)
    int64_t rows;        // scored rows
    const double* tab;   // counting samplers: the image k_state_tables wrote; explicit samplers: the chain's own image
    double* out;         // or null: [rows], this state's log p(x | state) (predictive) or ell (leave-one-out)
    // predictive
    double* resp;        // or null: [Kc][rows], this state's normalised category weights
    double* run_max;     // or null (nothing is folded): [rows] running maximum of logdens over the folded states
    double* run_sum;     //   [rows] sum over the folded states of exp(logdens - run_max)
    double* resp_acc;    // or null: [Kc][rows] running sums of the normalised category weights
    // leave-one-out
    const int32_t* X;    // generic path on the int32 layout: the matrix as handed over (else null)
    const int32_t* z;    // a counting sampler: the state's labels, 0-based (else null)
    double* acc;         // or null (nothing is folded): [kLooAcc][rows]
    int n;               // states folded before this one
};

// The table image of the counting samplers for a stored state, from the statistics as they stand (the pending deltas
// are added, nothing is folded or cleared: this kernel changes no state of the chain).  One workgroup per category,
// laid out as k_count_tables lays the image out; terms and constants are the count-table rules' (bmm_spec.h):
//   MINUS = false  BUILD_PREDICT, the predictive image of a new row (N, not N - 1: the new row is not among the N
//                  fitted observations), the plain set only, 256 threads: roles 0, 1
//   MINUS = true   BUILD_LOO, the leave-one-out image of the fitted rows: the plain set over N - 1 rows and the
//                  minus-self set in groups of kGroupWm (n_k - 1 and S_kd - x_d; an entry whose bit pattern no member
//                  of the label can have is never read), 512 threads: roles 0 to 3
//   finite sampler  label k: log(n_k + alpha/K) - log(rows + alpha), an empty label included (its prior weight and the
//                   prior Bernoulli terms log(beta) - log(beta + gamma), log(gamma) - log(beta + gamma))
//   DP              used label: log(n_k) - log(rows + alpha); unused label: -inf; category K, the new cluster:
//                   log(alpha) - log(rows + alpha) with the prior Bernoulli terms as a per-feature table like any other
template <bool MINUS>
__global__ __launch_bounds__(MINUS ? 512 : 256) void k_state_tables(ChainParams p, const int32_t* __restrict__ Nk,
                                                                    const int32_t* __restrict__ S,
                                                                    const int32_t* __restrict__ dNk,
                                                                    const int32_t* __restrict__ dS,
                                                                    const double* __restrict__ alpha_ptr,
                                                                    double* __restrict__ tab) {
    __shared__ double e1[kMaxP], e0[kMaxP], m1[MINUS ? kMaxP : 1], m0[MINUS ? kMaxP : 1], cst[4];  // cst: Cp, Cm, the two denominators
    const int k = blockIdx.x;
    const TableLayout L = layout_of(p, MINUS);
    const int P = p.P, K = p.K;
    const bool is_label = k < K;
    const size_t KP = (size_t)K * P;
    const int64_t n = is_label ? (int64_t)Nk[k] + delta_take(const_cast<int32_t*>(dNk), k, K) : 0;
    const CountRule r{MINUS ? BUILD_LOO : BUILD_PREDICT, p.mode == MODE_DP, K, p.Ntot, p.beta, p.gamma, *alpha_ptr};
    const int role = threadIdx.x >> 7, dl = threadIdx.x & 127;
    if (threadIdx.x == 0) {
        const double ak = rule_ak(r);  // one division; unrolled, each j is a constant and only the logs needed are taken
        double v[kRuleLogs];
#pragma unroll
        for (int j = 0; j < kRuleLogs; ++j) {
            double arg;
            v[j] = const_arg(r, ak, k, n, j, arg) ? log_(arg) : 0.0;
        }
        const CatConsts c = cat_consts(r, k, n, v);
        cst[0] = c.cp; cst[1] = c.cm; cst[2] = c.den_p; cst[3] = c.den_m;
        tab[L.cp() + k] = c.cp;
        tab[L.cm() + k] = c.cm;
        reinterpret_cast<int32_t*>(tab + L.nk())[k] = (int32_t)n;
    }
    __syncthreads();
    for (int c0 = 0; c0 < P; c0 += kChunkP) {
        const int pc = P - c0 < kChunkP ? P - c0 : kChunkP;
        if (dl < pc) {  // (accumulators past Kc keep all-zero tables under a -inf constant)
            const int d = c0 + dl;
            const int64_t s = is_label ? (int64_t)S[(size_t)k * P + d] + delta_take(const_cast<int32_t*>(dS), (size_t)k * P + d, KP) : 0;
            double arg;
            const bool have = term_arg(r, k, role, n, s, arg);
            const double t = term_of(have, have ? log_(arg) : 0.0, cst[2 + term_den(role)]);
            if (MINUS) (role == 0 ? e1 : role == 1 ? e0 : role == 2 ? m1 : m0)[dl] = t;
            else (role == 0 ? e1 : e0)[dl] = t;
        }
        __syncthreads();
        write_group_tables(p.W, e1, e0, pc, c0, p.KT, k, cst[0], tab + L.tp());
        if (MINUS) write_group_tables(kGroupWm, m1, m0, pc, c0, p.KT, k, cst[1], tab + L.tm());
        __syncthreads();
    }
    if (k == 0 && threadIdx.x < 256) tab[L.et() + threadIdx.x] = exp256_table()[threadIdx.x];
}

// one new row's share of the accumulators; ld = log p(x | state), ET the exp256 table
template <class Tab>
__device__ __forceinline__ void predict_fold(const ScoreArgs& a, int64_t m, double ld, Tab ET) {
    const double rm = a.run_max[m], rs = a.run_sum[m];
    const bool up = ld > rm;
    const double e = expw_tab(up ? rm - ld : ld - rm, ET);  // (-inf and NaN arguments give exactly 0)
    a.run_max[m] = up ? ld : rm;
    a.run_sum[m] = up ? rs * e + 1.0 : rs + e;
}

// empty accumulators: no state folded
__global__ __launch_bounds__(256) void k_predict_reset(int64_t M, double* __restrict__ run_max, double* __restrict__ run_sum) {
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
        run_max[m] = neg_inf();
        run_sum[m] = 0.0;
    }
}

// The accumulators after n folded states: lppd = run_max + log(run_sum) - log(n), resp = resp_acc / n.  The
// accumulators themselves are left as they are, so more sweeps may be folded afterwards.
__global__ __launch_bounds__(256) void k_predict_finish(int64_t M, int Kc, int n, const double* __restrict__ run_max,
                                                        const double* __restrict__ run_sum,
                                                        const double* __restrict__ resp_acc,
                                                        double* __restrict__ lppd, double* __restrict__ resp) {
    const double ln = log_((double)n), dn = (double)n;
    for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
        lppd[m] = (run_max[m] + log_(run_sum[m])) - ln;
        if (resp)
            for (int k = 0; k < Kc; ++k) resp[(int64_t)k * M + m] = div_(resp_acc[(int64_t)k * M + m], dn);
    }
}

// ---- leave-one-out predictive of the fitted rows ------------------------------
// ell_i = log p(x_i | everything else in the state), include/bmm_mcmc.h.  For the counting samplers that is the
// z-step of row i with its own contribution removed, normalised as the predictive is: every label scored from the
// plain tables (constants over N - 1 fitted rows), the row's own label from the minus-self tables (n_k - 1, S_k - x_i),
// max-shift, expw, total, ell = max + log(total).  No uniform, no draw, no histogram, no statistics.  For the explicit
// samplers the labels do not enter and the chain's own image (log pi in group 0) is scored as a new row is.
// A fitted row is owned by one lane, so the seven accumulators a row keeps across sweeps are updated without atomics
// and in a fixed order.
constexpr int kLooAcc = 7;
enum : int { LOO_MAX = 0, LOO_SUM, LOO_MIN, LOO_S1, LOO_S2, LOO_MEAN, LOO_M2 };
//   LOO_MAX, LOO_SUM   streaming pair of logsumexp(ell): sum_s exp(ell_s) = exp(MAX) * SUM
//   LOO_MIN, S1, S2    one running minimum for both harmonic sums: sum_s exp(-ell_s) = exp(-MIN) * S1,
//                      sum_s exp(-2 ell_s) = exp(-2 MIN) * S2
//   LOO_MEAN, LOO_M2   Welford's mean and sum of squared deviations of ell
constexpr int kLooOut = 5;  // per-row outputs of k_loo_finish: log_cpo, ess, lppd, mean, var

// one fitted row's share of the accumulators; ell = this state's value, ET the exp256 table
template <class Tab>
__device__ __forceinline__ void loo_fold(const ScoreArgs& a, int64_t i, double ell, Tab ET) {
    double* const A = a.acc + i;
    const int64_t N = a.rows;
    {
        const double rm = A[LOO_MAX * N], rs = A[LOO_SUM * N];
        const bool up = ell > rm;
        const double e = expw_tab(up ? rm - ell : ell - rm, ET);  // (-inf gives exactly 0: the first fold)
        A[LOO_MAX * N] = up ? ell : rm;
        A[LOO_SUM * N] = up ? rs * e + 1.0 : rs + e;
    }
    {
        const double mn = A[LOO_MIN * N], s1 = A[LOO_S1 * N], s2 = A[LOO_S2 * N];
        const bool dn = ell < mn;
        const double e = expw_tab(dn ? ell - mn : mn - ell, ET);
        const double e2 = e * e;
        A[LOO_MIN * N] = dn ? ell : mn;
        A[LOO_S1 * N] = dn ? s1 * e + 1.0 : s1 + e;
        A[LOO_S2 * N] = dn ? s2 * e2 + 1.0 : s2 + e2;
    }
    {
        const double mean = A[LOO_MEAN * N], m2 = A[LOO_M2 * N];
        const double delta = ell - mean;
        const double mean1 = mean + div_(delta, (double)(a.n + 1));
        A[LOO_MEAN * N] = mean1;
        A[LOO_M2 * N] = m2 + delta * (ell - mean1);
    }
}

// The scorer of stored states.  One lane per scored row, KT accumulators, NT threads; the LDS image is the head of the
// table image and the exp256 table (no histogram, no chunk counter), read as k_resample reads it: one ds_read_b64
// per category and group, conflict-free.  The next tile's words (and label) are loaded before this tile is scored.
//   LOO = false  the predictive of new rows (MINUS = 0): logdens, responsibilities, predict_fold
//   LOO = true   the leave-one-out predictive of the fitted rows: ell, loo_fold.  MINUS: 0 the explicit samplers (no
//                labels, no own pass), 1 the minus-self tables in LDS behind the plain ones, 2 the minus-self tables
//                gathered from global memory (the shapes whose resample kernel does the same).  The own-label score is
//                gathered before the accumulators are live, as k_resample's own pass does.
constexpr int kScoreThreads = 512;
template <int KT, int NT, int GW, int MINUS, bool LOO>
__global__ __launch_bounds__(NT) void k_score(ChainParams p, ScoreArgs a) {
    static_assert(LOO || MINUS == 0, "a new row has no label of its own");
    constexpr int GM = 1 << GW;
    constexpr int CH = KT <= 24 ? KT : (KT <= 48 ? KT / 2 : KT / 4);  // lookups issued together
    static_assert(KT % CH == 0, "chunking");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const TableLayout L{p.G, KT, MINUS ? p.Gm : 0, GM};
    double* const lds = reinterpret_cast<double*>(smem);
    const volatile lds_f64* const Tp = (const volatile lds_f64*)(lds + L.tp());
    const volatile lds_f64* const TmL = (const volatile lds_f64*)(lds + L.tm());
    const double* const TmG = a.tab + L.tm();
    const lds_f64* const ET = (const lds_f64*)(lds + L.et());
    const int P = p.P, G = p.G, Gm = p.Gm, K = p.K, Kc = p.Kc;
    const int tid = threadIdx.x;
    const int W = (P + 31) / 32;
    const int64_t ntiles = (a.rows + NT - 1) / NT;
    int64_t tile = blockIdx.x;
    uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    int z = -1;
    if (tile < ntiles) {  // the first tile's words go out before the image is staged
        const int64_t i0 = tile * NT + tid;
        const int64_t ic = i0 < a.rows ? i0 : a.rows - 1;
        load_words(a.Xb, a.rows, W, ic, b0, b1, b2, b3);
        if (MINUS) z = a.z[ic];
    }
    {
        const double2* src = reinterpret_cast<const double2*>(a.tab);
        double2* dst = reinterpret_cast<double2*>(smem);
        const int n2 = (MINUS == 1 ? L.doubles() : L.head()) / 2;  // even: every piece of the layout is
        for (int i0 = tid; i0 < n2; i0 += NT * 8) {
            double2 t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * NT;
                t[u] = src[i < n2 ? i : n2 - 1];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * NT;
                if (i < n2) dst[i] = t[u];
            }
        }
    }
    __syncthreads();
    for (; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * NT + tid;
        const bool valid = i < a.rows;
        const int64_t tnext = tile + gridDim.x;
        uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
        int zn = -1;
        if (tnext < ntiles) {
            const int64_t in = tnext * NT + tid;
            const int64_t ic = in < a.rows ? in : a.rows - 1;
            load_words(a.Xb, a.rows, W, ic, n0, n1, n2, n3);
            if (MINUS) zn = a.z[ic];
        }
        const bool seated = !MINUS || (unsigned)z < (unsigned)K;
        double own = 0.0;
        if (MINUS) {  // the row's own label from the minus-self tables, before the accumulators are live
            const int zc = seated ? z : 0;
#pragma unroll 1
            for (int h = 0; h < W; ++h) {
                const uint32_t cur = word_of(h, b0, b1, b2, b3), nxt = word_of(h + 1, b0, b1, b2, b3);
                const int g_lo = (32 * h + kGroupWm - 1) / kGroupWm;
                int g_hi = (32 * (h + 1) + kGroupWm - 1) / kGroupWm;
                g_hi = g_hi < Gm ? g_hi : Gm;
#pragma unroll 1
                for (int g = g_lo; g < g_hi; ++g) {
                    const unsigned nib = __builtin_amdgcn_alignbit(nxt, cur, (unsigned)(g * kGroupWm - 32 * h)) & (unsigned)(kGroupMm - 1);
                    const size_t at = ((size_t)g * KT + zc) * kGroupMm + nib;
                    own = own + (MINUS == 1 ? TmL[at] : TmG[at]);
                }
            }
        }
        // The own label's accumulator starts at -inf and stays there whatever is added (the tables hold no +inf), so
        // its plain score counts exactly 0 below; the minus-self score is one more category, summed last.  (Replacing
        // acc[z] after the scoring instead costs a second set of live accumulators: 254 VGPRs at KT = 32 and scratch
        // from KT = 40 on, against 127 and none this way.)
        double acc[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) acc[k] = MINUS && k == z ? neg_inf() : 0.0;
#pragma unroll 1
        for (int h = 0; h < W; ++h) {
            const uint32_t cur = word_of(h, b0, b1, b2, b3), nxt = word_of(h + 1, b0, b1, b2, b3);
            const int g_lo = (32 * h + GW - 1) / GW;
            int g_hi = (32 * (h + 1) + GW - 1) / GW;
            g_hi = g_hi < G ? g_hi : G;
#pragma unroll 1
            for (int g = g_lo; g < g_hi; ++g) {
                const unsigned nib = __builtin_amdgcn_alignbit(nxt, cur, (unsigned)(g * GW - 32 * h)) & (unsigned)(GM - 1);
                const volatile lds_f64* row = Tp + ((size_t)g * KT * GM + nib);
#pragma unroll
                for (int c0 = 0; c0 < KT; c0 += CH) {
                    double tv[CH];
#pragma unroll
                    for (int j = 0; j < CH; ++j) tv[j] = row[(c0 + j) * GM];
#pragma unroll
                    for (int j = 0; j < CH; ++j) acc[c0 + j] = acc[c0 + j] + tv[j];
                    if (CH < KT) __builtin_amdgcn_sched_barrier(0);  // keep the chunks apart
                }
            }
        }
        const double ownv = MINUS && seated ? own : neg_inf();
        double mx = ownv;
#pragma unroll
        for (int k = 0; k < KT; ++k) mx = __builtin_fmax(mx, acc[k]);
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const double w = expw_tab(acc[k] - mx, ET);
            tot = tot + w;
            if (!LOO) acc[k] = w;  // the responsibilities' numerators
            if ((k & 1) == 1) __builtin_amdgcn_sched_barrier(0);  // two at a time: bounds the temporaries
        }
        if (MINUS) tot = tot + expw_tab(ownv - mx, ET);
        const double ld = seated ? mx + log_(tot) : qnan();  // (the host refuses a state with an unseated row)
        if (valid) {
            if (a.out) a.out[i] = ld;
            if (LOO) {
                if (a.acc) loo_fold(a, i, ld, ET);
            } else {
                if (a.run_max) predict_fold(a, i, ld, ET);
                if (a.resp || a.resp_acc) {  // uniform
#pragma unroll
                    for (int k = 0; k < KT; ++k) {
                        if (k < Kc) {
                            const double r = div_(acc[k], tot);
                            if (a.resp) a.resp[(int64_t)k * a.rows + i] = r;
                            if (a.resp_acc) a.resp_acc[(int64_t)k * a.rows + i] += r;
                        }
                    }
                }
            }
        }
        b0 = n0; b1 = n1; b2 = n2; b3 = n3;
        z = zn;
    }
}

// Any shape (more than kMaxCats categories or P > kMaxP: the shapes k_resample_generic takes; and a counting chain's
// leave-one-out above kLooMaxOwnKT accumulators): tables gathered from global memory, the scores in a per-thread
// scratch column scr[k * stride + thread], as there.  Same arithmetic and the same order of sums as k_score.
template <bool LOO>
__global__ __launch_bounds__(256) void k_score_generic(ChainParams p, ScoreArgs a, double* scr, int64_t stride) {
    const bool has_minus = LOO && !explicit_params(p.mode);
    const TableLayout L = layout_of(p, has_minus);
    const int GM = L.M;
    const double* const Tp = a.tab + L.tp();
    const double* const Tm = a.tab + L.tm();
    const double* const ET = a.tab + L.et();
    const int P = p.P, G = p.G, K = p.K, Kc = p.Kc, KT = p.KT;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // < stride: the host sizes the grid
    double* const my = scr + gid;
    for (int64_t i = gid; i < a.rows; i += (int64_t)gridDim.x * blockDim.x) {
        const int z = has_minus ? a.z[i] : -1;
        const bool seated = !has_minus || (unsigned)z < (unsigned)K;
        const int zc = has_minus && seated ? z : 0;
        double own = 0.0;
        if (has_minus)
            for (int g = 0; g < p.Gm; ++g)
                own = own + Tm[((size_t)g * KT + zc) * kGroupMm + field_from_x(a.X, a.Xb, a.rows, P, i, g, kGroupWm)];
        const double ownv = has_minus && seated ? own : neg_inf();  // one more category, summed last, as in k_score
        double mx = ownv;
        for (int k0 = 0; k0 < Kc; k0 += 16) {
            double acc[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = has_minus && k0 + j == z ? neg_inf() : 0.0;
            for (int g = 0; g < G; ++g) {
                const double* row = Tp + ((size_t)g * KT + k0) * GM + field_from_x(a.X, a.Xb, a.rows, P, i, g, p.W);
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (k0 + j < Kc) acc[j] = acc[j] + row[j * GM];
            }
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (k0 + j < Kc) {
                    my[(int64_t)(k0 + j) * stride] = acc[j];
                    mx = __builtin_fmax(mx, acc[j]);
                }
        }
        double tot = 0.0;
        for (int k = 0; k < Kc; ++k) {
            const double w = expw_tab(my[(int64_t)k * stride] - mx, ET);
            tot = tot + w;
            if (!LOO) my[(int64_t)k * stride] = w;
        }
        if (has_minus) tot = tot + expw_tab(ownv - mx, ET);
        const double ld = seated ? mx + log_(tot) : qnan();
        if (a.out) a.out[i] = ld;
        if (LOO) {
            if (a.acc) loo_fold(a, i, ld, ET);
            continue;
        }
        if (a.run_max) predict_fold(a, i, ld, ET);
        if (a.resp || a.resp_acc)
            for (int k = 0; k < Kc; ++k) {
                const double r = div_(my[(int64_t)k * stride], tot);
                if (a.resp) a.resp[(int64_t)k * a.rows + i] = r;
                if (a.resp_acc) a.resp_acc[(int64_t)k * a.rows + i] += r;
            }
    }
}

// ---- incomplete new rows: the observed cells scored, the missing cells predicted -----------
// A new row with missing cells is not in the fit, so a missing cell marginalises out exactly: its Bernoulli term sums
// to 1 and simply leaves the product.  The group tables of k_score cannot score a group with a hole in it, and taking
// the masked terms back out of an entry cancels (and is -inf - -inf where an explicit theta is 0 or 1), so the image
// is split by bit value instead, in doubles:
//   T1  [G][KT][M]   T1[g][k][m] = sum over the bits j set in m of e1[g*W + j]   (the x = 1 terms)
//   T0  [G][KT][M]   T0[g][k][m] = sum over the bits j set in m of e0[g*W + j]   (the x = 0 terms; features past P: 0)
//   Cp  [KT]         the category's constant, log w_k: it STARTS the accumulator -- group 0 may be wholly missing
//   E   [256]        the exp256 table
// With nib the data bits and mn the mask bits (1 = missing) of group g, the group adds T1[g][k][nib & ~mn] and
// T0[g][k][~nib & ~mn]: two reads per category and group, terms of observed cells only, and a complete group costs
// the same two reads.  The single-bit entry T1[g][k][1 << j] is t_kd(1) itself, so the joint of a missing cell,
//   log q_md = log sum_k exp(acc_k + T1[g_d][k][1 << j_d]),
// needs no further table.  The mask is a second set of bit planes laid out as the data planes are, and the missing
// cells of a row a CSR list (off[m] .. off[m+1] into the sorted (row, column) list).  A row, and so each of its cells,
// is owned by one lane: the streaming pairs (run_max, run_sum) of the row and (cell_max, cell_sum) of the cell are
// folded without atomics and in a fixed order.
struct SplitLayout {
    int G, KT, M;
    __host__ __device__ int t1() const { return 0; }
    __host__ __device__ int t0() const { return G * KT * M; }
    __host__ __device__ int cp() const { return 2 * G * KT * M; }
    __host__ __device__ int et() const { return cp() + KT + (KT & 1); }
    __host__ __device__ int doubles() const { return et() + 256; }
};
__host__ __device__ inline SplitLayout split_layout_of(const ChainParams& p) { return SplitLayout{p.G, p.KT, 1 << p.W}; }

struct NaScoreArgs {
    const uint32_t* Xb;   // data planes of the new rows (k_pack_bits)
    const uint32_t* Mb;   // mask planes, the same layout: bit set = the cell is missing
    int64_t rows;
    const double* tab;    // the split image (k_split_tables)
    const int64_t* off;   // [rows + 1] offsets of a row's missing cells in the sorted cell list
    const int32_t* col;   // [cells] their columns
    double* out;          // or null: [rows], this state's log p(x_O | state)
    double* resp;         // or null: [Kc][rows], this state's normalised category weights, from the observed cells
    double* cell;         // or null: [cells], this state's q / p = P(x_d = 1 | x_O, state)
    double* run_max;      // or null (nothing is folded): the row pairs, as ScoreArgs
    double* run_sum;
    double* resp_acc;     // or null
    double* cell_max;     // [cells] the cell pairs: sum_s q_md(s) = exp(cell_max) * cell_sum
    double* cell_sum;
};

// one entry of a split table: the terms e[] of the features of group g whose bit is set in m (chunk-local, as group_entry)
__device__ __forceinline__ double split_entry(const double* e, int g, int pc, unsigned m, int W) {
    double t = 0.0;
    for (int j = 0; j < W; ++j) {
        const int d = g * W + j;
        if (d < pc && ((m >> j) & 1u)) t = t + e[d];
    }
    return t;
}

// The split image of the chain's current state, one workgroup per category, 256 threads: roles 0 (x = 1), 1 (x = 0).
//   counting samplers   the count-table rules, BUILD_PREDICT, from the statistics as they stand (pending deltas added,
//                       nothing folded or cleared), exactly the terms and constants k_state_tables<false> writes
//   explicit samplers   from the sweep's pi / theta with the log_ arguments of k_sb_theta_tables: log_(pi_k),
//                       log_(theta_kd), log_(1.0 - theta_kd); an accumulator past K: -inf over all-zero tables
__global__ __launch_bounds__(256) void k_split_tables(ChainParams p, const int32_t* __restrict__ Nk,
                                                      const int32_t* __restrict__ S, const int32_t* __restrict__ dNk,
                                                      const int32_t* __restrict__ dS,
                                                      const double* __restrict__ alpha_ptr,
                                                      const double* __restrict__ pi, const double* __restrict__ theta,
                                                      double* __restrict__ tab) {
    __shared__ double e1[kMaxP], e0[kMaxP], cst[2];  // cst: Cp, the terms' denominator
    const int k = blockIdx.x;
    const SplitLayout L = split_layout_of(p);
    const int P = p.P, K = p.K, W = p.W, M = L.M;
    const bool is_label = k < K;
    const bool expl = explicit_params(p.mode);
    const size_t KP = (size_t)K * P;
    const int64_t n = !expl && is_label ? (int64_t)Nk[k] + delta_take(const_cast<int32_t*>(dNk), k, K) : 0;
    const CountRule r{BUILD_PREDICT, p.mode == MODE_DP, K, p.Ntot, p.beta, p.gamma, expl ? 1.0 : *alpha_ptr};
    const int role = threadIdx.x >> 7, dl = threadIdx.x & 127;
    if (threadIdx.x == 0) {
        if (expl) {
            cst[0] = is_label ? log_(pi[k]) : neg_inf();
            cst[1] = 0.0;
        } else {
            const double ak = rule_ak(r);
            double v[kRuleLogs];
#pragma unroll
            for (int j = 0; j < kRuleLogs; ++j) {
                double arg;
                v[j] = const_arg(r, ak, k, n, j, arg) ? log_(arg) : 0.0;
            }
            const CatConsts c = cat_consts(r, k, n, v);
            cst[0] = c.cp;
            cst[1] = c.den_p;
        }
        tab[L.cp() + k] = cst[0];
        if ((L.KT & 1) && k == 0) tab[L.cp() + L.KT] = 0.0;  // the pad
    }
    __syncthreads();
    for (int c0 = 0; c0 < P; c0 += kChunkP) {
        const int pc = P - c0 < kChunkP ? P - c0 : kChunkP;
        if (dl < pc) {
            const int d = c0 + dl;
            double t = 0.0;
            if (expl) {
                if (is_label) {
                    const double th = theta[k + (size_t)d * K];
                    t = role == 0 ? log_(th) : log_(1.0 - th);
                }
            } else {
                const int64_t s = is_label ? (int64_t)S[(size_t)k * P + d] + delta_take(const_cast<int32_t*>(dS), (size_t)k * P + d, KP) : 0;
                double arg;
                const bool have = term_arg(r, k, role, n, s, arg);
                t = term_of(have, have ? log_(arg) : 0.0, cst[1]);
            }
            (role == 0 ? e1 : e0)[dl] = t;
        }
        __syncthreads();
        const int g0 = c0 / W, gc = (pc + W - 1) / W;
        for (int idx = threadIdx.x; idx < gc * M; idx += blockDim.x) {
            const int g = idx / M;
            const unsigned m = idx % M;
            const size_t at = ((size_t)(g0 + g) * L.KT + k) * M + m;
            tab[L.t1() + at] = split_entry(e1, g, pc, m, W);
            tab[L.t0() + at] = split_entry(e0, g, pc, m, W);
        }
        __syncthreads();
    }
    if (k == 0) tab[L.et() + threadIdx.x] = exp256_table()[threadIdx.x];  // 256 threads
}

// one value's share of a streaming log-sum-exp pair (the arithmetic of predict_fold); ET the exp256 table
template <class Tab>
__device__ __forceinline__ void lse_fold(double* __restrict__ vmax, double* __restrict__ vsum, int64_t at, double v, Tab ET) {
    const double rm = vmax[at], rs = vsum[at];
    const bool up = v > rm;
    const double e = expw_tab(up ? rm - v : v - rm, ET);  // (-inf and NaN arguments give exactly 0)
    vmax[at] = up ? v : rm;
    vsum[at] = up ? rs * e + 1.0 : rs + e;
}

// The masked scorer, LDS form: the whole split image staged as k_score stages its head, one lane per new row, KT
// accumulators, NT threads; the next tile's words and mask words are loaded before this tile is scored.  After the
// max-shift and the total the lane walks its own missing cells while the accumulators are still live.
template <int KT, int NT, int GW>
__global__ __launch_bounds__(NT) void k_score_na(ChainParams p, NaScoreArgs a) {
    constexpr int GM = 1 << GW;
    constexpr int CH = KT <= 24 ? KT : (KT <= 48 ? KT / 2 : KT / 4);  // lookups issued together
    static_assert(KT % CH == 0, "chunking");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SplitLayout L{p.G, KT, GM};
    double* const lds = reinterpret_cast<double*>(smem);
    const volatile lds_f64* const T1 = (const volatile lds_f64*)(lds + L.t1());
    const volatile lds_f64* const T0 = (const volatile lds_f64*)(lds + L.t0());
    const volatile lds_f64* const CP = (const volatile lds_f64*)(lds + L.cp());
    const lds_f64* const ET = (const lds_f64*)(lds + L.et());
    const int P = p.P, G = p.G, Kc = p.Kc;
    const int tid = threadIdx.x;
    const int W = (P + 31) / 32;
    const int64_t ntiles = (a.rows + NT - 1) / NT;
    int64_t tile = blockIdx.x;
    uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0, m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    if (tile < ntiles) {  // the first tile's words go out before the image is staged
        const int64_t i0 = tile * NT + tid;
        const int64_t ic = i0 < a.rows ? i0 : a.rows - 1;
        load_words(a.Xb, a.rows, W, ic, b0, b1, b2, b3);
        load_words(a.Mb, a.rows, W, ic, m0, m1, m2, m3);
    }
    {
        const double2* src = reinterpret_cast<const double2*>(a.tab);
        double2* dst = reinterpret_cast<double2*>(smem);
        const int n2 = L.doubles() / 2;  // even: every piece of the layout is
        for (int i0 = tid; i0 < n2; i0 += NT * 8) {
            double2 t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * NT;
                t[u] = src[i < n2 ? i : n2 - 1];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * NT;
                if (i < n2) dst[i] = t[u];
            }
        }
    }
    __syncthreads();
    for (; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * NT + tid;
        const bool valid = i < a.rows;
        const int64_t tnext = tile + gridDim.x;
        uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0, q0 = 0, q1 = 0, q2 = 0, q3 = 0;
        if (tnext < ntiles) {
            const int64_t in = tnext * NT + tid;
            const int64_t ic = in < a.rows ? in : a.rows - 1;
            load_words(a.Xb, a.rows, W, ic, n0, n1, n2, n3);
            load_words(a.Mb, a.rows, W, ic, q0, q1, q2, q3);
        }
        double acc[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) acc[k] = CP[k];
#pragma unroll 1
        for (int h = 0; h < W; ++h) {
            const uint32_t cur = word_of(h, b0, b1, b2, b3), nxt = word_of(h + 1, b0, b1, b2, b3);
            const uint32_t mcur = word_of(h, m0, m1, m2, m3), mnxt = word_of(h + 1, m0, m1, m2, m3);
            const int g_lo = (32 * h + GW - 1) / GW;
            int g_hi = (32 * (h + 1) + GW - 1) / GW;
            g_hi = g_hi < G ? g_hi : G;
#pragma unroll 1
            for (int g = g_lo; g < g_hi; ++g) {
                const unsigned sh = (unsigned)(g * GW - 32 * h);
                const unsigned nib = __builtin_amdgcn_alignbit(nxt, cur, sh), mn = __builtin_amdgcn_alignbit(mnxt, mcur, sh);
                const unsigned o1 = nib & ~mn & (unsigned)(GM - 1), o0 = ~nib & ~mn & (unsigned)(GM - 1);
                const volatile lds_f64* row1 = T1 + ((size_t)g * KT * GM + o1);
                const volatile lds_f64* row0 = T0 + ((size_t)g * KT * GM + o0);
#pragma unroll
                for (int c0 = 0; c0 < KT; c0 += CH) {
                    double tv[CH];
#pragma unroll
                    for (int j = 0; j < CH; ++j) tv[j] = row1[(c0 + j) * GM];
#pragma unroll
                    for (int j = 0; j < CH; ++j) acc[c0 + j] = acc[c0 + j] + tv[j];
                    __builtin_amdgcn_sched_barrier(0);  // keep the chunks apart
#pragma unroll
                    for (int j = 0; j < CH; ++j) tv[j] = row0[(c0 + j) * GM];
#pragma unroll
                    for (int j = 0; j < CH; ++j) acc[c0 + j] = acc[c0 + j] + tv[j];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        double mx = neg_inf();
#pragma unroll
        for (int k = 0; k < KT; ++k) mx = __builtin_fmax(mx, acc[k]);
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            tot = tot + expw_tab(acc[k] - mx, ET);
            if ((k & 1) == 1) __builtin_amdgcn_sched_barrier(0);  // two at a time: bounds the temporaries
        }
        const double ld = mx + log_(tot);
        if (valid) {
            if (a.out) a.out[i] = ld;
            if (a.run_max) lse_fold(a.run_max, a.run_sum, i, ld, ET);
            // the row's missing cells: the joint with x_d = 1 from the live accumulators and the single-bit entry
            const int64_t q_end = a.off[i + 1];
#pragma unroll 1
            for (int64_t q = a.off[i]; q < q_end; ++q) {
                const int d = a.col[q];
                const int g = d / GW, j = d - g * GW;
                const volatile lds_f64* r1 = T1 + ((size_t)g * KT * GM + (1u << j));
                // t_kd(1) <= 1: the row's own shift mx bounds every term of the joint, so one pass does (a second
                // maximum would keep KT more sums live: scratch from 32 accumulators on)
                double cs = 0.0;
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    cs = cs + expw_tab((acc[k] + r1[k * GM]) - mx, ET);
                    if ((k & 1) == 1) __builtin_amdgcn_sched_barrier(0);
                }
                const double lj = mx + log_(cs);
                if (a.cell) a.cell[q] = expw_tab(lj - ld, ET);
                if (a.cell_max) lse_fold(a.cell_max, a.cell_sum, q, lj, ET);
            }
            if (a.resp || a.resp_acc) {  // uniform
                // the column stride in a VGPR: as a scalar the compiler keeps all KT column offsets of both matrices
                // live across the tile loop (over a hundred spilled SGPRs at 28 accumulators)
                int64_t ld_resp = a.rows;
                asm volatile("" : "+v"(ld_resp));
                int64_t at = i;
                double mx_r = mx;  // the weights are computed again here, not kept live through the cell pass
                asm volatile("" : "+v"(mx_r));
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    if (k < Kc) {  // (a break here turns acc into an indexed array: a private segment)
                        const double r = div_(expw_tab(acc[k] - mx_r, ET), tot);
                        if (a.resp) a.resp[at] = r;
                        if (a.resp_acc) a.resp_acc[at] += r;
                    }
                    at += ld_resp;
                }
            }
        }
        b0 = n0; b1 = n1; b2 = n2; b3 = n3;
        m0 = q0; m1 = q1; m2 = q2; m3 = q3;
    }
}

// The masked scorer, global form: the doubled head does not fit in LDS, or the shape is k_resample_generic's.  Tables
// gathered from global memory (L2), the scores in a per-thread scratch column scr[k * stride + thread] as
// k_score_generic keeps them.  Same arithmetic and the same order of sums as k_score_na.
__global__ __launch_bounds__(256) void k_score_na_generic(ChainParams p, NaScoreArgs a, double* scr, int64_t stride) {
    const SplitLayout L = split_layout_of(p);
    const int GM = L.M;
    const double* const T1 = a.tab + L.t1();
    const double* const T0 = a.tab + L.t0();
    const double* const CP = a.tab + L.cp();
    const double* const ET = a.tab + L.et();
    const int P = p.P, G = p.G, Kc = p.Kc, KT = p.KT, GW = p.W;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // < stride: the host sizes the grid
    double* const my = scr + gid;
    for (int64_t i = gid; i < a.rows; i += (int64_t)gridDim.x * blockDim.x) {
        double mx = neg_inf();
        for (int k0 = 0; k0 < Kc; k0 += 16) {
            double acc[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = k0 + j < Kc ? CP[k0 + j] : 0.0;
            for (int g = 0; g < G; ++g) {
                const unsigned nib = field_from_x(nullptr, a.Xb, a.rows, P, i, g, GW);
                const unsigned mn = field_from_x(nullptr, a.Mb, a.rows, P, i, g, GW);
                const unsigned o1 = nib & ~mn & (unsigned)(GM - 1), o0 = ~nib & ~mn & (unsigned)(GM - 1);
                const double* row1 = T1 + ((size_t)g * KT + k0) * GM + o1;
                const double* row0 = T0 + ((size_t)g * KT + k0) * GM + o0;
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (k0 + j < Kc) acc[j] = (acc[j] + row1[j * GM]) + row0[j * GM];
            }
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (k0 + j < Kc) {
                    my[(int64_t)(k0 + j) * stride] = acc[j];
                    mx = __builtin_fmax(mx, acc[j]);
                }
        }
        double tot = 0.0;
        for (int k = 0; k < Kc; ++k) tot = tot + expw_tab(my[(int64_t)k * stride] - mx, ET);
        const double ld = mx + log_(tot);
        if (a.out) a.out[i] = ld;
        if (a.run_max) lse_fold(a.run_max, a.run_sum, i, ld, ET);
        const int64_t q_end = a.off[i + 1];
        for (int64_t q = a.off[i]; q < q_end; ++q) {
            const int d = a.col[q];
            const int g = d / GW, j = d - g * GW;
            const double* r1 = T1 + (size_t)g * KT * GM + (1u << j);
            double cs = 0.0;  // (the row's own shift, as k_score_na)
            for (int k = 0; k < Kc; ++k) cs = cs + expw_tab((my[(int64_t)k * stride] + r1[(size_t)k * GM]) - mx, ET);
            const double lj = mx + log_(cs);
            if (a.cell) a.cell[q] = expw_tab(lj - ld, ET);
            if (a.cell_max) lse_fold(a.cell_max, a.cell_sum, q, lj, ET);
        }
        if (a.resp || a.resp_acc)
            for (int k = 0; k < Kc; ++k) {
                const double r = div_(expw_tab(my[(int64_t)k * stride] - mx, ET), tot);
                if (a.resp) a.resp[(int64_t)k * a.rows + i] = r;
                if (a.resp_acc) a.resp_acc[(int64_t)k * a.rows + i] += r;
            }
    }
}

// The cell pairs after the folded states: cell_mean = sum_s q_md(s) / sum_s p(x_O | s), the states weighted by the
// density of the row's observed cells (the chain samples s | X, not s | X, x_O).  The number of states cancels.  The
// accumulators are left as they are, so more sweeps may be folded afterwards.
__global__ __launch_bounds__(256) void k_predict_cells_finish(int64_t cells, const int64_t* __restrict__ row,
                                                              const double* __restrict__ run_max,
                                                              const double* __restrict__ run_sum,
                                                              const double* __restrict__ cell_max,
                                                              const double* __restrict__ cell_sum,
                                                              double* __restrict__ cell_mean) {
    const double* const ET = exp256_table();
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < cells; q += (int64_t)gridDim.x * 256) {
        const int64_t m = row[q];
        cell_mean[q] = expw_tab((cell_max[q] + log_(cell_sum[q])) - (run_max[m] + log_(run_sum[m])), ET);
    }
}

// empty accumulators: no state folded
__global__ __launch_bounds__(256) void k_loo_reset(int64_t N, double* __restrict__ acc) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        acc[LOO_MAX * N + i] = neg_inf();
        acc[LOO_SUM * N + i] = 0.0;
        acc[LOO_MIN * N + i] = pos_inf();
        acc[LOO_S1 * N + i] = 0.0;
        acc[LOO_S2 * N + i] = 0.0;
        acc[LOO_MEAN * N + i] = 0.0;
        acc[LOO_M2 * N + i] = 0.0;
    }
}

// The per-row outputs after n folded states, into a buffer of their own ([kLooOut][N]: log_cpo, ess, lppd, mean,
// var); the accumulators are left as they are, so more sweeps may be folded afterwards.
//   log_cpo = log n - logsumexp(-ell) = log n + MIN - log S1        ess = S1^2 / S2
//   lppd    = MAX + log SUM - log n                                 var = M2 / (n - 1), NaN when n = 1
__global__ __launch_bounds__(256) void k_loo_finish(int64_t N, int n, const double* __restrict__ acc,
                                                    double* __restrict__ out) {
    const double ln = log_((double)n);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const double s1 = acc[LOO_S1 * N + i];
        out[0 * N + i] = (ln + acc[LOO_MIN * N + i]) - log_(s1);
        out[1 * N + i] = div_(s1 * s1, acc[LOO_S2 * N + i]);
        out[2 * N + i] = (acc[LOO_MAX * N + i] + log_(acc[LOO_SUM * N + i])) - ln;
        out[3 * N + i] = acc[LOO_MEAN * N + i];
        out[4 * N + i] = n > 1 ? div_(acc[LOO_M2 * N + i], (double)(n - 1)) : qnan();
    }
}

// The scalars, in an order fixed by N alone: 1024 partial sums (row i in partial i mod 1024, ascending), then a
// binary tree.  One workgroup.  scal: lpml = sum log_cpo, min ess, sum lppd, p_waic = sum var,
// elpd_waic = sum lppd - p_waic.
__global__ __launch_bounds__(1024) void k_loo_reduce(int64_t N, const double* __restrict__ out, double* __restrict__ scal) {
    __shared__ double sh[4][1024];
    const int t = threadIdx.x;
    double cpo = 0.0, lp = 0.0, vr = 0.0, es = pos_inf();
    for (int64_t i = t; i < N; i += 1024) {
        cpo = cpo + out[0 * N + i];
        es = __builtin_fmin(es, out[1 * N + i]);
        lp = lp + out[2 * N + i];
        vr = vr + out[4 * N + i];
    }
    sh[0][t] = cpo; sh[1][t] = es; sh[2][t] = lp; sh[3][t] = vr;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (t < s) {
            sh[0][t] = sh[0][t] + sh[0][t + s];
            sh[1][t] = __builtin_fmin(sh[1][t], sh[1][t + s]);
            sh[2][t] = sh[2][t] + sh[2][t + s];
            sh[3][t] = sh[3][t] + sh[3][t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        scal[0] = sh[0][0]; scal[1] = sh[1][0]; scal[2] = sh[2][0]; scal[3] = sh[3][0];
        scal[4] = sh[2][0] - sh[3][0];
    }
}

// ---- self-check kernels ----------------------------------------------------------
__global__ void k_test_math(int op, const double* in, const double* in2, double* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = in[i];
    double y;
    if (op == 0) y = log_(x);
    else if (op == 1) y = exp_(x);
    else if (op == 2) y = div_(x, in2[i]);
    else if (op == 3) y = sqrt_(x);
    else y = expw_(x);
    out[i] = y;
}
#ifdef BMM_DEBUG_HOOKS
// Test variant: k_resample_pk's draw (pk_draw2; SPEC = false) or the statement it is held to (draw_pk, bmm_spec.h;
// SPEC = true) on rows of scores and their uniforms, one row per lane; the maximum is taken as the kernel takes it.
// out[2 i ...]: count and verdict.  Two kernels, so that neither draw shares a subexpression with the other
// (tests/test_gpu_pk_lean.py compares them).
template <int KT, bool SPEC>
__global__ __launch_bounds__(256) void k_test_pk_draw(const float* __restrict__ scores, const double* __restrict__ u,
                                                      int G, int64_t n, int* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float sc[KT];
    float m = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        sc[k] = scores[i * KT + k];
        m = __builtin_fmaxf(m, sc[k]);
    }
    int cnt = 0;
    bool ok;
    if constexpr (SPEC) {
        ok = draw_pk<KT>(sc, m, u[i], G, kPkEpsUnit, cnt);
    } else {
        pk_f2 s2[KT / 2];
#pragma unroll
        for (int j = 0; j < KT / 2; ++j) s2[j] = pk_f2{sc[2 * j], sc[2 * j + 1]};
        ok = pk_draw2<KT>(s2, m, u[i], G, kPkEpsUnit, cnt);
    }
    out[2 * i] = cnt; out[2 * i + 1] = ok ? 1 : 0;
}
#endif
__global__ void k_test_variates(int kind, double pp, double qq, uint64_t seed, uint32_t sweep, double* out,
                                int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double y;
    if (kind == 0) {
        Stream s = make_stream(seed, (uint32_t)i, sweep, kStreamThetaA);
        y = rgamma_(pp, s);
    } else if (kind == 1) {
        Stream sa = make_stream(seed, (uint32_t)i, sweep, kStreamThetaA);
        Stream sb = make_stream(seed, (uint32_t)i, sweep, kStreamThetaB);
        y = rbeta_(pp, qq, sa, sb);
    } else {
        y = update_alpha_(pp, 1.0, 1.0, 1000.0, (int)qq, seed + (uint64_t)i, sweep);
    }
    out[i] = y;
}
// The same with parameters per element (bmm_device_variates_ex): kind 0 gamma(p[i]), 1 beta(p[i], q[i]), 2
// update_alpha_ from alpha_old = p[i] with K = (int)q[i] under (a, b, N); stream index and seed offset i as above.
__global__ void k_test_variates_ex(int kind, const double* __restrict__ p, const double* __restrict__ q, double a,
                                   double b, double N, uint64_t seed, uint32_t sweep, double* __restrict__ out,
                                   int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double y;
    if (kind == 0) {
        Stream s = make_stream(seed, (uint32_t)i, sweep, kStreamThetaA);
        y = rgamma_(p[i], s);
    } else if (kind == 1) {
        Stream sa = make_stream(seed, (uint32_t)i, sweep, kStreamThetaA);
        Stream sb = make_stream(seed, (uint32_t)i, sweep, kStreamThetaB);
        y = rbeta_(p[i], q[i], sa, sb);
    } else {
        y = update_alpha_(p[i], a, b, N, (int)q[i], seed + (uint64_t)i, sweep);
    }
    out[i] = y;
}
// Kind 3: update_alpha_wave as the kernels call it, one whole wave per element, lane 0's value.  256 threads.
__global__ __launch_bounds__(256) void k_test_alpha_wave(const double* __restrict__ p, const double* __restrict__ q,
                                                         double a, double b, double N, uint64_t seed, uint32_t sweep,
                                                         double* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // uniform over the wave
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    const double y = update_alpha_wave(p[i], a, b, N, (int)q[i], seed + (uint64_t)i, sweep, lane);
    if (lane == 0) out[i] = y;
}
// Kind 4: Beta(p[i], q[i]) split over two threads exactly as k_sb_theta_tables draws theta: thread dl of the first
// 128 draws X, thread 128 + dl draws Y (sb_theta_half), LDS and a barrier between them and the quotient.  256 threads.
__global__ __launch_bounds__(256) void k_test_split_beta(const double* __restrict__ p, const double* __restrict__ q,
                                                         uint64_t seed, uint32_t sweep, double* __restrict__ out,
                                                         int64_t n) {
    __shared__ double gam[2][128];
    const int half = threadIdx.x >> 7, dl = threadIdx.x & 127;
    const int64_t i = (int64_t)blockIdx.x * 128 + dl;
    if (i < n) gam[half][dl] = sb_theta_half(seed, (uint32_t)i, sweep, half, half ? q[i] : p[i]);
    __syncthreads();
    if (i < n && half == 0) out[i] = rbeta_join_(gam[0][dl], gam[1][dl]);
}

// ---- partition summaries over a label trace (include/bmm_mcmc.h "clustering point estimate")
// Labels are 0-based, one row of `pitch` labels per kept sweep (pitch a multiple of 16, so that every row starts on
// a 16-byte boundary; the cells past N are never read), one byte each up to 256 categories, int32 above.  Every
// count is an integer and every floating-point sum runs in an order that depends on the shape alone: each of the
// 256 threads adds its cells in ascending order (cell k belongs to thread k mod 256), then a binary tree over the
// threads.  No float atomics anywhere: results do not depend on scheduling.
constexpr int kPtThreads = 256;
constexpr int kPtMaxLdsK = 64;  // tables of Kc^2 uint32 bins in LDS up to here (16 KB each at 64)

template <class T>
__device__ inline T pt_block_sum(T v, T* slot) {
    const int tid = threadIdx.x;
    __syncthreads();
    slot[tid] = v;
    __syncthreads();
    for (int h = kPtThreads / 2; h > 0; h >>= 1) {
        if (tid < h) slot[tid] += slot[tid + h];
        __syncthreads();
    }
    return slot[0];
}
__device__ inline double pt_f(uint32_t n) { return n ? (double)n * log_((double)n) : 0.0; }  // f(n) = n log n, f(0) = 0

// Label (s, i) of the source, at src[s * ss + li * si] for li = i - i0 in [0, rows), minus `base`, into row s of the
// label block: a 32 x 32 tile through LDS, read along whichever of the two source strides is 1 (the resident trace
// has si = 1; a block of the caller's S x N column-major matrix has ss = 1) and written along i.  A label outside
// 0 .. Kc-1 raises the flag and is stored as 0: nothing downstream indexes out of its tables.
template <class L>
__global__ __launch_bounds__(256) void k_pt_narrow(const int32_t* __restrict__ src, int64_t ss, int64_t si, int base,
                                                   int S, int64_t i0, int64_t rows, int Kc, L* __restrict__ out,
                                                   int64_t pitch, int* __restrict__ flag) {
    __shared__ int32_t tile[32][33];
    const int64_t b0 = (int64_t)blockIdx.x * 32;
    const int s0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        if (si == 1) {
            const int s = s0 + r;
            const int64_t li = b0 + tx;
            tile[r][tx] = (s < S && li < rows) ? src[(size_t)s * ss + li] : base;
        } else {
            const int s = s0 + tx;
            const int64_t li = b0 + r;
            tile[tx][r] = (s < S && li < rows) ? src[(size_t)s * ss + (size_t)li * si] : base;
        }
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int s = s0 + r;
        const int64_t li = b0 + tx;
        if (s < S && li < rows) {
            int v = tile[r][tx] - base;
            if ((uint32_t)v >= (uint32_t)Kc) { *flag = 1; v = 0; }
            out[(size_t)s * pitch + i0 + li] = (L)v;
        }
    }
}

// Row s: the cluster sizes n_a (one histogram per wave in LDS), A[s] = sum_a n_a^2 and F[s] = sum_a f(n_a).
// Dynamic LDS: 4 * Kc uint32.
template <class L>
__global__ __launch_bounds__(256) void k_pt_sizes(const L* __restrict__ lab, int64_t pitch, int64_t N, int Kc,
                                                  uint64_t* __restrict__ A, double* __restrict__ F) {
    extern __shared__ uint32_t pt_lds[];
    __shared__ uint64_t su[kPtThreads];
    __shared__ double sd[kPtThreads];
    const int tid = threadIdx.x;
    for (int k = tid; k < 4 * Kc; k += kPtThreads) pt_lds[k] = 0;
    __syncthreads();
    const L* __restrict__ row = lab + (size_t)blockIdx.x * pitch;
    uint32_t* const h = pt_lds + (tid >> 6) * Kc;
    for (int64_t i = tid; i < N; i += kPtThreads) atomicAdd(&h[(uint32_t)row[i]], 1u);
    __syncthreads();
    uint64_t a = 0;
    double f = 0.0;
    for (int k = tid; k < Kc; k += kPtThreads) {
        const uint32_t n = pt_lds[k] + pt_lds[Kc + k] + pt_lds[2 * Kc + k] + pt_lds[3 * Kc + k];
        a += (uint64_t)n * n;
        f += pt_f(n);
    }
    a = pt_block_sum(a, su);
    f = pt_block_sum(f, sd);
    if (tid == 0) { A[blockIdx.x] = a; F[blockIdx.x] = f; }
}

// The hot path.  Workgroup (x, y): candidate row rc = y * stride against the draws t of block x, [x * T, x * T + T),
// one pass over all N (a contingency table must be complete before it is squared: the split is over pairs, never
// over N).  Per draw a table of Kc^2 uint32 bins in LDS, key a * Kc + b, filled with LDS integer adds that return
// nothing; R copies of each table, the waves of the workgroup spread over them (the few big clusters put most lanes
// of a wave on a handful of bins).  Byte labels, four per dword.  At the end each table becomes one cell of
// Q[y][t] = sum_ab n_ab^2 and, for VI, G[y][t] = sum_ab f(n_ab).  tri (every row a candidate, stride 1): only
// t > rc is counted and the cell is mirrored.  Dynamic LDS: T * R * Kc^2 uint32.
template <bool VI>
__global__ __launch_bounds__(256) void k_pt_pairs(const uint8_t* __restrict__ lab, int64_t pitch, int64_t N, int S,
                                                  int Kc, int stride, int T, int R, int tri,
                                                  uint64_t* __restrict__ Q, double* __restrict__ G) {
    extern __shared__ uint32_t pt_lds[];
    __shared__ uint64_t su[kPtThreads];
    __shared__ double sd[kPtThreads];
    const int tid = threadIdx.x;
    const int c = blockIdx.y, rc = c * stride;
    int t0 = blockIdx.x * T;
    const int t1 = t0 + T < S ? t0 + T : S;
    if (tri && t0 <= rc) t0 = rc + 1;
    if (t0 >= t1) return;  // the whole workgroup
    const int nT = t1 - t0, KK = Kc * Kc, TS = R * KK;
    for (int k = tid; k < nT * TS; k += kPtThreads) pt_lds[k] = 0;
    __syncthreads();
    uint32_t* const mine = pt_lds + ((tid >> 6) % R) * KK;  // table tt, copy r at (tt * R + r) * KK
    const uint8_t* __restrict__ ca = lab + (size_t)rc * pitch;
    const uint8_t* __restrict__ da = lab + (size_t)t0 * pitch;
    const int64_t W = N >> 2;
    for (int64_t w = tid; w < W; w += kPtThreads) {
        const uint32_t a4 = reinterpret_cast<const uint32_t*>(ca)[w];
        const uint32_t k0 = (a4 & 255u) * Kc, k1 = ((a4 >> 8) & 255u) * Kc, k2 = ((a4 >> 16) & 255u) * Kc, k3 = (a4 >> 24) * Kc;
#pragma unroll 4
        for (int tt = 0; tt < nT; ++tt) {
            if (t0 + tt == rc) continue;  // a row against itself is never used (k_pt_loss): no pass over it
            const uint32_t b4 = reinterpret_cast<const uint32_t*>(da + (size_t)tt * pitch)[w];
            uint32_t* const tb = mine + tt * TS;
            atomicAdd(tb + k0 + (b4 & 255u), 1u);
            atomicAdd(tb + k1 + ((b4 >> 8) & 255u), 1u);
            atomicAdd(tb + k2 + ((b4 >> 16) & 255u), 1u);
            atomicAdd(tb + k3 + (b4 >> 24), 1u);
        }
    }
    for (int64_t i = (W << 2) + tid; i < N; i += kPtThreads) {
        const uint32_t k0 = (uint32_t)ca[i] * Kc;
        for (int tt = 0; tt < nT; ++tt)
            if (t0 + tt != rc) atomicAdd(mine + tt * TS + k0 + da[(size_t)tt * pitch + i], 1u);
    }
    __syncthreads();
    for (int tt = 0; tt < nT; ++tt) {
        uint64_t q = 0;
        double g = 0.0;
        for (int k = tid; k < KK; k += kPtThreads) {
            uint32_t n = 0;
            for (int r = 0; r < R; ++r) n += pt_lds[(tt * R + r) * KK + k];
            q += (uint64_t)n * n;
            if (VI) g += pt_f(n);
        }
        q = pt_block_sum(q, su);
        if (VI) g = pt_block_sum(g, sd);
        if (tid == 0) {
            const int t = t0 + tt;
            Q[(size_t)c * S + t] = q;
            if (VI) G[(size_t)c * S + t] = g;
            if (tri) {
                Q[(size_t)t * S + c] = q;
                if (VI) G[(size_t)t * S + c] = g;
            }
        }
    }
}

// The same for more than kPtMaxLdsK categories (up to the 1024 the generic resample path takes): one table of
// Kc^2 uint32 per workgroup in global memory, zeroed per pair, filled with global integer adds and read back past
// the L1, the workgroups striding over the C x S pairs.  A correctness fallback, as k_resample_generic is.
template <class L, bool VI>
__global__ __launch_bounds__(256) void k_pt_pairs_generic(const L* __restrict__ lab, int64_t pitch, int64_t N, int S,
                                                          int Kc, int stride, int C, int tri, uint32_t* tabs,
                                                          uint64_t* __restrict__ Q, double* __restrict__ G) {
    __shared__ uint64_t su[kPtThreads];
    __shared__ double sd[kPtThreads];
    const int tid = threadIdx.x;
    const size_t KK = (size_t)Kc * Kc;
    uint32_t* const tab = tabs + (size_t)blockIdx.x * KK;
    for (int64_t p = blockIdx.x; p < (int64_t)C * S; p += gridDim.x) {
        const int c = (int)(p / S), t = (int)(p % S), rc = c * stride;
        if (tri ? t <= rc : t == rc) continue;  // the whole workgroup
        for (size_t k = tid; k < KK; k += kPtThreads) __hip_atomic_store(tab + k, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        __syncthreads();
        const L* __restrict__ ca = lab + (size_t)rc * pitch;
        const L* __restrict__ da = lab + (size_t)t * pitch;
        for (int64_t i = tid; i < N; i += kPtThreads) atomicAdd(tab + (size_t)(uint32_t)ca[i] * Kc + (uint32_t)da[i], 1u);
        __threadfence();
        __syncthreads();
        uint64_t q = 0;
        double g = 0.0;
        for (size_t k = tid; k < KK; k += kPtThreads) {
            const uint32_t n = __hip_atomic_load(tab + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            q += (uint64_t)n * n;
            if (VI) g += pt_f(n);
        }
        q = pt_block_sum(q, su);
        if (VI) g = pt_block_sum(g, sd);
        if (tid == 0) {
            Q[(size_t)c * S + t] = q;
            if (VI) G[(size_t)c * S + t] = g;
            if (tri) {
                Q[(size_t)t * S + c] = q;
                if (VI) G[(size_t)t * S + c] = g;
            }
        }
    }
}

// Candidate c (row rc = c * stride) against every draw: 2 B(rc, t) = A[rc] + A[t] - 2 Q[c][t], exact in uint64, and
// VI(rc, t) = (F[rc] + F[t] - 2 G[c][t]) / N -- exactly 0 on the diagonal (not computed) and wherever the Binder
// distance is 0 (the two rows are one partition).  sum2[c] = sum_t 2 B, loss[c] = sum2 / (2 S) or the mean VI;
// dist, unless null, is C x S column-major: B as a double (exact below 2^53) or VI.
__global__ __launch_bounds__(256) void k_pt_loss(const uint64_t* __restrict__ A, const double* __restrict__ F,
                                                 const uint64_t* __restrict__ Q, const double* __restrict__ G, int S,
                                                 int C, int stride, int64_t N, int vi, uint64_t* __restrict__ sum2,
                                                 double* __restrict__ loss, double* __restrict__ dist) {
    __shared__ uint64_t su[kPtThreads];
    __shared__ double sd[kPtThreads];
    const int tid = threadIdx.x, c = blockIdx.x, rc = c * stride;
    uint64_t b = 0;
    double v = 0.0;
    for (int t = tid; t < S; t += kPtThreads) {
        uint64_t d2 = 0;
        double dv = 0.0;
        if (t != rc) {
            d2 = A[rc] + A[t] - 2 * Q[(size_t)c * S + t];
            if (vi && d2 != 0) dv = (F[rc] + F[t] - 2.0 * G[(size_t)c * S + t]) / (double)N;
        }
        b += d2;
        v += dv;
        if (dist) dist[(size_t)c + (size_t)C * t] = vi ? dv : (double)(d2 >> 1);
    }
    b = pt_block_sum(b, su);
    v = pt_block_sum(v, sd);
    if (tid == 0) {
        sum2[c] = b;
        loss[c] = vi ? v / (double)S : (double)b / (2.0 * (double)S);
    }
}

// the candidate with the smallest loss (Binder: the exact integer total; VI: the double), lowest index on ties
__global__ __launch_bounds__(256) void k_pt_argmin(const uint64_t* __restrict__ sum2, const double* __restrict__ loss,
                                                   int C, int vi, int* __restrict__ best) {
    __shared__ int idx[kPtThreads];
    const int tid = threadIdx.x;
    auto less = [&](int i, int j) {  // i beats j
        if (j < 0) return i >= 0;
        if (i < 0) return false;
        if (vi) return loss[i] < loss[j] || (loss[i] == loss[j] && i < j);
        return sum2[i] < sum2[j] || (sum2[i] == sum2[j] && i < j);
    };
    int m = -1;
    for (int c = tid; c < C; c += kPtThreads) if (less(c, m)) m = c;
    idx[tid] = m;
    __syncthreads();
    for (int h = kPtThreads / 2; h > 0; h >>= 1) {
        if (tid < h && less(idx[tid + h], idx[tid])) idx[tid] = idx[tid + h];
        __syncthreads();
    }
    if (tid == 0) *best = idx[0];
}

// the labels of the chosen observations, gathered once: g[s][u] = lab[s][idx[u]]
template <class L>
__global__ __launch_bounds__(256) void k_pt_gather(const L* __restrict__ lab, int64_t pitch, const int64_t* __restrict__ idx,
                                                   int64_t M, L* __restrict__ g) {
    const int64_t u = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
    if (u < M) g[(size_t)blockIdx.y * M + u] = lab[(size_t)blockIdx.y * pitch + idx[u]];
}
// Posterior similarity counts cnt[u][v] = #{s : g[s][u] == g[s][v]}: a 64 x 64 tile per workgroup, 4 x 4 cells per
// thread, the counts in registers over all S rows and stored once; tiles on or above the diagonal, mirrored on store.
template <class L>
__global__ __launch_bounds__(256) void k_pt_psm(const L* __restrict__ g, int S, int64_t M, uint32_t* __restrict__ cnt) {
    if (blockIdx.x < blockIdx.y) return;
    const int64_t u0 = (int64_t)blockIdx.y * 64 + (threadIdx.x >> 4) * 4;
    const int64_t v0 = (int64_t)blockIdx.x * 64 + (threadIdx.x & 15) * 4;
    uint32_t n[4][4] = {};
    for (int s = 0; s < S; ++s) {
        const L* __restrict__ row = g + (size_t)s * M;
        L lu[4], lv[4];
        for (int a = 0; a < 4; ++a) {
            lu[a] = u0 + a < M ? row[u0 + a] : (L)0;
            lv[a] = v0 + a < M ? row[v0 + a] : (L)0;
        }
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) n[a][b] += lu[a] == lv[b] ? 1u : 0u;
    }
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b)
            if (u0 + a < M && v0 + b < M) {
                cnt[(size_t)(u0 + a) * M + (v0 + b)] = n[a][b];
                cnt[(size_t)(v0 + b) * M + (u0 + a)] = n[a][b];
            }
}

// ---- greedy search for the point estimate (include/bmm_mcmc.h "greedy search") ----------
// The candidate c is N int32 slots in 0 .. Ka-1, the draws are the byte label block of k_pt_narrow.  One table per
// draw, T[t][b][a] = #{i : c_i = a, z_t,i = b}, uint32, laid out [b][a] with the b stride KaP = 8 * ceil(Ka / 8) + 4
// (the cells past Ka stay 0), in global memory between the launches and in LDS inside k_ps_score -- the two layouts
// are the same, so staging a block of draws is one flat copy.  A row reads runs of kPsChunk slots, 16-byte aligned.
// Every count is an integer; every floating-point sum runs in an order fixed by the shape.  No float atomics.
constexpr int kPsChunk = 8;  // slots per thread of k_ps_score

// Tables and sizes from c and the label block (both zeroed by the caller): workgroup (x, t) adds the rows
// [x * span, x * span + span) of draw t into a table in LDS and flushes its non-zero cells with integer adds; the
// workgroups of draw 0 also count the sizes n_a.  Dynamic LDS: Kc * KaP + KaP uint32.
__global__ __launch_bounds__(256) void k_ps_tables(const uint8_t* __restrict__ lab, int64_t pitch, int64_t N, int Kc,
                                                   int KaP, int64_t span, const int32_t* __restrict__ c,
                                                   uint32_t* __restrict__ T, uint32_t* __restrict__ n) {
    extern __shared__ uint32_t pt_lds[];
    const int tid = threadIdx.x, t = blockIdx.y, cells = Kc * KaP;
    for (int k = tid; k < cells + KaP; k += kPtThreads) pt_lds[k] = 0;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * span, i1 = i0 + span < N ? i0 + span : N;
    const uint8_t* __restrict__ row = lab + (size_t)t * pitch;
    for (int64_t i = i0 + tid; i < i1; i += kPtThreads) {
        const int a = c[i];
        atomicAdd(&pt_lds[(uint32_t)row[i] * KaP + a], 1u);
        if (t == 0) atomicAdd(&pt_lds[cells + a], 1u);
    }
    __syncthreads();
    uint32_t* const Tt = T + (size_t)t * cells;
    for (int k = tid; k < cells; k += kPtThreads)
        if (pt_lds[k]) atomicAdd(&Tt[k], pt_lds[k]);
    if (t == 0)
        for (int k = tid; k < KaP; k += kPtThreads)
            if (pt_lds[cells + k]) atomicAdd(&n[k], pt_lds[cells + k]);
}

// phi(n) = f(n + 1) - f(n), phi(0) = 0: what a cell of n gains in f when a row joins it
__device__ inline double ps_phi(uint32_t n) { return pt_f(n + 1u) - pt_f(n); }

// VI only, after every change of the tables: phi[k] = phi(T[k]) and phim[k] = phi(T[k] - 1) (0 where T[k] = 0: never
// read, a row's own cell holds the row) for every cell, and the same of the sizes into sphi[0 .. KaP), sphi[KaP .. 2 KaP).
__global__ __launch_bounds__(256) void k_ps_phi(const uint32_t* __restrict__ T, const uint32_t* __restrict__ n,
                                                int64_t cells, int KaP, double* __restrict__ phi,
                                                double* __restrict__ phim, double* __restrict__ sphi) {
    const int64_t stride = (int64_t)gridDim.x * kPtThreads;
    for (int64_t k = (int64_t)blockIdx.x * kPtThreads + threadIdx.x; k < cells; k += stride) {
        const uint32_t v = T[k];
        phi[k] = ps_phi(v);
        phim[k] = v ? ps_phi(v - 1u) : 0.0;
    }
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < KaP; k += kPtThreads) {
            const uint32_t v = n[k];
            sphi[k] = ps_phi(v);
            sphi[KaP + k] = v ? ps_phi(v - 1u) : 0.0;
        }
}

// The hot path: the rows [i0, i1) scored against the tables as they stand.  Thread (r, ch) of a workgroup holds row
// i0 + blockIdx.x * rows + r and the slots [8 ch, 8 ch + 8); the nch threads of a row are neighbours.  The draws come
// through LDS in blocks of D tables (uint32 for Binder, the binary64 phi tables for VI): per draw a thread reads its
// row's label b and one run of 8 cells at [b][8 ch ..], lanes with the same label reading the same address.
//   Binder  sum_t T_t[a][z_t,i] in uint32 within a block (D * N < 2^32, the plan's promise), in uint64 across blocks;
//           g_a = S m_a - 2 (sum - S own), int64
//   VI      sum_t phi(U_t,a) in binary64, ascending t; the own slot's cell is T - 1, read from phim in global memory;
//           g_a = S phi(m_a) - 2 sum
// with own = [a = c_i], m_a = n_a - own.  Then the g of a row meet in LDS and its first thread takes the smallest,
// the current slot on a tie, then the lowest: newc[i].  Dynamic LDS: max(D tables, 256 * 8 * 8 bytes).
template <bool VI>
__global__ __launch_bounds__(256) void k_ps_score(const uint8_t* __restrict__ lab, int64_t pitch, int S, int Kc, int Ka,
                                                  int KaP, int nch, int rows, int D, const uint32_t* __restrict__ T,
                                                  const double* __restrict__ phi, const double* __restrict__ phim,
                                                  const double* __restrict__ sphi, const uint32_t* __restrict__ n,
                                                  const int32_t* __restrict__ c, int64_t i0, int64_t i1,
                                                  int32_t* __restrict__ newc) {
    extern __shared__ uint4 ps_lds4[];
    const int tid = threadIdx.x, r = tid / nch, ch = tid - r * nch;
    const int64_t i = i0 + (int64_t)blockIdx.x * rows + r;
    const bool live = r < rows && i < i1;
    const int cells = Kc * KaP;
    const int a0 = live ? c[i] : 0;
    const int j0 = a0 - ch * kPsChunk;  // the own slot's place in this thread's run, if it is in it
    const bool owner = live && j0 >= 0 && j0 < kPsChunk;
    uint64_t acc[kPsChunk];
    double accd[kPsChunk];
#pragma unroll
    for (int j = 0; j < kPsChunk; ++j) { acc[j] = 0; accd[j] = 0.0; }
    for (int t0 = 0; t0 < S; t0 += D) {
        const int nD = S - t0 < D ? S - t0 : D;
        __syncthreads();  // the block before has been read
        if (VI) {
            const double2* __restrict__ src = reinterpret_cast<const double2*>(phi + (size_t)t0 * cells);
            double2* const dst = reinterpret_cast<double2*>(ps_lds4);
            for (int k = tid; k < nD * cells / 2; k += kPtThreads) dst[k] = src[k];
        } else {
            const uint4* __restrict__ src = reinterpret_cast<const uint4*>(T + (size_t)t0 * cells);
            for (int k = tid; k < nD * cells / 4; k += kPtThreads) ps_lds4[k] = src[k];
        }
        __syncthreads();
        if (!live) continue;
        if (VI) {
            const double* const tab = reinterpret_cast<const double*>(ps_lds4);
#pragma unroll 2
            for (int tt = 0; tt < nD; ++tt) {
                const uint32_t b = lab[(size_t)(t0 + tt) * pitch + i];
                const int at = (tt * Kc + (int)b) * KaP + ch * kPsChunk;
                const double2* const p = reinterpret_cast<const double2*>(tab + at);
                double v[kPsChunk];
#pragma unroll
                for (int q = 0; q < kPsChunk / 2; ++q) { const double2 x = p[q]; v[2 * q] = x.x; v[2 * q + 1] = x.y; }
                if (owner) {
                    const double pm = phim[(size_t)(t0 + tt) * cells + ((int)b * KaP + a0)];
#pragma unroll
                    for (int j = 0; j < kPsChunk; ++j) v[j] = j == j0 ? pm : v[j];
                }
#pragma unroll
                for (int j = 0; j < kPsChunk; ++j) accd[j] += v[j];
            }
        } else {
            const uint32_t* const tab = reinterpret_cast<const uint32_t*>(ps_lds4);
            uint32_t a32[kPsChunk];
#pragma unroll
            for (int j = 0; j < kPsChunk; ++j) a32[j] = 0;
#pragma unroll 4
            for (int tt = 0; tt < nD; ++tt) {
                const uint32_t b = lab[(size_t)(t0 + tt) * pitch + i];
                const uint4* const p = reinterpret_cast<const uint4*>(tab + (tt * Kc + (int)b) * KaP + ch * kPsChunk);
                const uint4 x = p[0], y = p[1];
                a32[0] += x.x; a32[1] += x.y; a32[2] += x.z; a32[3] += x.w;
                a32[4] += y.x; a32[5] += y.y; a32[6] += y.z; a32[7] += y.w;
            }
#pragma unroll
            for (int j = 0; j < kPsChunk; ++j) acc[j] += a32[j];
        }
    }
    __syncthreads();  // the last block has been read: the LDS now carries the scores
    if (VI) {
        double* const g = reinterpret_cast<double*>(ps_lds4);
        if (live) {
#pragma unroll
            for (int j = 0; j < kPsChunk; ++j) {
                const int a = ch * kPsChunk + j;
                const double pm = sphi[(a == a0 ? KaP : 0) + a];  // phi(m_a)
                g[tid * kPsChunk + j] = (double)S * pm - 2.0 * accd[j];
            }
        }
    } else {
        int64_t* const g = reinterpret_cast<int64_t*>(ps_lds4);
        if (live) {
#pragma unroll
            for (int j = 0; j < kPsChunk; ++j) {
                const int a = ch * kPsChunk + j;
                const int64_t own = a == a0 ? 1 : 0;
                g[tid * kPsChunk + j] = (int64_t)S * ((int64_t)n[a] - own) - 2 * ((int64_t)acc[j] - (int64_t)S * own);
            }
        }
    }
    __syncthreads();
    if (live && ch == 0) {
        int best = a0;
        if (VI) {
            const double* const g = reinterpret_cast<const double*>(ps_lds4) + (size_t)tid * kPsChunk;
            for (int a = 0; a < Ka; ++a) if (g[a] < g[best]) best = a;
        } else {
            const int64_t* const g = reinterpret_cast<const int64_t*>(ps_lds4) + (size_t)tid * kPsChunk;
            for (int a = 0; a < Ka; ++a) if (g[a] < g[best]) best = a;
        }
        newc[i] = best;
    }
}

// The moves of the rows [i0, i1): thread x of workgroup (x, y) holds a row and the draws [y len, y len + len); a moved
// row takes itself out of its old cell of each of those draws' tables and into the new one (integer adds: exact in
// any order), and in the workgroups of y = 0 it moves between the two sizes and is counted.  c is only read: the
// caller copies newc over it behind this launch.
__global__ __launch_bounds__(256) void k_ps_apply(const uint8_t* __restrict__ lab, int64_t pitch, int S, int Kc, int KaP,
                                                  int len, uint32_t* __restrict__ T, uint32_t* __restrict__ n,
                                                  const int32_t* __restrict__ c, const int32_t* __restrict__ newc,
                                                  int64_t i0, int64_t i1, unsigned long long* __restrict__ moved) {
    const int64_t i = i0 + (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
    if (i >= i1) return;
    const int a0 = c[i], a1 = newc[i];
    if (a0 == a1) return;
    const size_t cells = (size_t)Kc * KaP;
    const int t0 = blockIdx.y * len, t1 = t0 + len < S ? t0 + len : S;
    for (int t = t0; t < t1; ++t) {
        uint32_t* const rowb = T + (size_t)t * cells + (size_t)lab[(size_t)t * pitch + i] * KaP;
        atomicSub(rowb + a0, 1u);
        atomicAdd(rowb + a1, 1u);
    }
    if (blockIdx.y == 0) {
        atomicSub(n + a0, 1u);
        atomicAdd(n + a1, 1u);
        atomicAdd(moved, 1ull);
    }
}

// The totals of the state, draw t per workgroup: A = sum_a n_a^2 and F = sum_a f(n_a) of the candidate, the same of the
// draw's own sizes n_t,b = sum_a T[b][a], Q = sum_ab T^2 and G = sum_ab f(T) -- cell k = a * Kc + b in partial
// k mod 256, ascending, then the tree, as k_pt_pairs adds them.  d2[t] = 2 B(c, z_t), exact; w[t] = F_c + F_t - 2 G,
// N times the VI distance, and exactly 0 where d2 is 0, as k_pt_loss has it.
template <bool VI>
__global__ __launch_bounds__(256) void k_ps_total(const uint32_t* __restrict__ T, const uint32_t* __restrict__ n, int Kc,
                                                  int Ka, int KaP, uint64_t* __restrict__ d2, double* __restrict__ w) {
    __shared__ uint64_t su[kPtThreads];
    __shared__ double sd[kPtThreads];
    const int tid = threadIdx.x, t = blockIdx.x;
    const uint32_t* __restrict__ Tt = T + (size_t)t * Kc * KaP;
    uint64_t ac = 0, at = 0, q = 0;
    double fc = 0.0, ft = 0.0, g = 0.0;
    for (int a = tid; a < Ka; a += kPtThreads) {
        const uint32_t v = n[a];
        ac += (uint64_t)v * v;
        if (VI) fc += pt_f(v);
    }
    for (int b = tid; b < Kc; b += kPtThreads) {
        uint32_t v = 0;
        for (int a = 0; a < Ka; ++a) v += Tt[b * KaP + a];
        at += (uint64_t)v * v;
        if (VI) ft += pt_f(v);
    }
    for (int k = tid; k < Ka * Kc; k += kPtThreads) {
        const int a = k / Kc, b = k - a * Kc;
        const uint32_t v = Tt[b * KaP + a];
        q += (uint64_t)v * v;
        if (VI) g += pt_f(v);
    }
    ac = pt_block_sum(ac, su);
    at = pt_block_sum(at, su);
    q = pt_block_sum(q, su);
    if (VI) {
        fc = pt_block_sum(fc, sd);
        ft = pt_block_sum(ft, sd);
        g = pt_block_sum(g, sd);
    }
    if (tid == 0) {
        const uint64_t d = ac + at - 2 * q;
        d2[t] = d;
        w[t] = (VI && d != 0) ? fc + ft - 2.0 * g : 0.0;
    }
}
// binder2 = sum_t d2[t] and vi_tot = sum_t w[t] (draw t in partial t mod 256, ascending, then the tree), and the count
// of moved rows beside them: the 24 bytes a pass reads back.  One workgroup.
__global__ __launch_bounds__(256) void k_ps_reduce(const uint64_t* __restrict__ d2, const double* __restrict__ w, int S,
                                                   const unsigned long long* __restrict__ moved,
                                                   unsigned long long* __restrict__ res) {
    __shared__ uint64_t su[kPtThreads];
    __shared__ double sd[kPtThreads];
    uint64_t b = 0;
    double v = 0.0;
    for (int t = threadIdx.x; t < S; t += kPtThreads) { b += d2[t]; v += w[t]; }
    b = pt_block_sum(b, su);
    v = pt_block_sum(v, sd);
    if (threadIdx.x == 0) {
        res[0] = b;
        res[1] = (unsigned long long)__double_as_longlong(v);
        res[2] = *moved;
    }
}

// ---- credible ball and row-to-cluster similarity (include/bmm_mcmc.h "credible ball") -----
// Around one centre c: the tables T_t of k_ps_tables and d2[t], w[t] of k_ps_total as the search has them, unchanged.
// k_t, the non-empty labels of draw t, from the row sums of T_t (n_t,b = sum_a T_t[b][a]): one workgroup per draw.
__global__ __launch_bounds__(256) void k_cb_sizes(const uint32_t* __restrict__ T, int Kc, int Ka, int KaP,
                                                  int32_t* __restrict__ k) {
    __shared__ uint32_t su[kPtThreads];
    const int tid = threadIdx.x, t = blockIdx.x;
    const uint32_t* __restrict__ Tt = T + (size_t)t * Kc * KaP;
    uint32_t used = 0;
    for (int b = tid; b < Kc; b += kPtThreads) {
        uint32_t v = 0;
        for (int a = 0; a < Ka; ++a) v += Tt[b * KaP + a];
        used += v ? 1u : 0u;
    }
    used = pt_block_sum(used, su);
    if (tid == 0) k[t] = (int32_t)used;
}

// The hot path: sim[u][a] = sum_t T_t[a][z_t,u] for the M chosen rows.  `lab` is the label block itself (all rows:
// pitch as k_pt_narrow left it, row u is observation u) or the [S][M] block k_pt_gather made of a subset (pitch M).
// Thread (r, ch) of a workgroup holds row blockIdx.x * rows + r and the slots [8 ch, 8 ch + 8); the nch threads of a
// row are neighbours.  The draws come through LDS in blocks of D tables, one flat copy each (the layout is that of
// global memory); per draw a thread reads its row's label b and the run of 8 cells at [b][8 ch ..], 16-byte aligned,
// lanes with the same label reading the same address.  The kernel waits on its label loads more than on the LDS
// (section 29), so a thread issues the loads of kCbAhead draws together.  uint32 sums within a block (D * N < 2^32, the plan's promise),
// uint64 across blocks; the cells past Ka of a run are zero and are not stored.  Integers only, no atomics, nothing
// decided here.  Dynamic LDS: D tables.
constexpr int kCbAhead = 8;  // label loads of a row issued together
__global__ __launch_bounds__(256) void k_cb_member(const uint8_t* __restrict__ lab, int64_t pitch, int S, int Kc, int Ka,
                                                   int KaP, int nch, int rows, int D, const uint32_t* __restrict__ T,
                                                   int64_t M, uint64_t* __restrict__ sim) {
    extern __shared__ uint4 cb_lds4[];
    const int tid = threadIdx.x, r = tid / nch, ch = tid - r * nch;
    const int64_t u = (int64_t)blockIdx.x * rows + r;
    const bool live = r < rows && u < M;
    const int cells = Kc * KaP;
    uint64_t acc[kPsChunk];
#pragma unroll
    for (int j = 0; j < kPsChunk; ++j) acc[j] = 0;
    for (int t0 = 0; t0 < S; t0 += D) {
        const int nD = S - t0 < D ? S - t0 : D;
        __syncthreads();  // the block before has been read
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(T + (size_t)t0 * cells);
        for (int k = tid; k < nD * cells / 4; k += kPtThreads) cb_lds4[k] = src[k];
        __syncthreads();
        if (!live) continue;
        const uint32_t* const tab = reinterpret_cast<const uint32_t*>(cb_lds4);
        uint32_t a32[kPsChunk];
#pragma unroll
        for (int j = 0; j < kPsChunk; ++j) a32[j] = 0;
        const uint8_t* __restrict__ col = lab + (size_t)t0 * pitch + u;
        auto add = [&](int tt, uint32_t b) {
            const uint4* const p = reinterpret_cast<const uint4*>(tab + (tt * Kc + (int)b) * KaP + ch * kPsChunk);
            const uint4 x = p[0], y = p[1];
            a32[0] += x.x; a32[1] += x.y; a32[2] += x.z; a32[3] += x.w;
            a32[4] += y.x; a32[5] += y.y; a32[6] += y.z; a32[7] += y.w;
        };
        int tt = 0;
        for (; tt + kCbAhead <= nD; tt += kCbAhead) {  // the labels of kCbAhead draws in flight before the first is used
            uint32_t b[kCbAhead];
#pragma unroll
            for (int q = 0; q < kCbAhead; ++q) b[q] = col[(size_t)(tt + q) * pitch];
#pragma unroll
            for (int q = 0; q < kCbAhead; ++q) add(tt + q, b[q]);
        }
        for (; tt < nD; ++tt) add(tt, col[(size_t)tt * pitch]);
#pragma unroll
        for (int j = 0; j < kPsChunk; ++j) acc[j] += a32[j];
    }
    if (!live) return;
    uint64_t* const out = sim + (size_t)u * Ka + ch * kPsChunk;
#pragma unroll
    for (int j = 0; j < kPsChunk; ++j)
        if (ch * kPsChunk + j < Ka) out[j] = acc[j];
}

// ---- split-merge moves (include/bmm_mcmc.h "split-merge moves", "split-merge moves of the allocation sampler";
// DESIGN.md sections 15 and 24) ----------------------------------------------------------------------------------------
// One move = k_sm_launch, `scans` + 1 launches of k_sm_scan, k_sm_decide, k_sm_commit, stream-ordered; the host
// never reads anything back.  The two labels of the move are its sides 0 and 1.  One byte per row: its side (0 / 1)
// for a member, 2 + side for the two anchors, kSmOut for every other row.  The statistics of the two sides after
// the launch state (set 0) and after scan t (set t) live in `stat`, a set being {n_0, S_0[P], n_1, S_1[P]} int32:
// scan t reads set t - 1, frozen, and adds into set t, which the host zeroed when it enqueued the move.  The last
// set (scans + 1) is the proposal of a split.  A workgroup holds 256 consecutive rows, one per lane.
// The four kernels are templates over the target, and a flavour's own statements stand behind `if constexpr`:
//   ALLOC = false  the DP chain: a split takes the first empty label, the prior ratio is the CRP's.
//   ALLOC = true   the allocation chain (AsArgs, AsCell: the DP move's with the K cell, p(K) and the Dirichlet
//                  parameter a behind them): the same restricted scans under the allocation sampler's target, the
//                  weights w_c carrying `+ a`.  A split opens label K, the first closed one, and is skipped at
//                  K == maxK; a merge closes label K - 1 after moving it into the label the merge freed, as an
//                  absorb does.  Its draws come from a stream of their own (as_move_draws).
constexpr int kSmThreads = 256;
constexpr int kSmMaxP = 1024;  // the per-feature terms (32 bytes a feature) and the histogram stay below 64 KiB of LDS
constexpr uint8_t kSmOut = 255;
enum : int { SM_SPLIT = 0, SM_MERGE = 1, SM_SKIPPED = 2 };
struct SmCell {
    long long row_i, row_j, members, n_before[2], n_after[2];
    int32_t label_a, label_b, kind, accepted;
    uint32_t salt, pad;
    double log_prior, log_lik, log_q, log_u, log_r;
};
struct SmArgs {
    const uint32_t* Xb;
    int32_t* z;              // the label row the move works on, in place
    int32_t *Nk, *S;         // the chain's statistics, nothing pending
    const double* alpha_ptr;
    uint8_t *side, *side_launch;  // side_launch: a copy of the launch state for the caller, or null
    double* lq;              // [N]: the final scan's log probability per row, 0 outside the members
    int32_t* stat;           // [scans + 2] sets
    SmCell* cell;
    long long* counters;     // proposed / accepted splits, proposed / accepted merges, skipped
    uint32_t sweep, move;
    int scans;
};
struct AsCell {
    SmCell m;
    int32_t k_before, k_after, moved, pad;  // moved: the label a committed merge moved into the gap, or -1
};
struct AsArgs : SmArgs {        // (alpha_ptr is not read; SmArgs::cell points at AsCell::m)
    int32_t* K;                 // the number of open labels
    const double* log_prior_k;  // [maxK]: log p(K = k + 1)
    AsCell* as_cell;
    double a;                   // the Dirichlet parameter per component
};
// A kernel binds `a`, the DP move's arguments, to its parameter itself (const SmArgs& a = g): handed through a function,
// however inlined, the parameter is copied first and its loads lose what the compiler knows of kernel arguments.
template <bool ALLOC>
using SmArgsOf = std::conditional_t<ALLOC, AsArgs, SmArgs>;
__device__ __forceinline__ size_t sm_set(int P) { return (size_t)2 * (P + 1); }

// The rows of one wave into the histogram {n_0, S_0[P], n_1, S_1[P]} of a workgroup: a ballot per feature, one
// LDS atomic per feature, side and wave.  Uniform over the wave.
__device__ __forceinline__ void sm_count_wave(bool counted, int sd, const uint32_t* __restrict__ Xb, int64_t N, int P,
                                              int64_t r, int32_t* hist, int lane) {
    const unsigned long long any = __ballot(counted);
    if (!any) return;
    const unsigned long long m1 = __ballot(counted && sd == 1), m0 = any & ~m1;
    if (lane == 0) {
        if (m0) atomicAdd(&hist[0], (int)__popcll(m0));
        if (m1) atomicAdd(&hist[P + 1], (int)__popcll(m1));
    }
    const int W = (P + 31) >> 5;
    for (int w = 0; w < W; ++w) {
        const uint32_t bits = counted ? Xb[(int64_t)w * N + r] : 0u;
        const int nd = P - w * 32 < 32 ? P - w * 32 : 32;
        for (int t = 0; t < nd; ++t) {
            const unsigned long long b = __ballot(((bits >> t) & 1u) != 0);
            if (lane == t) {
                const int c0 = (int)__popcll(b & m0), c1 = (int)__popcll(b & m1);
                if (c0) atomicAdd(&hist[1 + w * 32 + t], c0);
                if (c1) atomicAdd(&hist[P + 2 + w * 32 + t], c1);
            }
        }
    }
}
__device__ __forceinline__ void sm_flush(const int32_t* hist, int P, int32_t* set, int tid) {
    for (int i = tid; i < 2 * (P + 1); i += kSmThreads) {
        const int32_t v = hist[i];
        if (v != 0) atomicAdd(&set[i], v);
    }
}

// The pair, the two labels and the kind of the move (every workgroup derives them; workgroup 0 records them), then
// the launch state: anchor i on side 0, anchor j on side 1, every other row of the two labels on either side with
// probability 1/2 from its own uniform, whatever its current label.  The label a split opens: the first empty one
// (DP; none: skipped), the K cell's (ALLOC; K == maxK: skipped).
template <bool ALLOC>
__global__ __launch_bounds__(kSmThreads) void k_sm_launch(ChainParams p, SmArgsOf<ALLOC> g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int32_t* const hist = reinterpret_cast<int32_t*>(smem);
    const SmArgs& a = g;
    __shared__ int sh_free, sh_la, sh_lb, sh_kind;
    __shared__ long long sh_i, sh_j;
    __shared__ uint32_t sh_salt;
    const int P = p.P, K = p.K, tid = threadIdx.x, lane = tid & 63;
    const int64_t N = p.N;
    for (int i = tid; i < 2 * (P + 1); i += kSmThreads) hist[i] = 0;
    if constexpr (!ALLOC) {
        if (tid == 0) sh_free = K;
        __syncthreads();
        for (int k = tid; k < K; k += kSmThreads)
            if (a.Nk[k] == 0) atomicMin(&sh_free, k);
        __syncthreads();
    }
    if (tid == 0) {
        int Ka = 0;  // ALLOC: the number of open labels
        if constexpr (ALLOC) Ka = *g.K;
        const SmDraws dr = ALLOC ? as_move_draws(p.seed, a.sweep, a.move, N) : sm_move_draws(p.seed, a.sweep, a.move, N);
        const int la = a.z[dr.i], zj = a.z[dr.j];
        const int kind = la != zj ? SM_MERGE : ((ALLOC ? Ka : sh_free) < K ? SM_SPLIT : SM_SKIPPED);
        const int lb = kind == SM_MERGE ? zj : ALLOC ? (kind == SM_SPLIT ? Ka : la) : sh_free;
        sh_i = dr.i; sh_j = dr.j; sh_la = la; sh_lb = lb; sh_kind = kind; sh_salt = dr.salt;
        if (blockIdx.x == 0) {
            SmCell* c = a.cell;
            if constexpr (ALLOC) c = &g.as_cell->m;  // (the same cell, through the one pointer the flavour follows)
            c->row_i = dr.i; c->row_j = dr.j; c->label_a = la; c->label_b = lb; c->kind = kind; c->salt = dr.salt;
            if constexpr (ALLOC) c->pad = 0;
            c->accepted = 0; c->members = 0;
            c->n_before[0] = a.Nk[la]; c->n_before[1] = kind == SM_MERGE ? a.Nk[lb] : 0;
            c->n_after[0] = c->n_after[1] = 0;
            c->log_u = log_(dr.u);
            c->log_prior = c->log_lik = c->log_q = c->log_r = 0.0;
            if constexpr (ALLOC) { g.as_cell->k_before = Ka; g.as_cell->k_after = Ka; g.as_cell->moved = -1; g.as_cell->pad = 0; }
        }
    }
    __syncthreads();
    const int kind = sh_kind, la = sh_la, lb = sh_lb;
    if (kind == SM_SKIPPED) return;
    const int64_t r = (int64_t)blockIdx.x * kSmThreads + tid;
    int sd = kSmOut;
    if (r < N) {
        const int zr = a.z[r];
        if (zr == la || (kind == SM_MERGE && zr == lb)) {
            if (r == sh_i) sd = 2;
            else if (r == sh_j) sd = 3;
            else sd = sm_member_uniform(sh_salt, (uint64_t)(p.obs0 + r), 0u) < 0.5 ? 0 : 1;
        }
        a.side[r] = (uint8_t)sd;
        if (a.side_launch) a.side_launch[r] = (uint8_t)sd;
    }
    sm_count_wave(sd != kSmOut, sd & 1, a.Xb, N, P, r, hist, lane);
    __syncthreads();
    sm_flush(hist, P, a.stat, tid);
}

// log probabilities of the two sides from diff = log w_0 - log w_1
__device__ __forceinline__ void sm_side_logp(double diff, double& lp0, double& lp1) {
    const bool pos = diff > 0.0;
    const double l = -log_(1.0 + exp_(pos ? -diff : diff));  // the likelier side
    lp0 = pos ? l : l + diff;
    lp1 = pos ? l - diff : l;
}

// Restricted scan t (1 .. scans + 1; the last one is `final`): every member is redrawn between the two sides at
// once against set t - 1 with its own contribution removed exactly, w_c = (n_c - [own]) prod_d (the Beta-Bernoulli
// predictive of side c without the row).  The per-feature terms are differences D[d][own][x] = log term of side 0
// - log term of side 1 (own side "minus self", other side plain), built once per workgroup; a member adds them in
// feature order onto base[own] = log(n_0 - [own = 0]) - log(n_1 - [own = 1]).  The final scan of a split is drawn
// like the others and records the log probability of the side drawn; the final scan of a merge draws nothing and
// records the log probability of the side that is the row's current label.
template <bool ALLOC>
__global__ __launch_bounds__(kSmThreads) void k_sm_scan(ChainParams p, SmArgsOf<ALLOC> g, int t, int final) {
    const SmArgs& a = g;
    extern __shared__ __attribute__((aligned(32))) char smem[];
    const int P = p.P, tid = threadIdx.x, lane = tid & 63;
    const int64_t N = p.N;
    double* const D = reinterpret_cast<double*>(smem);                // [P][2][2]
    int32_t* const hist = reinterpret_cast<int32_t*>(D + 4 * (size_t)P);
    __shared__ double base[2];
    const int kind = a.cell->kind;
    if (kind == SM_SKIPPED) return;
    const bool score_only = final && kind == SM_MERGE;
    const int64_t r = (int64_t)blockIdx.x * kSmThreads + tid;
    const int sd = r < N ? a.side[r] : kSmOut;
    const bool member = sd < 2, counted = sd != kSmOut;
    if (final && r < N && !member) a.lq[r] = 0.0;
    if (!__syncthreads_or(counted)) return;
    const int32_t* const in = a.stat + (size_t)(t - 1) * sm_set(P);
    const int32_t n0 = in[0], n1 = in[P + 1];
    const double bg = p.beta + p.gamma;
    for (int idx = tid; idx < 4 * P; idx += kSmThreads) {
        const int d = idx >> 2, own = (idx >> 1) & 1, x = idx & 1;
        const int32_t s0 = in[1 + d], s1 = in[P + 2 + d];
        const int64_t nm = (own ? n1 : n0) - 1, sm = own ? s1 : s0, np = own ? n0 : n1, sp = own ? s0 : s1;
        const double denm = log_(bg + (double)nm), denp = log_(bg + (double)np);
        // (a member with x = 1 is one of the sm rows, one with x = 0 one of the nm + 1 - sm: the other entries are never read)
        double m = 0.0;
        if (x) { if (sm >= 1) m = term_x1(p.beta, sm - 1, denm); }
        else if (sm <= nm) m = term_x0(p.gamma, nm, sm, denm);
        const double pl = x ? term_x1(p.beta, sp, denp) : term_x0(p.gamma, np, sp, denp);
        D[idx] = own ? pl - m : m - pl;
    }
    for (int i = tid; i < 2 * (P + 1); i += kSmThreads) hist[i] = 0;
    if constexpr (ALLOC) {
        if (tid < 2) base[tid] = log_((double)(n0 - (tid == 0)) + g.a) - log_((double)(n1 - (tid == 1)) + g.a);
    } else {
        if (tid < 2) base[tid] = log_((double)(n0 - (tid == 0))) - log_((double)(n1 - (tid == 1)));
    }
    __syncthreads();
    int ns = sd & 1;
    if (member) {
        const int own = sd;
        double acc = base[own];
        const int W = (P + 31) >> 5;
        for (int w = 0; w < W; ++w) {
            const uint32_t bits = a.Xb[(int64_t)w * N + r];
            const int nd = P - w * 32 < 32 ? P - w * 32 : 32;
            for (int q = 0; q < nd; ++q) {
                const double4 e = *reinterpret_cast<const double4*>(D + 4 * (size_t)(w * 32 + q));  // one address for the wave
                const bool x = (bits >> q) & 1u;
                acc = acc + (own ? (x ? e.w : e.z) : (x ? e.y : e.x));
            }
        }
        double lp0, lp1;
        sm_side_logp(acc, lp0, lp1);
        if (score_only) {
            a.lq[r] = a.z[r] == a.cell->label_a ? lp0 : lp1;
        } else {
            const double u = sm_member_uniform(a.cell->salt, (uint64_t)(p.obs0 + r), (uint32_t)t);
            ns = u < exp_(lp0) ? 0 : 1;
            a.side[r] = (uint8_t)ns;
            if (final) a.lq[r] = ns ? lp1 : lp0;
        }
    }
    if (score_only) return;
    sm_count_wave(counted, ns, a.Xb, N, P, r, hist, lane);
    __syncthreads();
    sm_flush(hist, P, a.stat + (size_t)t * sm_set(P), tid);
}

// One workgroup: log q in an order fixed by N (1024 partial sums, row i in partial i mod 1024, ascending, then a
// binary tree, as k_loo_reduce), the marginal-likelihood ratio the same way over the features, the prior ratio (the
// CRP's; ALLOC: the spec's as_log_prior, and with it what the move does to K), the decision and the counters.
__device__ __forceinline__ double sm_pair(double beta, double gamma, int64_t n, int64_t s) {
    return lgamma_(beta + (double)s) + lgamma_((gamma + (double)n) - (double)s);
}
template <bool ALLOC>
__global__ __launch_bounds__(1024) void k_sm_decide(ChainParams p, SmArgsOf<ALLOC> g) {
    __shared__ double sh[2][1024];
    const SmArgs& a = g;
    const int t = threadIdx.x, P = p.P;
    SmCell* c = a.cell;
    if constexpr (ALLOC) c = &g.as_cell->m;
    const int kind = c->kind;
    if (kind == SM_SKIPPED) {
        if (t == 0) a.counters[4] += 1;
        return;
    }
    const int la = c->label_a, lb = c->label_b;
    const int32_t* const fin = a.stat + (size_t)(a.scans + 1) * sm_set(P);
    const bool split = kind == SM_SPLIT;
    const int64_t no0 = a.Nk[la], no1 = split ? 0 : a.Nk[lb];
    const int64_t nn0 = split ? fin[0] : no0 + no1, nn1 = split ? fin[P + 1] : 0;
    double lq = 0.0, ll = 0.0;
    for (int64_t i = t; i < p.N; i += 1024) lq = lq + a.lq[i];
    for (int d = t; d < P; d += 1024) {
        const int64_t so0 = a.S[(size_t)la * P + d], so1 = split ? 0 : a.S[(size_t)lb * P + d];
        const int64_t sn0 = split ? fin[1 + d] : so0 + so1, sn1 = split ? fin[P + 2 + d] : 0;
        double term;
        if (split) term = (sm_pair(p.beta, p.gamma, nn0, sn0) + sm_pair(p.beta, p.gamma, nn1, sn1)) - sm_pair(p.beta, p.gamma, no0, so0);
        else term = sm_pair(p.beta, p.gamma, nn0, sn0) - (sm_pair(p.beta, p.gamma, no0, so0) + sm_pair(p.beta, p.gamma, no1, so1));
        ll = ll + term;
    }
    sh[0][t] = lq; sh[1][t] = ll;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (t < s) { sh[0][t] = sh[0][t] + sh[0][t + s]; sh[1][t] = sh[1][t] + sh[1][t + s]; }
        __syncthreads();
    }
    if (t != 0) return;
    const double bg = p.beta + p.gamma;
    double la_ = 0.0;  // DP: log alpha
    if constexpr (!ALLOC) la_ = log_(*a.alpha_ptr);
    const double c0 = (lgamma_(bg) - lgamma_(p.beta)) - lgamma_(p.gamma);
    const double log_q = sh[0][0];
    double cst, log_prior;
    if (split) {
        cst = ((c0 - lgamma_(bg + (double)nn0)) - lgamma_(bg + (double)nn1)) + lgamma_(bg + (double)no0);
        if constexpr (!ALLOC) log_prior = ((la_ + lgamma_((double)nn0)) + lgamma_((double)nn1)) - lgamma_((double)no0);
    } else {
        cst = ((lgamma_(bg + (double)no0) + lgamma_(bg + (double)no1)) - lgamma_(bg + (double)nn0)) - c0;
        if constexpr (!ALLOC) log_prior = ((lgamma_((double)nn0) - lgamma_((double)no0)) - lgamma_((double)no1)) - la_;
    }
    int K = 0;  // ALLOC: the number of open labels before the move
    if constexpr (ALLOC) {
        K = g.as_cell->k_before;
        log_prior = split ? as_log_prior(K, (double)p.Ntot, g.a, g.log_prior_k, no0, nn0, nn1, true)
                          : as_log_prior(K, (double)p.Ntot, g.a, g.log_prior_k, nn0, no0, no1, false);
    }
    const double log_lik = sh[1][0] + (double)P * cst;
    const double log_r = split ? (log_prior + log_lik) - log_q : (log_prior + log_lik) + log_q;
    const int acc = c->log_u < log_r ? 1 : 0;
    c->log_prior = log_prior; c->log_lik = log_lik; c->log_q = log_q; c->log_r = log_r; c->accepted = acc;
    c->n_after[0] = nn0; c->n_after[1] = nn1;
    const int32_t* const first = a.stat;
    c->members = (long long)first[0] + first[P + 1] - 2;
    if constexpr (ALLOC) {
        g.as_cell->k_after = acc ? (split ? K + 1 : K - 1) : K;
        g.as_cell->moved = acc && !split && lb != K - 1 ? K - 1 : -1;
    }
    a.counters[split ? 0 : 2] += 1;
    if (acc) a.counters[split ? 1 : 3] += 1;
}

// An accepted move: the labels and the exact integer statistics of the labels touched.  A rejected or skipped one:
// nothing, so the host never waits inside a move.  Every workgroup relabels its own rows from the record alone: a
// split gives the rows of side 1 label lb; a DP merge gives the rows of the higher label the lower one; an ALLOC merge
// gives the rows of lb label la and then, as an absorb, the rows of label K - 1 the freed label lb (with la == K - 1
// the merged component ends up under lb).  Workgroup 0 writes the statistics and, ALLOC, the K cell, which no other
// workgroup reads.
template <bool ALLOC>
__global__ __launch_bounds__(kSmThreads) void k_sm_commit(ChainParams p, SmArgsOf<ALLOC> g) {
    const SmArgs& a = g;
    const SmCell* c = a.cell;
    if constexpr (ALLOC) c = &g.as_cell->m;
    if (!c->accepted) return;
    const int P = p.P, tid = threadIdx.x, la = c->label_a, lb = c->label_b;
    int last = 0;  // ALLOC: label K - 1, which a merge moves into the gap
    if constexpr (ALLOC) last = g.as_cell->k_before - 1;
    const bool split = c->kind == SM_SPLIT;
    const int lo = la < lb ? la : lb, hi = la < lb ? lb : la;
    const int64_t r = (int64_t)blockIdx.x * kSmThreads + tid;
    if (r < p.N) {
        if (split) {
            const int sd = a.side[r];
            if (sd == 1 || sd == 3) a.z[r] = lb;
        } else if constexpr (ALLOC) {
            const int zr = a.z[r];
            if (zr == lb) a.z[r] = (la == last && lb != last) ? lb : la;
            else if (zr == last && lb != last) a.z[r] = lb;
        } else if (a.z[r] == hi) {
            a.z[r] = lo;
        }
    }
    if (blockIdx.x != 0) return;
    const int32_t* const fin = a.stat + (size_t)(a.scans + 1) * sm_set(P);
    for (int idx = tid; idx <= P; idx += kSmThreads) {
        int32_t* const A = idx == 0 ? a.Nk + la : a.S + (size_t)la * P + (idx - 1);
        int32_t* const B = idx == 0 ? a.Nk + lb : a.S + (size_t)lb * P + (idx - 1);
        if (split) {
            *A = fin[idx]; *B = fin[P + 1 + idx];
        } else if constexpr (ALLOC) {  // in this order: la may be the last label
            int32_t* const Z = idx == 0 ? a.Nk + last : a.S + (size_t)last * P + (idx - 1);
            const int32_t s = *A + *B;
            *A = s; *B = 0;
            if (lb != last) { *B = *Z; *Z = 0; }
        } else {
            const int32_t s = *A + *B;
            *(la < lb ? A : B) = s;
            *(la < lb ? B : A) = 0;
        }
    }
    if constexpr (ALLOC) {
        if (tid == 0) *g.K = g.as_cell->k_after;
    }
}

// ---- feature selection for the counting samplers (include/bmm_mcmc.h "feature selection") ----
// The gamma-step behind a sweep end: every inclusion indicator redrawn from its exact conditional given the folded
// counts.  A workgroup owns the 32 features of one mask word, one wave per feature (16 waves, two rounds); lanes
// stride over the clusters in ascending order, an empty cluster is skipped, and the 64 partial sums are added by a
// butterfly, so the order of the sum is fixed by K alone.  lgamma_(beta + gamma + N_k) is the same for every
// feature: once per workgroup, in LDS.  Lane 0 of a wave decides, records and folds; the word is put together in LDS
// and written once with a plain store.  Nothing is atomic in global memory: one seed gives the same bits twice.
// lgamma_ and the logistic are called, not inlined, in k_fs_gamma: inlined at their five places their binary64
// constants crowd the scalar registers (28 of them spilled to vector lanes); called, the kernel spills nothing and
// still needs no stack.  Same arithmetic, same bits.
__device__ __attribute__((noinline)) double fs_lgamma(double x) { return lgamma_(x); }
__device__ __attribute__((noinline)) double fs_prob(double lam) { return div_(1.0, 1.0 + exp_(-lam)); }
__device__ __forceinline__ double fs_pair(double beta, double gamma, int64_t n, int64_t s) {  // sm_pair, called
    return fs_lgamma(beta + (double)s) + fs_lgamma((gamma + (double)n) - (double)s);
}
constexpr int kFsThreads = 1024;
struct FsArgs {
    const int32_t *Nk, *S;   // the chain's statistics, nothing pending (k_count_sweep_end folded them)
    uint32_t* mask;          // [ceil(P / 32)] words: the indicators the next sweep's tables read
    uint8_t* gamma;          // [P] the same, a byte each
    uint8_t* gamma_row;      // or null: [P], this sweep's row of a trace
    double* rec;             // [3][P]: Lambda, p, u of this step
    uint32_t* incl_count;    // [P] accumulators over the folded steps: the draws ...
    double* incl_prob;       // ... and their probabilities (one add per step: a fixed order)
    double logit_rho;        // log rho - log(1 - rho)
    uint32_t sweep;
    int fold;
};
__global__ __launch_bounds__(kFsThreads) void k_fs_gamma(ChainParams p, FsArgs a) {
    // lgamma_ of: beta + gamma + N_k (k < K; 0 for an empty cluster), beta + gamma + N, beta, gamma, beta + gamma
    __shared__ double lg[kMaxCatsAny + 4];
    __shared__ unsigned sh_word;
    const int P = p.P, K = p.K, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double bg = p.beta + p.gamma;
    for (int i = tid; i < K + 4; i += kFsThreads) {
        const int32_t n = i < K ? a.Nk[i] : 1;
        const double arg = i < K ? bg + (double)n : (i == K ? bg + (double)p.N : (i == K + 1 ? p.beta : (i == K + 2 ? p.gamma : bg)));
        lg[i] = n > 0 ? fs_lgamma(arg) : 0.0;
    }
    if (tid == 0) sh_word = 0u;
    __syncthreads();
    const double lb0 = (lg[K + 1] + lg[K + 2]) - lg[K + 3];  // lB(beta, gamma)
    for (int r = 0; r < 2; ++r) {
        const int bit = r * 16 + wave, d = blockIdx.x * 32 + bit;
        if (d >= P) break;  // uniform over the wave
        int64_t T = 0;  // (an empty cluster's count is 0)
        for (int k = lane; k < K; k += 64) T += a.S[(size_t)k * P + d];
        for (int o = 32; o > 0; o >>= 1) T += __shfl_xor(T, o);
        // lane l walks the clusters l, l + 64, ... in ascending order, an empty one skipped (not added as a zero); the
        // all-rows term of the noise model is entry K of the same walk, subtracted
        double acc = 0.0;
        for (int k = lane; k <= K; k += 64) {
            const int64_t n = k < K ? (int64_t)a.Nk[k] : p.N;
            if (n <= 0) continue;
            const int64_t s = k < K ? (int64_t)a.S[(size_t)k * P + d] : T;
            const double t = (fs_pair(p.beta, p.gamma, n, s) - lg[k]) - lb0;
            acc = k < K ? acc + t : acc - t;
        }
        for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
        if (lane != 0) continue;
        const double lam = a.logit_rho + acc;
        const double pr = fs_prob(lam);
        const double u = fs_uniform(p.seed, (uint32_t)d, a.sweep);
        const unsigned g = u < pr ? 1u : 0u;
        if (g) atomicOr(&sh_word, 1u << bit);
        a.gamma[d] = (uint8_t)g;
        if (a.gamma_row) a.gamma_row[d] = (uint8_t)g;
        a.rec[d] = lam; a.rec[(size_t)P + d] = pr; a.rec[(size_t)2 * P + d] = u;
        if (a.fold) {
            a.incl_count[d] += g;
            a.incl_prob[d] = a.incl_prob[d] + pr;
        }
    }
    __syncthreads();
    if (tid == 0) a.mask[blockIdx.x] = sh_word;
}

// ---- k-modes++ initial allocation (include/bmm_mcmc.h "initial allocation") ---------------
// Seeding: k_init_dist(0), then k_init_pick(j), k_init_dist(j) for j = 1 .. Kc - 1; seating: k_init_assign(0), which
// gives every row its nearest seeded centre (the strict minimum of the seeding, so the labels it writes are `near`)
// and counts them; refinement round r = 1 .. iters: k_init_modes(r), k_init_assign(r).  All stream-ordered, nothing is
// read back in between: the cell's `stop` (fewer distinct rows than centres) and `done` (a round changed no label)
// make the launches that are left over return at once.  Integers throughout; the one product per centre is
// init_uniform * (double)T.  A workgroup holds 256 consecutive rows, one per lane.
constexpr int kInitThreads = 256;
constexpr int kInitMaxCentreBytes = 65536;  // Kc * W * 4 above this is refused (the centres live in LDS)
// centres and the count histogram of k_init_assign in dynamic LDS up to here (of the 160 KiB of a gfx950 workgroup; the
// kernel has a few bytes of static LDS besides, and its launches set the attribute that allows the size); above it
// the labels are counted by k_count_labels_generic behind the launch
constexpr size_t kInitLdsBudget = 131072;
struct InitCell {
    int32_t k_eff, stop, done, rounds_run;
    long long changed[2], cost[2];  // of the assign launch of round r in slot r & 1 (the seating counts as round 0)
};
struct InitArgs {
    const uint32_t* Xb;
    int32_t *dist, *lab;   // [N]: distance to the nearest centre so far; the labels (0-based)
    int32_t* blocksum;     // [ceil(N / 256)]: sum of dist over a workgroup's rows (at most 256 * (P + 1) < 2^31)
    uint32_t* centres;     // [Kc][W], the last word masked to its valid bits
    long long* rows;       // [Kc]: the picked rows
    int32_t *Nk, *S;       // [Kc], [Kc][P]: counts of the labels of the last assign launch
    InitCell* cell;
    int Kc;
};

// inclusive prefix sum over the workgroup (wave scan, then the wave totals through LDS); shw: one slot per wave
__device__ __forceinline__ long long init_block_scan(long long v, long long* shw, long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    long long x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const long long y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    __syncthreads();  // shw may still be read from an earlier call
    if (lane == 63) shw[wave] = x;
    __syncthreads();
    long long before = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        const long long s = shw[w];
        tot += s;
        if (w < wave) before += s;
    }
    total = tot;
    return x + before;
}

// Centre m against every row: Hamming distance by XOR and popcount, strict minimum into dist / lab (ties keep the
// lower label), and the workgroup's sum of dist.  Centre 0 is row r_0, which every workgroup derives from the draw
// itself; later centres were written by k_init_pick.  The centre's words are read through one address per wave.
__global__ __launch_bounds__(kInitThreads) void k_init_dist(ChainParams p, InitArgs a, int m) {
    __shared__ int sh_sum;
    InitCell* const cell = a.cell;
    if (m > 0 && cell->stop) return;
    const int tid = threadIdx.x, P = p.P, W = (P + 31) >> 5;
    const int64_t N = p.N;
    const uint32_t* src = a.centres + (size_t)m * W;
    int64_t stride = 1;
    if (m == 0) {
        int64_t r0 = (int64_t)(init_uniform(p.seed, 0u) * (double)N);
        r0 = r0 > N - 1 ? N - 1 : r0;
        src = a.Xb + r0;
        stride = N;
        if (blockIdx.x == 0) {
            for (int w = tid; w < W; w += kInitThreads) a.centres[w] = src[(int64_t)w * N] & init_word_mask(P, w);
            if (tid == 0) { a.rows[0] = r0; cell->k_eff = a.Kc; }
        }
    }
    if (tid == 0) sh_sum = 0;
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * kInitThreads + tid;
    int d = 0;
    if (r < N) {
        int h = 0;
        for (int w = 0; w < W; ++w) h += __popc((a.Xb[(int64_t)w * N + r] ^ src[(int64_t)w * stride]) & init_word_mask(P, w));
        d = m == 0 ? P + 1 : a.dist[r];
        if (h < d) { d = h; a.dist[r] = h; a.lab[r] = m; }
    }
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
    if ((tid & 63) == 0) atomicAdd(&sh_sum, d);
    __syncthreads();
    if (tid == 0) a.blocksum[blockIdx.x] = sh_sum;
}

// One workgroup: T = sum of dist, t = min(T - 1, (int64)(u_j * (double)T)), the smallest row whose inclusive prefix
// sum of dist exceeds t -- first the workgroup of k_init_dist that holds it (1024 block sums a trip, the running total
// carried), then the row among that workgroup's 256 -- and that row's words as centre j.  T == 0: every row coincides
// with a centre; k_eff = j and the seeding stops.
__global__ __launch_bounds__(1024) void k_init_pick(ChainParams p, InitArgs a, int j, int nblocks) {
    __shared__ long long shw[16];
    __shared__ long long sh_off, sh_row;
    __shared__ int sh_blk;
    InitCell* const cell = a.cell;
    if (cell->stop) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = p.P, W = (P + 31) >> 5;
    const int64_t N = p.N;
    long long part = 0;
    for (int b = tid; b < nblocks; b += 1024) part += a.blocksum[b];
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 0) shw[wave] = part;
    if (tid == 0) { sh_blk = -1; sh_row = -1; }
    __syncthreads();
    long long T = 0;
    for (int w = 0; w < 16; ++w) T += shw[w];
    if (T == 0) {
        if (tid == 0) { cell->k_eff = j; cell->stop = 1; }
        return;
    }
    long long t = (long long)(init_uniform(p.seed, (uint32_t)j) * (double)T);
    t = t > T - 1 ? T - 1 : t;
    long long carry = 0;
    for (int base = 0; base < nblocks; base += 1024) {
        const int b = base + tid;
        const long long v = b < nblocks ? a.blocksum[b] : 0;
        long long total;
        const long long incl = carry + init_block_scan(v, shw, total);
        if (incl > t && incl - v <= t) { sh_blk = b; sh_off = t - (incl - v); }
        carry += total;
        __syncthreads();
        if (sh_blk >= 0) break;
    }
    const int blk = sh_blk;
    if (blk < 0) return;  // (t < T: never)
    const long long off = sh_off;
    const int64_t r = (int64_t)blk * kInitThreads + tid;
    const long long v = tid < kInitThreads && r < N ? a.dist[r] : 0;
    long long total;
    const long long incl = init_block_scan(v, shw, total);
    if (incl > off && incl - v <= off) sh_row = r;
    __syncthreads();
    const int64_t row = sh_row;
    if (row < 0) return;
    for (int w = tid; w < W; w += 1024) a.centres[(size_t)j * W + w] = a.Xb[(int64_t)w * N + row] & init_word_mask(P, w);
    if (tid == 0) a.rows[j] = row;
}

// The labelled rows of one wave into the histogram {Nk, S[P]} per label of a workgroup, as sm_count_wave counts its
// two sides: one ballot per feature, kept by the lane of that feature; then, per label present in the wave, one
// ballot for its rows and one LDS atomic per feature with a count.  Uniform over the wave.
__device__ __forceinline__ void init_count_wave(bool valid, int label, const uint32_t* __restrict__ Xb, int64_t N, int P,
                                                int64_t r, int32_t* hist, int lane) {
    const unsigned long long any = __ballot(valid);
    if (!any) return;
    const int W = (P + 31) >> 5;
    for (int w = 0; w < W; ++w) {
        const uint32_t bits = valid ? Xb[(int64_t)w * N + r] : 0u;
        const int nd = P - w * 32 < 32 ? P - w * 32 : 32;
        unsigned long long mine = 0;  // lane t: the rows of the wave with feature w * 32 + t set
        for (int t = 0; t < nd; ++t) {
            const unsigned long long b = __ballot(((bits >> t) & 1u) != 0);
            if (lane == t) mine = b;
        }
        unsigned long long left = any;
        while (left) {
            const int k = __shfl(label, __builtin_ctzll(left));
            const unsigned long long mk = __ballot(valid && label == k);
            left &= ~mk;
            int32_t* const h = hist + (size_t)k * (P + 1);
            if (w == 0 && lane == 0) atomicAdd(&h[0], (int)__popcll(mk));
            if (lane < nd) {
                const int cnt = (int)__popcll(mine & mk);
                if (cnt) atomicAdd(&h[1 + w * 32 + lane], cnt);
            }
        }
    }
}

// Every row takes the nearest of the k_eff centres (LDS), ties to the lowest label; `changed` against the label it had
// (not counted by the seating, round 0), the cost (the sum of the distances to the centres taken), and with COUNT the
// new labels' Nk and S, flushed once per workgroup.  Rows of up to four words keep them in registers.
template <bool COUNT>
__global__ __launch_bounds__(kInitThreads) void k_init_assign(ChainParams p, InitArgs a, int round) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int sh_changed, sh_cost;
    InitCell* const cell = a.cell;
    if (cell->done) return;
    const int tid = threadIdx.x, lane = tid & 63, P = p.P, W = (P + 31) >> 5, ke = cell->k_eff;
    const int64_t N = p.N;
    uint32_t* const cen = reinterpret_cast<uint32_t*>(smem);
    int32_t* const hist = reinterpret_cast<int32_t*>(cen + (size_t)ke * W);
    for (int i = tid; i < ke * W; i += kInitThreads) cen[i] = a.centres[i];
    if (COUNT) for (int i = tid; i < ke * (P + 1); i += kInitThreads) hist[i] = 0;
    if (tid == 0) { sh_changed = 0; sh_cost = 0; }
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * kInitThreads + tid;
    const bool valid = r < N;
    int best = 0, bd = 0;
    if (valid) {
        bd = 0x7fffffff;
        if (W <= 4) {
            uint32_t x[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) x[w] = w < W ? a.Xb[(int64_t)w * N + r] & init_word_mask(P, w) : 0u;
            for (int k = 0; k < ke; ++k) {
                int h = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) h += w < W ? __popc(x[w] ^ cen[k * W + w]) : 0;
                if (h < bd) { bd = h; best = k; }
            }
        } else {
            for (int k = 0; k < ke; ++k) {
                int h = 0;
                for (int w = 0; w < W; ++w) h += __popc((a.Xb[(int64_t)w * N + r] & init_word_mask(P, w)) ^ cen[(size_t)k * W + w]);
                if (h < bd) { bd = h; best = k; }
            }
        }
    }
    const bool moved = valid && round > 0 && a.lab[r] != best;
    if (valid) a.lab[r] = best;
    const unsigned long long mv = __ballot(moved);
    int cs = bd;
    for (int o = 32; o > 0; o >>= 1) cs += __shfl_xor(cs, o);
    if (lane == 0) {
        if (mv) atomicAdd(&sh_changed, (int)__popcll(mv));
        if (cs) atomicAdd(&sh_cost, cs);
    }
    if (COUNT) init_count_wave(valid, best, a.Xb, N, P, r, hist, lane);
    __syncthreads();
    if (COUNT)
        for (int i = tid; i < ke * (P + 1); i += kInitThreads) {
            const int32_t v = hist[i];
            if (v == 0) continue;
            const int k = i / (P + 1), d = i - k * (P + 1);
            atomicAdd(d == 0 ? &a.Nk[k] : &a.S[(size_t)k * P + d - 1], v);
        }
    if (tid == 0) {
        if (sh_changed) atomicAdd(reinterpret_cast<unsigned long long*>(&cell->changed[round & 1]), (unsigned long long)sh_changed);
        if (sh_cost) atomicAdd(reinterpret_cast<unsigned long long*>(&cell->cost[round & 1]), (unsigned long long)sh_cost);
    }
}

// Round `round` >= 1, one workgroup per centre: a round after one that changed no label ends the refinement (`done`).
// Otherwise bit d of centre k becomes 1 if 2 S > Nk, 0 if 2 S < Nk and keeps its value on a tie or when Nk == 0; the
// counts it has read are cleared for the assign launch that follows, and so are that launch's two totals.
__global__ __launch_bounds__(kInitThreads) void k_init_modes(ChainParams p, InitArgs a, int round) {
    InitCell* const cell = a.cell;
    if (cell->done) return;
    const int tid = threadIdx.x, P = p.P, W = (P + 31) >> 5, k = blockIdx.x;
    if (round > 1 && cell->changed[(round - 1) & 1] == 0) {
        if (k == 0 && tid == 0) cell->done = 1;
        return;
    }
    if (k == 0 && tid == 0) { cell->rounds_run = round; cell->changed[round & 1] = 0; cell->cost[round & 1] = 0; }
    if (k >= cell->k_eff) return;
    const int32_t nk = a.Nk[k];
    __syncthreads();
    for (int w = tid; w < W; w += kInitThreads) {
        uint32_t c = a.centres[(size_t)k * W + w];
        const int nd = P - w * 32 < 32 ? P - w * 32 : 32;
        for (int t = 0; t < nd; ++t) {
            int32_t* const sp = a.S + (size_t)k * P + w * 32 + t;
            const int64_t s2 = 2 * (int64_t)*sp;
            if (s2 > nk) c |= 1u << t;
            else if (s2 < nk) c &= ~(1u << t);
            *sp = 0;
        }
        a.centres[(size_t)k * W + w] = c;
    }
    if (tid == 0) a.Nk[k] = 0;
}

// ---- the allocation sampler: unknown K for the finite chain (include/bmm_mcmc.h "allocation sampler")
// (its table build is k_count_tables<TAB_ALLOC>)

// ---- parallel tempering (include/bmm_mcmc.h "parallel tempering") --------------------------
// (a rung's table build is k_count_tables<TAB_TEMPER>)
// The exchange of a replica ladder: R <= kTemperMaxR chains ("rungs") over the same data at inverse temperatures
// 1 = b_0 > b_1 > ...; rung r's row of k_log_joint_finish holds L_r = log p(x | z_r) of its current state.
// k_temper_decide: one wave; lane j takes pair r = 2 j + (t mod 2), the pairs of exchange point t (they are disjoint,
// so all are decided at once): d, u and the decision by the rules of bmm_spec.h, the record, the counters and the
// walker ids, all plain stores by the deciding lane; the pairs that are not proposed at t get an empty record from
// the lane that would own them at t + 1.  `lik_row` (or null) receives every rung's L as it stands after the
// exchange.  k_temper_exchange: one y-slice of the grid per proposed pair, stream-ordered behind the lane that
// wrote accept[r], so a slice whose pair was rejected returns at once and no block reads a cell another is writing;
// an accepted pair swaps the two chains' current label rows, folded statistics, every replica of the pending deltas
// as they stand (no fold) and the concentration.  States move, temperatures stay.  Nothing is atomic in global memory.
constexpr int kTemperMaxR = 8;
constexpr int kTemperThreads = 256;
struct TemperStep {
    double d, u;
    int32_t proposed, accepted;
};
struct TemperRung {
    const double* lj_out;  // the rung's log joint row: [0] = log_lik
    int32_t* z;            // its current label row [N]
    int32_t *Nk, *S;       // [K], [K * P]
    int32_t *dNk, *dS;     // kDeltaReps replicas of each
    double* alpha;
    double* alpha_row;     // or null: the cell of the alpha trace that holds this state's concentration
    double b;
};
struct TemperArgs {
    TemperRung rung[kTemperMaxR];
    int R;
    uint32_t t;
    unsigned long long seed;
    int32_t* accept;       // [R - 1]
    int32_t* walker;       // [R]
    long long* counters;   // proposed [R - 1], then accepted [R - 1]
    TemperStep* rec;       // [R - 1]
    double* lik_row;       // or null: [R]
    int64_t N;
    int K, P;
};
__global__ __launch_bounds__(64) void k_temper_decide(TemperArgs a) {
    const int lane = threadIdx.x, par = (int)(a.t & 1u);
    const int r = 2 * lane + par, idle = 2 * lane + 1 - par;  // this lane's pair at t, and the one it leaves alone
    if (idle + 1 < a.R) {
        TemperStep e;
        e.d = qnan(); e.u = qnan(); e.proposed = 0; e.accepted = 0;
        a.rec[idle] = e;
        a.accept[idle] = 0;
    }
    if (r + 1 < a.R) {
        const double Lr = a.rung[r].lj_out[0], Lr1 = a.rung[r + 1].lj_out[0];
        TemperStep e;
        e.d = temper_log_ratio(a.rung[r].b, a.rung[r + 1].b, Lr, Lr1);
        e.u = temper_uniform(a.seed, (uint32_t)r, a.t);
        const bool acc = temper_accepts(e.d, e.u);
        e.proposed = 1; e.accepted = acc ? 1 : 0;
        a.rec[r] = e;
        a.accept[r] = e.accepted;
        a.counters[r] += 1;
        if (acc) {
            a.counters[a.R - 1 + r] += 1;
            const int32_t w = a.walker[r];
            a.walker[r] = a.walker[r + 1];
            a.walker[r + 1] = w;
        }
        if (a.lik_row) { a.lik_row[r] = acc ? Lr1 : Lr; a.lik_row[r + 1] = acc ? Lr : Lr1; }
    }
    // a rung outside every pair of this point: the first at an odd point, the last when the pairs end before it
    if (a.lik_row && lane < a.R) {
        const int first = lane - ((lane - par) & 1);  // the pair that would hold rung `lane`
        if (lane < par || first + 1 >= a.R) a.lik_row[lane] = a.rung[lane].lj_out[0];
    }
}
// n int32 of x and y exchanged by the workgroups of one grid slice: 16 bytes per access where both are so aligned
__device__ __forceinline__ void temper_swap(int32_t* __restrict__ x, int32_t* __restrict__ y, int64_t n) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;
    if ((((uintptr_t)x | (uintptr_t)y) & 15u) == 0) {
        int4* const x4 = reinterpret_cast<int4*>(x);
        int4* const y4 = reinterpret_cast<int4*>(y);
        const int64_t n4 = n >> 2;
        for (int64_t i = tid; i < n4; i += nth) {
            const int4 u = x4[i], v = y4[i];
            x4[i] = v; y4[i] = u;
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += nth) {
        const int32_t u = x[i], v = y[i];
        x[i] = v; y[i] = u;
    }
}
__global__ __launch_bounds__(kTemperThreads) void k_temper_exchange(TemperArgs a) {
    const int r = 2 * (int)blockIdx.y + (int)(a.t & 1u);
    if (r + 1 >= a.R || !a.accept[r]) return;
    const TemperRung& x = a.rung[r];
    const TemperRung& y = a.rung[r + 1];
    const int64_t K = a.K, KP = (int64_t)a.K * a.P;
    temper_swap(x.z, y.z, a.N);
    temper_swap(x.Nk, y.Nk, K);
    temper_swap(x.S, y.S, KP);
    temper_swap(x.dNk, y.dNk, K * kDeltaReps);
    temper_swap(x.dS, y.dS, KP * kDeltaReps);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double ax = *x.alpha, ay = *y.alpha;
        *x.alpha = ay; *y.alpha = ax;
        if (x.alpha_row) *x.alpha_row = ay;
        if (y.alpha_row) *y.alpha_row = ax;
    }
}

// The eject / absorb move of Nobile & Fearnside (2007), p_E integrated out of the proposal density: k_ea_launch,
// k_ea_decide, k_ea_commit, stream-ordered; the host never reads anything back.  One byte per row.  An eject of label
// j1 into the appended label j2 = K: 0 a row of j1 that stays, 1 one that moves.  An absorb of j2 into j1: 0 a row of
// j1, 1 a row of j2 (it takes j1), 2 a row of label K - 1 when j2 != K - 1 (it takes the freed label j2, after the
// rows of j2 have moved: with j1 == K - 1 the rows of j1 carry 2 and the merged component ends up under j2).  kEaOut
// every other row.  `stat` = {n2', S2'[P]}, the statistics of the rows an eject moves, zeroed by the host.
constexpr int kEaThreads = 256;
constexpr int kEaMaxP = 1024;
constexpr uint8_t kEaOut = 255;
struct EaCell {
    long long members, n_before[2], n_after[2];
    int32_t kind, j1, j2, accepted, k_before, k_after;
    uint32_t salt, pad;
    unsigned long long pe_bits;
    double log_prior, log_lik, log_q, log_move, log_u, log_r;
};
struct EaArgs {
    const uint32_t* Xb;
    int32_t* z;               // the label row the move works on, in place
    int32_t *Nk, *S;          // the chain's statistics, nothing pending
    int32_t* K;               // the number of open labels
    const double* log_prior_k;  // [maxK]: log p(K = k + 1)
    uint8_t* side;
    int32_t* stat;
    EaCell* cell;
    long long* counters;      // proposed / accepted ejects, proposed / accepted absorbs
    double a, eject_a;
    uint32_t sweep, move;
};

// Every workgroup derives the move; workgroup 0 records it.  Then the side bytes and, for an eject, the statistics of
// the rows that move: a ballot per feature, one LDS atomic per feature and wave, one flush per workgroup.
__global__ __launch_bounds__(kEaThreads) void k_ea_launch(ChainParams p, EaArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int32_t* const hist = reinterpret_cast<int32_t*>(smem);  // [P + 1]
    __shared__ int sh_kind, sh_j1, sh_j2, sh_K;
    __shared__ uint32_t sh_salt;
    __shared__ double sh_pe;
    const int P = p.P, tid = threadIdx.x, lane = tid & 63;
    const int64_t N = p.N;
    for (int i = tid; i <= P; i += kEaThreads) hist[i] = 0;
    if (tid == 0) {
        const int K = *a.K;
        const EaDraws dr = ea_move_draws(p.seed, a.sweep, a.move, K, p.K, a.eject_a);
        sh_kind = dr.kind; sh_j1 = dr.j1; sh_j2 = dr.j2; sh_K = K; sh_salt = dr.salt; sh_pe = dr.pe;
        if (blockIdx.x == 0) {
            EaCell* c = a.cell;
            c->kind = dr.kind; c->j1 = dr.j1; c->j2 = dr.j2; c->salt = dr.salt; c->pe_bits = dbits(dr.pe);
            c->accepted = 0; c->members = 0; c->k_before = K; c->k_after = K;
            c->n_before[0] = a.Nk[dr.j1]; c->n_before[1] = dr.kind == kEaAbsorb ? a.Nk[dr.j2] : 0;
            c->n_after[0] = c->n_after[1] = 0;
            c->log_u = log_(dr.u);
            c->log_prior = c->log_lik = c->log_q = c->log_move = c->log_r = 0.0;
        }
    }
    __syncthreads();
    const int kind = sh_kind, j1 = sh_j1, j2 = sh_j2, last = sh_K - 1;
    const int64_t r = (int64_t)blockIdx.x * kEaThreads + tid;
    int sd = kEaOut;
    if (r < N) {
        const int zr = a.z[r];
        if (kind == kEaEject) {
            if (zr == j1) sd = sm_member_uniform(sh_salt, (uint64_t)(p.obs0 + r), 0u) < sh_pe ? 1 : 0;
        } else {
            if (zr == last && j2 != last) sd = 2;
            else if (zr == j2) sd = 1;
            else if (zr == j1) sd = 0;
        }
        a.side[r] = (uint8_t)sd;
    }
    if (kind != kEaEject) return;
    // the split-merge counting with every counted row on its side 0: the histogram's first set {n, S[P]} is all it
    // writes, and all this workgroup holds
    sm_count_wave(sd == 1, 0, a.Xb, N, P, r, hist, lane);
    __syncthreads();
    for (int i = tid; i <= P; i += kEaThreads) {
        const int32_t v = hist[i];
        if (v != 0) atomicAdd(&a.stat[i], v);
    }
}

// One workgroup: the marginal-likelihood ratio over the features in a fixed order (feature d in partial d mod 1024,
// ascending, then a binary tree), the prior ratio, log q in closed form, the decision and the counters.  Everything is
// computed in the eject's direction, from the smaller K; an absorb negates it.
__global__ __launch_bounds__(1024) void k_ea_decide(ChainParams p, EaArgs a) {
    __shared__ double sh[1024];
    const int t = threadIdx.x, P = p.P;
    EaCell* const c = a.cell;
    const bool eject = c->kind == kEaEject;
    const int j1 = c->j1, j2 = c->j2, K = c->k_before;
    const int64_t n1 = eject ? (int64_t)a.Nk[j1] - a.stat[0] : a.Nk[j1];
    const int64_t n2 = eject ? a.stat[0] : a.Nk[j2];
    const int64_t n = n1 + n2;
    double ll = 0.0;
    for (int d = t; d < P; d += 1024) {
        const int64_t sa = a.S[(size_t)j1 * P + d];
        const int64_t s2 = eject ? a.stat[1 + d] : a.S[(size_t)j2 * P + d];
        const int64_t s1 = eject ? sa - s2 : sa, s = s1 + s2;
        ll = ll + ((sm_pair(p.beta, p.gamma, n1, s1) + sm_pair(p.beta, p.gamma, n2, s2)) - sm_pair(p.beta, p.gamma, n, s));
    }
    sh[t] = ll;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    if (t != 0) return;
    const double bg = p.beta + p.gamma, A = a.a, e = a.eject_a, Nd = (double)p.Ntot;
    const double c0 = (lgamma_(bg) - lgamma_(p.beta)) - lgamma_(p.gamma);
    const double cst = ((c0 - lgamma_(bg + (double)n1)) - lgamma_(bg + (double)n2)) + lgamma_(bg + (double)n);
    const double lik = sh[0] + (double)P * cst;
    const int Kl = eject ? K : K - 1;  // the smaller K: the eject goes from Kl to Kl + 1
    const double ka = (double)Kl * A, kb = (double)(Kl + 1) * A;
    const double prior = (((a.log_prior_k[Kl] - a.log_prior_k[Kl - 1]) + ((lgamma_(kb) - lgamma_(kb + Nd)) - (lgamma_(ka) - lgamma_(ka + Nd)))) +
                          ((lgamma_(A + (double)n1) + lgamma_(A + (double)n2)) - lgamma_(A + (double)n))) - lgamma_(A);
    const double log_q = ea_log_q(e, n1, n2);
    // log(1 - pe_{Kl + 1}) - log pe_{Kl}: pe_1 = 1, pe_maxK = 0, 1/2 otherwise
    const double log_move = log_(Kl + 1 == p.K ? 1.0 : 0.5) - log_(Kl == 1 ? 1.0 : 0.5);
    const double log_prior = eject ? prior : -prior, log_lik = eject ? lik : -lik;
    const double log_r = eject ? ((log_prior + log_lik) + log_move) - log_q : ((log_prior + log_lik) - log_move) + log_q;
    const int acc = c->log_u < log_r ? 1 : 0;
    c->log_prior = log_prior; c->log_lik = log_lik; c->log_q = log_q; c->log_move = log_move; c->log_r = log_r;
    c->accepted = acc;
    c->n_after[0] = eject ? n1 : n; c->n_after[1] = eject ? n2 : 0;
    c->members = n2;
    c->k_after = acc ? (eject ? K + 1 : K - 1) : K;
    a.counters[eject ? 0 : 2] += 1;
    if (acc) a.counters[eject ? 1 : 3] += 1;
}

// An accepted move: the labels, the exact integer statistics of the labels touched (the swapped label included) and K.
// A rejected one: nothing.
__global__ __launch_bounds__(kEaThreads) void k_ea_commit(ChainParams p, EaArgs a) {
    const EaCell* const c = a.cell;
    if (!c->accepted) return;
    const int P = p.P, tid = threadIdx.x, j1 = c->j1, j2 = c->j2, last = c->k_before - 1;
    const bool eject = c->kind == kEaEject;
    const int64_t r = (int64_t)blockIdx.x * kEaThreads + tid;
    if (r < p.N) {
        const int sd = a.side[r];
        if (eject) { if (sd == 1) a.z[r] = j2; }
        else if (sd == 1) a.z[r] = (j1 == last && j2 != last) ? j2 : j1;
        else if (sd == 2) a.z[r] = j2;
    }
    if (blockIdx.x != 0) return;
    for (int idx = tid; idx <= P; idx += kEaThreads) {
        int32_t* const A = idx == 0 ? a.Nk + j1 : a.S + (size_t)j1 * P + (idx - 1);
        int32_t* const B = idx == 0 ? a.Nk + j2 : a.S + (size_t)j2 * P + (idx - 1);
        int32_t* const Z = idx == 0 ? a.Nk + last : a.S + (size_t)last * P + (idx - 1);
        if (eject) {
            const int32_t v = a.stat[idx];
            *B = v; *A = *A - v;
        } else {  // in this order: j1 may be the last label
            const int32_t s = *A + *B;
            *A = s; *B = 0;
            if (j2 != last) { *B = *Z; *Z = 0; }
        }
    }
    if (tid == 0) *a.K = c->k_after;
}

// ---- split-merge moves of the allocation chain (include/bmm_mcmc.h "split-merge moves of the allocation sampler";
// DESIGN.md section 24): the ALLOC flavour of k_sm_launch / k_sm_scan / k_sm_decide / k_sm_commit above.

// ---- ECR relabelling from the label trace alone (include/bmm_mcmc.h "ECR") -----------------
// Label rows as the partition kernels hold them: 0-based, row t at lab + t * pitch, either the resident int32 trace
// (pitch = N; -1 = unassigned, skipped everywhere) or the one-byte block k_pt_narrow makes of host input.  The pivot
// is N int32 labels.  A table is K^2 uint32, cell a * K + b = #{i : z_t[i] = a, pivot[i] = b}: read as a K x K
// column-major matrix its rows are pivot labels and its columns draw labels, which is the cost matrix k_st_assign
// takes once negated.  Every count is an integer add, so the results do not depend on scheduling.
constexpr int kEcrThreads = 256;
constexpr int kEcrMaxRows = 8;     // label rows per workgroup of k_ecr_tables
constexpr int kEcrMaxCopies = 16;  // copies of a row's table in LDS

// Workgroup (x, y): rows [y * T, y * T + T) against observations [x * span, x * span + span).  LDS form: R copies of
// each row's table, a lane adding to copy lane mod R -- section 13 found k_pt_pairs bound by the lanes of one wave
// adding to one bin (a few big clusters own most cells), so the copies go across the lanes of a wave here, not across
// the waves -- and a copy is K^2 | 1 words long, so that the same cell of neighbouring copies lies in neighbouring
// banks.  The copies are summed and flushed with one global integer add per non-empty cell.  Generic form (a table
// does not fit): the adds go to the global table directly.  Dynamic LDS: T * R * (K^2 | 1) uint32, or none.
template <class L, bool LDS>
__global__ __launch_bounds__(256) void k_ecr_tables(const L* __restrict__ lab, int64_t pitch,
                                                    const int32_t* __restrict__ pivot, int64_t N, int S, int K, int T,
                                                    int R, int64_t span, uint32_t* __restrict__ tables) {
    extern __shared__ uint32_t ecr_lds[];
    const int tid = threadIdx.x;
    const int t0 = blockIdx.y * T;
    const int nT = t0 + T < S ? T : S - t0;
    const int64_t i0 = (int64_t)blockIdx.x * span;
    const int64_t i1 = i0 + span < N ? i0 + span : N;
    const int KK = K * K, CS = KK | 1, TS = R * CS;
    if (LDS) {
        for (int k = tid; k < nT * TS; k += kEcrThreads) ecr_lds[k] = 0;
        __syncthreads();
    }
    uint32_t* const mine = ecr_lds + (tid % R) * CS;
    const L* __restrict__ rows = lab + (size_t)t0 * pitch;
    uint32_t* const out = tables + (size_t)t0 * KK;
    for (int64_t i = i0 + tid; i < i1; i += kEcrThreads) {
        const int b = pivot[i];
        if ((uint32_t)b >= (uint32_t)K) continue;
#pragma unroll 4
        for (int tt = 0; tt < nT; ++tt) {
            const int a = (int)rows[(size_t)tt * pitch + i];
            if ((uint32_t)a >= (uint32_t)K) continue;  // unassigned
            if (LDS) atomicAdd(mine + tt * TS + a * K + b, 1u);
            else atomicAdd(out + (size_t)tt * KK + a * K + b, 1u);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int e = tid; e < nT * KK; e += kEcrThreads) {
            const int tt = e / KK, k = e - tt * KK;
            uint32_t n = 0;
            for (int r = 0; r < R; ++r) n += ecr_lds[tt * TS + r * CS + k];
            if (n) atomicAdd(out + e, n);
        }
    }
}

// cost(t) = -(double) table(t), cell for cell: exact, and already in the layout of k_st_assign.  Grid (ceil(K^2 / 256), S).
__global__ __launch_bounds__(256) void k_ecr_cost(const uint32_t* __restrict__ tables, int KK, double* __restrict__ cost) {
    const int e = blockIdx.x * kEcrThreads + threadIdx.x;
    if (e < KK) cost[(size_t)blockIdx.y * KK + e] = -(double)tables[(size_t)blockIdx.y * KK + e];
}

// agree[t] = sum_a table(t)[a, perm(t, a)] and total += agree[t] (an integer add: exact in any order).  One wave per row.
__global__ __launch_bounds__(64) void k_ecr_agree(const uint32_t* __restrict__ tables, int K,
                                                  const int32_t* __restrict__ perm, int64_t ld,
                                                  int64_t* __restrict__ agree, unsigned long long* __restrict__ total) {
    __shared__ unsigned long long part[64];
    const int lane = threadIdx.x, t = blockIdx.x;
    const uint32_t* __restrict__ tab = tables + (size_t)t * K * K;
    unsigned long long s = 0;
    for (int a = lane; a < K; a += 64) {
        const int b = min(max(perm[t + (int64_t)a * ld], 0), K - 1);
        s += tab[a * K + b];
    }
    part[lane] = s;
    __syncthreads();
    for (int h = 32; h > 0; h >>= 1) {
        if (lane < h) part[lane] += part[lane + h];
        __syncthreads();
    }
    if (lane == 0) {
        agree[t] = (int64_t)part[0];
        atomicAdd(total, part[0]);
    }
}

// The pivot of the iterative form: observation i gets the label with the most votes among perm(t, z_t[i]) over the S
// rows, the lowest label on a tie.  One thread per observation down the rows (a wave reads 64 neighbouring labels of
// a row), K 16-bit counters per thread (S <= 65535), two to a word, word w of thread j at [w * stride + j]: in LDS
// stride = 256, so the lanes of a wave are in 64 neighbouring words whatever labels they count; in the generic form
// (the counters of 256 threads do not fit) the same layout in global memory, stride = the threads of the grid.
// Dynamic LDS: ceil(K / 2) * 256 uint32, or none.
template <class L, bool LDS>
__global__ __launch_bounds__(256) void k_ecr_votes(const L* __restrict__ lab, int64_t pitch,
                                                   const int32_t* __restrict__ perm, int64_t ld, int64_t N, int S, int K,
                                                   uint32_t* __restrict__ scratch, int32_t* __restrict__ pivot) {
    extern __shared__ uint32_t ecr_lds[];
    const int tid = threadIdx.x;
    const int W = (K + 1) / 2;
    const int64_t nth = (int64_t)gridDim.x * kEcrThreads;
    const int64_t j = (int64_t)blockIdx.x * kEcrThreads + tid;
    uint32_t* const cnt = LDS ? ecr_lds + tid : scratch + j;
    const int64_t stride = LDS ? kEcrThreads : nth;
    for (int64_t i = j; i < N; i += nth) {
        for (int w = 0; w < W; ++w) cnt[w * stride] = 0;
        for (int t = 0; t < S; ++t) {
            const int a = (int)lab[(size_t)t * pitch + i];
            if ((uint32_t)a >= (uint32_t)K) continue;  // unassigned
            const int v = min(max(perm[t + (int64_t)a * ld], 0), K - 1);
            cnt[(v >> 1) * stride] += 1u << (16 * (v & 1));
        }
        uint32_t best = 0;
        int bk = 0;
        for (int k = 0; k < K; ++k) {
            const uint32_t n = (cnt[(k >> 1) * stride] >> (16 * (k & 1))) & 0xffffu;
            if (n > best) { best = n; bk = k; }
        }
        pivot[i] = bk;
    }
}

__global__ void k_test_lgamma(const double* in, double* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = lgamma_(in[i]);
}

// ---- log joint trace and keep-best allocation (include/bmm_mcmc.h "log joint trace") --------
// The log joint of the chain's state from its integer statistics, in the order bmm_spec.h states (log_joint_spec is
// the same statement for the host).  k_log_joint: one workgroup of kLjLanes threads per label and, with a mask, one
// more for the pooled term of the excluded features; thread t adds the cells of features t, t + kLjLanes, ... in
// ascending order, the partials are folded by a binary tree in LDS, thread 0 writes the label's total and its prior
// term.  The statistics are read as they stand, pending deltas added and nothing cleared (as k_state_tables reads
// them), so a finite chain before its first sweep is scored from its delta replicas.  No X is read: both layouts, any
// P, up to kMaxCatsAny labels.  k_log_joint_finish: one lane adds the labels' values in ascending order, writes the
// row and, when the state is folded, decides `improved` for the keep-best cell; k_log_joint_keep then copies the
// label row only when `improved` is set -- stream-ordered behind the lane that wrote it, so no block reads a cell
// another is writing.  Nothing is atomic in global memory: one state gives the same bits twice.
struct LjBest {
    double total;      // the largest log_joint folded so far (-inf: none)
    int32_t sweep;     // the sweep it belongs to (-1: none)
    int32_t improved;  // whether the last folded state replaced it
};
struct LjArgs {
    const int32_t *Nk, *S, *dNk, *dS;  // the chain's statistics and their delta replicas
    const uint32_t* mask;              // [ceil(P / 32)] words, or null: no feature mask
    const double* alpha_ptr;
    const int32_t* k_open;             // the allocation sampler's open label count, or null
    const double* log_prior_k;         // ... and its log p(K), K = 1 .. maxK
    double *lik, *prior;               // [K + 1], [K]: the labels' values between the two launches (lik[K]: the pooled term)
    double* out;                       // [4]: the row
    double* out_row;                   // or null: [4], this sweep's row of a trace
    LjBest* best;                      // the keep-best cell
    double rho;
    int kind;                          // LJ_*
    int sweep, fold;
};
__device__ __forceinline__ LjModel lj_model_of(const ChainParams& p, const LjArgs& a) {
    LjModel m;
    m.kind = a.kind; m.K = p.K; m.k_open = a.k_open ? *a.k_open : p.K; m.P = p.P; m.N = p.N;
    m.beta = p.beta; m.gamma = p.gamma; m.alpha = *a.alpha_ptr; m.sample_alpha = p.sample_alpha; m.a = p.a; m.b = p.b;
    m.log_pk = 0.0; m.masked = a.mask != nullptr; m.rho = a.rho; m.p_in = p.P;
    return m;
}
__global__ __launch_bounds__(kLjLanes) void k_log_joint(ChainParams p, LjArgs a) {
    __shared__ double part[kLjLanes];
    __shared__ double sh_c[2];  // lgamma_(beta + gamma + n), lB(beta, gamma)
    __shared__ unsigned long long sh_after;
    const int K = p.K, P = p.P, tid = threadIdx.x, k = blockIdx.x;
    const size_t KP = (size_t)K * P;
    const LjModel m = lj_model_of(p, a);
    const bool pooled = k == K;  // (launched with a mask only)
    const int64_t n = pooled ? p.N : (int64_t)a.Nk[k] + delta_take(const_cast<int32_t*>(a.dNk), k, K);
    const bool lik_on = pooled || lj_label_lik(m, k, n);  // uniform over the workgroup
    if (tid == 0) {
        sh_after = 0ull;
        if (lik_on) { sh_c[0] = lgamma_((p.beta + p.gamma) + (double)n); sh_c[1] = lj_lb0(p.beta, p.gamma); }
    }
    __syncthreads();
    double acc = 0.0;
    if (lik_on) {
        const double lgden = sh_c[0], lb0 = sh_c[1];
        for (int d = tid; d < P; d += kLjLanes) {
            if (lj_included(a.mask, d) == pooled) continue;
            int64_t s = 0;
            if (!pooled) {
                s = (int64_t)a.S[(size_t)k * P + d] + delta_take(const_cast<int32_t*>(a.dS), (size_t)k * P + d, KP);
            } else {
                for (int l = 0; l < K; ++l)
                    s += (int64_t)a.S[(size_t)l * P + d] + delta_take(const_cast<int32_t*>(a.dS), (size_t)l * P + d, KP);
            }
            acc = acc + lj_cell(p.beta, p.gamma, n, s, lgden, lb0);
        }
    }
    part[tid] = acc;
    // the rows of the labels above k (the stick-breaking prior): an integer, so the order of the adds is free
    const bool prior_on = !pooled && lj_label_prior(m, k, n);
    if (prior_on && m.kind == LJ_SB) {
        unsigned long long after = 0ull;
        for (int l = k + 1 + tid; l < K; l += kLjLanes)
            after += (unsigned long long)((int64_t)a.Nk[l] + delta_take(const_cast<int32_t*>(a.dNk), l, K));
        if (after) atomicAdd(&sh_after, after);  // LDS
    }
    __syncthreads();
    for (int o = kLjLanes / 2; o > 0; o >>= 1) {
        if (tid < o) part[tid] = part[tid] + part[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        a.lik[k] = part[0];
        if (!pooled) a.prior[k] = prior_on ? lj_prior_term(m, n, (int64_t)sh_after) : 0.0;
    }
}
struct LjNkOf {
    const int32_t *Nk, *dNk;
    int K;
    __device__ int64_t operator()(int k) const { return (int64_t)Nk[k] + delta_take(const_cast<int32_t*>(dNk), k, K); }
};
__global__ __launch_bounds__(64) void k_log_joint_finish(ChainParams p, LjArgs a) {
    if (threadIdx.x != 0) return;
    LjModel m = lj_model_of(p, a);
    if (a.log_prior_k) m.log_pk = a.log_prior_k[m.k_open - 1];
    if (a.mask) {
        int in = 0;
        for (int w = 0; w < (p.P + 31) / 32; ++w) in += __popc(a.mask[w] & init_word_mask(p.P, w));
        m.p_in = in;
    }
    double row[4];
    lj_finish(m, a.lik, a.prior, LjNkOf{a.Nk, a.dNk, p.K}, a.mask ? a.lik[p.K] : 0.0, row);
    for (int q = 0; q < 4; ++q) {
        a.out[q] = row[q];
        if (a.out_row) a.out_row[q] = row[q];
    }
    if (a.fold) {
        const bool improved = row[3] > a.best->total;  // strict: the earliest sweep wins a tie, a NaN never wins
        a.best->improved = improved ? 1 : 0;
        if (improved) { a.best->total = row[3]; a.best->sweep = a.sweep; }
    }
}
__global__ __launch_bounds__(256) void k_log_joint_keep(const LjBest* __restrict__ best, const int32_t* __restrict__ z,
                                                        int64_t N, int32_t* __restrict__ z_best) {
    if (!best->improved) return;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) z_best[i] = z[i];
}

// ---- pairwise local-dependence check (include/bmm_mcmc.h "pairwise local-dependence check") ----
// k_pc_slices, once per arming: the chosen features out of the bit planes into column slices Xt[m][C], C = ceil(N/64)
// words of 64 rows; bit r of word c is x of row 64 c + r, bits past N are zero.  One ballot per feature and chunk.
// k_pc_counts, once per evaluated state: a workgroup of kPcThreads lanes owns a kPcTile x kPcTile block of the upper
// triangle of the M x M pairs (blockIdx.x, diagonal blocks included), a slice of the chunks (blockIdx.y) and KA labels
// (blockIdx.z).  Per round of kPcRound chunks it stages the 2 kPcTile slices of the tile and the labels of those rows
// in LDS.  Lane (q, lj) owns the R pairs (R q .. R q + R - 1, lj) of the tile.  Per chunk a wave reads the 64 labels,
// one per lane, and forms mask_k = ballot(z == k) itself: a compare whose result is a scalar register pair, used as
// it is by the R pairs of every lane -- no mask goes through LDS (the first form staged them there, and one LDS read
// per pair, label and chunk held the kernel at a third of its rate) -- and each pair adds
// popcount(slice_a & slice_b & mask_k) into its KA accumulators.  The margins come from the same pass, so the result
// is a function of (X, z) alone: a pair slot on the diagonal of a diagonal tile holds slice & slice = the feature's
// own ones (s_kd), and the first wave of the first tile adds popcount(mask_k) (n_k) in scalar registers.  Slots below
// the diagonal are computed and dropped.  At the end every non-zero accumulator is added with one integer atomic; the
// buffers are zeroed stream-ordered ahead of the launch.  Labels below 0 never reach the kernel (the callers refuse
// such states); they would match no mask.
// k_pc_stats: one lane per pair walks the labels in ascending order with bmm_spec.h's pc_label, writes the state's
// values, the trace row if one is recorded, and adds to the fold.  No floating-point atomic anywhere.
constexpr int kPcTile = 32, kPcRound = 16, kPcKA = 8, kPcR = 4, kPcThreads = kPcTile * kPcTile / kPcR;
struct PcArgs {
    const uint64_t* Xt;  // [M][C]
    const int32_t* z;    // [N], 0-based
    int64_t N, C;        // rows, chunks of 64 rows
    int64_t cps;         // chunks per row slice (a multiple of kPcRound)
    int M, Kc;
    uint32_t *cnt, *marg, *nk;  // [Kc][npairs], [Kc][M], [Kc]
};
__global__ __launch_bounds__(256) void k_pc_slices(const uint32_t* __restrict__ Xb, int64_t N, const int32_t* __restrict__ feat,
                                                   int64_t C, uint64_t* __restrict__ Xt) {
    const int m = blockIdx.y, f = feat[m], lane = threadIdx.x & 63;
    const uint32_t* plane = Xb + (size_t)(f >> 5) * (size_t)N;
    for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < C; c += (int64_t)gridDim.x * 4) {
        const int64_t row = c * 64 + lane;
        const bool bit = row < N && ((plane[row] >> (f & 31)) & 1u);
        const unsigned long long b = __ballot(bit);
        if (lane == 0) Xt[(size_t)m * (size_t)C + (size_t)c] = b;
    }
}
template <int KA, int R>
__global__ __launch_bounds__(kPcThreads) void k_pc_counts(PcArgs a) {
    static_assert(kPcTile * kPcTile == kPcThreads * R && kPcTile % R == 0, "a tile is R pairs per lane");
    __shared__ unsigned long long sX[kPcRound][2 * kPcTile];
    __shared__ int32_t sZ[kPcRound][64];
    const int tid = threadIdx.x, q = tid >> 5, lj = tid & 31, lane = tid & 63;
    const int T = (a.M + kPcTile - 1) / kPcTile;
    int ti = 0, tj = (int)blockIdx.x;
    while (tj >= T - ti) { tj -= T - ti; ++ti; }
    tj += ti;
    const int j = tj * kPcTile + lj, kbase = (int)blockIdx.z * KA;
    const bool rows = blockIdx.x == 0 && tid < 64;  // uniform over a wave
    const int64_t c_lo = (int64_t)blockIdx.y * a.cps, c_hi = c_lo + a.cps < a.C ? c_lo + a.cps : a.C;
    uint32_t acc[R][KA], nrows[KA];
#pragma unroll
    for (int k = 0; k < KA; ++k) {
        nrows[k] = 0u;
#pragma unroll
        for (int p = 0; p < R; ++p) acc[p][k] = 0u;
    }
    for (int64_t c0 = c_lo; c0 < c_hi; c0 += kPcRound) {
        // kPcRound x 2 kPcTile slice words and kPcRound x 64 labels, kPcThreads lanes
        for (int t = tid; t < kPcRound * 2 * kPcTile; t += kPcThreads) {
            const int sf = t / kPcRound, sr = t % kPcRound;
            const int sm = sf < kPcTile ? ti * kPcTile + sf : tj * kPcTile + (sf - kPcTile);
            const int64_t c = c0 + sr;
            sX[sr][sf] = (sm < a.M && c < c_hi) ? a.Xt[(size_t)sm * (size_t)a.C + (size_t)c] : 0ull;
        }
        for (int t = tid; t < kPcRound * 64; t += kPcThreads) {
            const int64_t c = c0 + (t >> 6), row = c * 64 + (t & 63);
            sZ[t >> 6][t & 63] = (c < c_hi && row < a.N) ? a.z[row] : -1;
        }
        __syncthreads();
#pragma unroll 2
        for (int r = 0; r < kPcRound; ++r) {
            const int32_t zz = sZ[r][lane];
            const unsigned long long b = sX[r][kPcTile + lj];
            uint32_t wlo[R], whi[R];
#pragma unroll
            for (int p = 0; p < R; ++p) {
                const unsigned long long w = sX[r][q * R + p] & b;
                wlo[p] = (uint32_t)w; whi[p] = (uint32_t)(w >> 32);
            }
#pragma unroll
            for (int k = 0; k < KA; ++k) {
                const unsigned long long m = __ballot(zz == kbase + k);
                const uint32_t mlo = (uint32_t)m, mhi = (uint32_t)(m >> 32);
                if (rows) nrows[k] += (uint32_t)__popcll(m);
                // two population counts that add into the accumulator as they count
#pragma unroll
                for (int p = 0; p < R; ++p) acc[p][k] = (uint32_t)__popc(whi[p] & mhi) + ((uint32_t)__popc(wlo[p] & mlo) + acc[p][k]);
            }
        }
        __syncthreads();
    }
    const int64_t np = pc_npairs(a.M);
#pragma unroll
    for (int p = 0; p < R; ++p) {
        const int i = ti * kPcTile + q * R + p;
        uint32_t* dst = nullptr;
        size_t stride = 0;
        if (i < j && j < a.M) { dst = a.cnt + pc_pair_index(i, j, a.M); stride = (size_t)np; }
        else if (i == j && i < a.M) { dst = a.marg + i; stride = (size_t)a.M; }
        if (!dst) continue;
#pragma unroll
        for (int k = 0; k < KA; ++k)
            if (kbase + k < a.Kc && acc[p][k]) atomicAdd(dst + (size_t)(kbase + k) * stride, acc[p][k]);
    }
    if (rows && tid == 0) {
#pragma unroll
        for (int k = 0; k < KA; ++k)
            if (kbase + k < a.Kc && nrows[k]) atomicAdd(a.nk + (kbase + k), nrows[k]);
    }
}
struct PcStatArgs {
    const uint32_t *cnt, *marg, *nk;
    int M, Kc;
    double *z, *x2;       // [npairs]: the state's values
    int32_t* df;
    double* out_row;      // or null: [2 npairs], Z then X2, this sweep's row of a trace
    double *sum_z, *sum_z2, *sum_x2;  // the fold
    long long* sum_df;
    int32_t* n_z;
    uint32_t* n11;
    int fold;
};
__global__ __launch_bounds__(256) void k_pc_stats(PcStatArgs a) {
    const int64_t np = pc_npairs(a.M), q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= np) return;
    int i = 0, j = 0;
    pc_pair_ij(q, a.M, i, j);
    PcSums t = pc_zero();
    uint32_t both = 0u;
    for (int k = 0; k < a.Kc; ++k) {
        const uint32_t c = a.cnt[(size_t)k * np + q];
        both += c;
        pc_label(t, (int64_t)c, (int64_t)a.nk[k], (int64_t)a.marg[(size_t)k * a.M + i], (int64_t)a.marg[(size_t)k * a.M + j]);
    }
    const double z = pc_z(t);
    a.z[q] = z; a.x2[q] = t.X2; a.df[q] = t.df;
    if (a.out_row) { a.out_row[q] = z; a.out_row[np + q] = t.X2; }
    if (a.fold) {
        if (t.V > 0.0) { a.sum_z[q] = a.sum_z[q] + z; a.sum_z2[q] = a.sum_z2[q] + z * z; a.n_z[q] += 1; }
        a.sum_x2[q] = a.sum_x2[q] + t.X2;
        a.sum_df[q] += t.df;
        a.n11[q] = both;
    }
}

// ---- missing data: NA cells imputed behind every sweep (include/bmm_mcmc.h "missing data") ----
// The missing cells are a list of sites: one (row i, plane word w) with the mask of its missing bits and the index of its
// first cell in the caller's (row, column) order, so a site's cells are consecutive there.  One thread owns a site: it
// reads z_i and the word Xb[w * N + i], rewrites the masked bits and stores the word with a plain store -- no two
// threads touch the same word, and a cell's sums have one owner too, so nothing floating-point is atomic and one seed
// gives the same bits twice.  What is atomic is integer: the census and the S deltas, added in LDS per workgroup
// (ds_add_u32; lanes that meet on a bank take turns, nothing more) and flushed with one device-scope atomicAdd per
// non-empty cell, which is resolved in the memory side of the L2s and so holds across XCDs; integer adds in any order
// give the same bits.  The site arrays are read a lane a site (coalesced), the words are gathers: a wave's 64 sites lie
// in ascending (row, word) order, so its words of one plane fall into few cache lines when the holes are dense and into
// one line each when they are sparse -- 64 B fetched for 4 B used, the price of a hole.
// Above kNaLdsBytes the tables stay in global memory: the census and the deltas add there, phi / theta is read there.
constexpr int kNaThreads = 256;
constexpr size_t kNaLdsBytes = 49152;  // what the other histogram kernels allow themselves
__host__ __device__ inline bool na_tables_in_lds(int K, int P) { return (size_t)K * (size_t)P * 8 <= kNaLdsBytes; }
struct NaArgs {
    const int64_t* row;     // [n_sites]
    const int32_t* word;    // [n_sites] plane word w
    const uint32_t* mask;   // [n_sites] the missing bits of the word
    const int64_t* first;   // [n_sites] index of the site's first cell in the cell list
    int64_t n_sites;
    uint32_t* Xb;           // the planes [W][N]
    const int32_t* z;       // [N] labels, 0-based (< 0: the row has no seat yet and is left alone); null: no row has one
    int32_t* S;             // [K][P] the folded counts the deltas are added to
    int32_t* cnt;           // [2][K*P]: M_kj, then O_kj (k_na_census, k_na_phi)
    int32_t *Nk, *dNk, *dS; // the chain's sizes and pending deltas (k_na_phi reads the sums)
    double* phi;            // [k + j*K]: the step's rates -- the auxiliary draws of a counting chain, theta of an explicit one
    double* sum_phi;        // [n_cells] folds, or null
    uint32_t* ones;         // [n_cells]
    uint32_t sweep;
    int fold;
};

// the starting fill: every cell Bernoulli(beta / (beta + gamma)) from the uniform of sweep 0; rows with a seat move S
__global__ __launch_bounds__(kNaThreads) void k_na_fill(ChainParams p, NaArgs a) {
    const double rate = div_(p.beta, p.beta + p.gamma);
    for (int64_t t = (int64_t)blockIdx.x * kNaThreads + threadIdx.x; t < a.n_sites; t += (int64_t)gridDim.x * kNaThreads) {
        const int64_t i = a.row[t];
        const int w = a.word[t];
        const int k = a.z ? a.z[i] : -1;
        uint32_t m = a.mask[t];
        const size_t at = (size_t)w * (size_t)p.N + (size_t)i;
        uint32_t x = a.Xb[at];
        while (m) {
            const int b = __ffs(m) - 1;
            m &= m - 1;
            const int j = w * 32 + b;
            const uint32_t nb = na_uniform(p.seed, (uint64_t)i * (uint64_t)p.P + (uint64_t)j, 0u) < rate ? 1u : 0u;
            const int d = (int)nb - (int)((x >> b) & 1u);
            x = (x & ~(1u << b)) | (nb << b);
            if (d != 0 && k >= 0) atomicAdd(&a.S[(size_t)k * p.P + j], d);
        }
        a.Xb[at] = x;
    }
}

// the sites' words as they stand, for the host (bmm_chain_get_missing_state)
__global__ __launch_bounds__(kNaThreads) void k_na_words(ChainParams p, NaArgs a, uint32_t* __restrict__ out) {
    for (int64_t t = (int64_t)blockIdx.x * kNaThreads + threadIdx.x; t < a.n_sites; t += (int64_t)gridDim.x * kNaThreads)
        out[t] = a.Xb[(size_t)a.word[t] * (size_t)p.N + (size_t)a.row[t]];
}

// flush of an LDS table of n integers into global memory: one add per non-empty cell
__device__ __forceinline__ void na_flush(const int32_t* hist, int n, int32_t* dst) {
    for (int q = threadIdx.x; q < n; q += kNaThreads) {
        const int32_t v = hist[q];
        if (v != 0) atomicAdd(&dst[q], v);
    }
}

// counting chains: M_kj, the missing cells among label k's rows, and O_kj, how many of them hold a 1
template <bool LDS>
__global__ __launch_bounds__(kNaThreads) void k_na_census(ChainParams p, NaArgs a) {
    extern __shared__ int32_t na_hist[];
    const int KP = p.K * p.P;
    if (LDS) {
        for (int q = threadIdx.x; q < 2 * KP; q += kNaThreads) na_hist[q] = 0;
        __syncthreads();
    }
    int32_t* const dst = LDS ? na_hist : a.cnt;
    for (int64_t t = (int64_t)blockIdx.x * kNaThreads + threadIdx.x; t < a.n_sites; t += (int64_t)gridDim.x * kNaThreads) {
        const int64_t i = a.row[t];
        const int k = a.z[i];
        if (k < 0) continue;
        const int w = a.word[t];
        uint32_t m = a.mask[t];
        const uint32_t x = a.Xb[(size_t)w * (size_t)p.N + (size_t)i];
        while (m) {
            const int b = __ffs(m) - 1;
            m &= m - 1;
            const int kj = k * p.P + w * 32 + b;
            atomicAdd(&dst[kj], 1);
            if ((x >> b) & 1u) atomicAdd(&dst[KP + kj], 1);
        }
    }
    if (LDS) {
        __syncthreads();
        na_flush(na_hist, 2 * KP, a.cnt);
    }
}

// counting chains: phi_kj ~ Beta(beta + s, gamma + n - s) from the observed-only counts, where a label has a hole in the feature
__global__ __launch_bounds__(kNaThreads) void k_na_phi(ChainParams p, NaArgs a) {
    const int KP = p.K * p.P;
    const int kj = blockIdx.x * kNaThreads + threadIdx.x;
    if (kj >= KP) return;
    const int32_t M = a.cnt[kj];
    if (M <= 0) return;
    const int k = kj / p.P, j = kj % p.P;
    const int64_t s = (int64_t)a.S[kj] + delta_take(a.dS, (size_t)kj, (size_t)KP) - a.cnt[KP + kj];
    const int64_t n = (int64_t)a.Nk[k] + delta_take(a.dNk, (size_t)k, (size_t)p.K) - M;
    a.phi[k + (size_t)j * p.K] = na_phi(p.seed, p.beta, p.gamma, (uint32_t)kj, a.sweep, s, n);
}

// the draw: bit = u_ij < phi_{z_i, j} for every missing cell, the word rewritten, S moved by the sum of (new - old)
template <bool LDS>
__global__ __launch_bounds__(kNaThreads) void k_na_draw(ChainParams p, NaArgs a) {
    extern __shared__ double na_tab[];
    const int KP = p.K * p.P;
    int32_t* const hist = reinterpret_cast<int32_t*>(na_tab + KP);
    if (LDS) {
        for (int q = threadIdx.x; q < KP; q += kNaThreads) { na_tab[q] = a.phi[q]; hist[q] = 0; }
        __syncthreads();
    }
    const double* const phi = LDS ? na_tab : a.phi;
    int32_t* const dst = LDS ? hist : a.S;
    for (int64_t t = (int64_t)blockIdx.x * kNaThreads + threadIdx.x; t < a.n_sites; t += (int64_t)gridDim.x * kNaThreads) {
        const int64_t i = a.row[t];
        const int k = a.z[i];
        if (k < 0) continue;
        const int w = a.word[t];
        uint32_t m = a.mask[t];
        int64_t cell = a.first[t];
        const size_t at = (size_t)w * (size_t)p.N + (size_t)i;
        uint32_t x = a.Xb[at];
        while (m) {
            const int b = __ffs(m) - 1;
            m &= m - 1;
            const int j = w * 32 + b;
            const double ph = phi[k + (size_t)j * p.K];
            const uint32_t nb = na_uniform(p.seed, (uint64_t)i * (uint64_t)p.P + (uint64_t)j, a.sweep) < ph ? 1u : 0u;
            const int d = (int)nb - (int)((x >> b) & 1u);
            x = (x & ~(1u << b)) | (nb << b);
            if (d != 0) atomicAdd(&dst[k * p.P + j], d);
            if (a.fold) {
                a.sum_phi[cell] = a.sum_phi[cell] + ph;
                a.ones[cell] += nb;
            }
            ++cell;
        }
        a.Xb[at] = x;
    }
    if (LDS) {
        __syncthreads();
        na_flush(hist, KP, a.S);
    }
}

// ---- posterior summary folded behind the sweeps (include/bmm_mcmc.h "posterior summary") ------
// The membership counts are K planes of `pitch` uint32 words, plane k word i = the folded sweeps in which observation
// i carried (relabelled) label k: the lanes of a wave own neighbouring observations, so whatever labels they carry
// they touch neighbouring words of at most K planes.  perm: the sweep's K-entry permutation (perm[l] = the label draw
// label l leaves as), entry l at perm[l]; an entry out of range is clamped, as k_ecr_agree clamps it.
constexpr int kSumThreads = 256;

// One lane per observation, grid-stride; the permutation is staged once per workgroup (dynamic LDS: K int32).  A word
// is owned by the lane of its observation: plain read-modify-write.  An unassigned label (-1) is skipped.
__global__ __launch_bounds__(kSumThreads) void k_sum_fold(const int32_t* __restrict__ z, const int32_t* __restrict__ perm,
                                                          int64_t N, int K, int64_t pitch, uint32_t* __restrict__ cnt) {
    extern __shared__ int32_t sum_perm[];
    for (int l = threadIdx.x; l < K; l += kSumThreads) sum_perm[l] = min(max(perm[l], 0), K - 1);
    __syncthreads();
    const int64_t nth = (int64_t)gridDim.x * kSumThreads;
    for (int64_t i = (int64_t)blockIdx.x * kSumThreads + threadIdx.x; i < N; i += nth) {
        const int a = z[i];
        if ((uint32_t)a >= (uint32_t)K) continue;  // unassigned
        uint32_t* const w = cnt + (size_t)sum_perm[a] * (size_t)pitch + (size_t)i;
        *w = *w + 1u;
    }
}

// K P lanes: cell (l, j) of the sweep's theta row (theta[l + j K], exactly as it goes into the theta trace) is added
// to cell (perm[l], j) of the sums, its square (rounded before the add) to the sums of squares; a NaN cell (the finite
// sampler's empty label) is left out, and theta_n[perm[l]] counts the sweeps whose cell (l, 0) was not NaN.  perm is a
// permutation, so every cell of the sums has one lane: one add per sweep, in sweep order.  Lane 0 also folds the
// sweep's alpha (acc[0] += alpha, acc[1] += alpha * alpha) and records the sweep's agreement (agree_in null: 0).
__global__ __launch_bounds__(kSumThreads) void k_sum_profiles(const double* __restrict__ theta, const double* __restrict__ alpha,
                                                              const int32_t* __restrict__ perm, int K, int P,
                                                              double* __restrict__ theta_sum, double* __restrict__ theta_sq,
                                                              int32_t* __restrict__ theta_n, double* __restrict__ alpha_acc,
                                                              const int64_t* __restrict__ agree_in, int64_t* __restrict__ agree_out) {
    const int e = blockIdx.x * kSumThreads + threadIdx.x;
    if (e < K * P) {
        const int j = e / K, l = e - j * K;
        const double t = theta[e];
        if (t == t) {
            const int to = min(max(perm[l], 0), K - 1);
            const size_t o = (size_t)to + (size_t)j * K;
            const double sq = __dmul_rn(t, t);
            theta_sum[o] = __dadd_rn(theta_sum[o], t);
            theta_sq[o] = __dadd_rn(theta_sq[o], sq);
            if (j == 0) theta_n[to] += 1;
        }
    }
    if (e == 0) {
        const double a = *alpha;
        const double sq = __dmul_rn(a, a);
        alpha_acc[0] = __dadd_rn(alpha_acc[0], a);
        alpha_acc[1] = __dadd_rn(alpha_acc[1], sq);
        if (agree_out) *agree_out = agree_in ? *agree_in : 0;
    }
}

// After the last fold: one lane per observation down the K planes (coalesced across the lanes) writes z_hat, the label
// with the largest count, the lowest on a tie, 1-based, and n_max, that count; size_sum[k] receives the sum of plane k,
// the cluster sizes under the permutations added over the folded sweeps (wave sums, then one integer add per
// workgroup and label: exact in any order).  size_sum is zero on entry.  Dynamic LDS: K uint64.
__global__ __launch_bounds__(kSumThreads) void k_sum_finish(const uint32_t* __restrict__ cnt, int64_t N, int K, int64_t pitch,
                                                            int32_t* __restrict__ z_hat, uint32_t* __restrict__ n_max,
                                                            unsigned long long* __restrict__ size_sum) {
    extern __shared__ unsigned long long sum_size[];
    for (int k = threadIdx.x; k < K; k += kSumThreads) sum_size[k] = 0;
    __syncthreads();
    const int64_t nth = (int64_t)gridDim.x * kSumThreads;
    for (int64_t base = (int64_t)blockIdx.x * kSumThreads; base < N; base += nth) {  // (a trip is uniform over the workgroup)
        const int64_t i = base + threadIdx.x;
        uint32_t best = 0;
        int bk = 0;
        for (int k = 0; k < K; ++k) {
            const uint32_t n = i < N ? cnt[(size_t)k * (size_t)pitch + (size_t)i] : 0u;
            if (n > best) { best = n; bk = k; }
            unsigned long long s = n;
            for (int h = 32; h > 0; h >>= 1) s += __shfl_down(s, h, 64);
            if ((threadIdx.x & 63) == 0 && s) atomicAdd(&sum_size[k], s);
        }
        if (i < N) { z_hat[i] = bk + 1; n_max[i] = best; }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += kSumThreads)
        if (sum_size[k]) atomicAdd(&size_sum[k], sum_size[k]);
}

}  // namespace bmm
