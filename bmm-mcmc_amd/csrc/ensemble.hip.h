// ensemble.hip.h -- k_ens_sweep: an ensemble of exact sequential-scan chains, one wavefront per chain
// (include/bmm_mcmc.h "ensemble of exact chains").
//
// A chain here is the batch = 1 chain of the counting samplers: every row is scored against the statistics as the row
// before it left them.  A label's log terms are a function of its counts alone, so a draw that keeps its label changes
// nothing and a draw that moves dirties two labels; at N < 2^16 the terms of every label, the counts and the
// exponential table of one chain fit in a slice of LDS, and one wave walks the rows.  There is no communication between
// waves: no barrier anywhere in this file, a workgroup is only a way to place several chains on one compute unit.
//
//   categories on lanes    lane k scores category k; its constants Cp, Cm and its size n_k live in lane k's registers
//   terms in LDS           T[(d * 4 + role) * Kc + k]: role 0, 1 = x is 1, 0 against the full statistics (term_x1,
//                          term_x0), role 2, 3 = the same with the scored row removed; neighbouring lanes read
//                          neighbouring doubles.  The DP's new cluster, category K, holds zeros
//   the order of a score   ((C + T_0) + T_1) + ..., T_g the group's terms added from 0.0 in ascending column order: the
//                          sums the 2^W-entry group tables of the other kernels hold (group_entry), taken column by
//                          column.  Lane z_i closes a group every kGroupWm columns, the others every W
//   rows                   64 at a time: lane l loads the plane words, the label and the uniform of row base + l from
//                          global memory (the planes are shared by all chains and stay in L2); the wave then takes the
//                          rows one by one through v_readlane
//   a move                 the counts of the two labels change in LDS (a column per lane) and their 8 P terms and 8
//                          constants are recomputed, one log_ per lane and pass
// The state of a chain lives in global memory between launches (labels, Nk, S, alpha), so a launch may stop after any
// row: a sweep over more than ens_rows(P) rows is several launches, each of which stages the counts and rebuilds every
// term from them -- the same values, being functions of the counts.  The launch that reaches row N ends the sweep:
// theta-hat, the concentration (update_alpha_wave) and the trace rows, by the chain's own wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bmm_spec.h"
#include "kernels.hip.h"  // update_alpha_wave

namespace bmm {

constexpr int kEnsWaves = 4;       // chains per workgroup, at most: a wave per SIMD
constexpr int kEnsRows = 2048;     // rows per launch, at most (a multiple of 64)
constexpr int kEnsMaxN = 1 << 16;  // N below this
constexpr int kEnsMaxCats = 64;
constexpr int kEnsMaxP = 128;

// Rows per launch, a multiple of 64: a move recomputes 8 P terms, ceil(P / 8) passes of one log_ per lane, and that is
// what a row costs at large P (measured: 1.2 us a row at P = 5, 5.8 us at P = 50), so the rows shrink with the passes and
// a launch stays near a millisecond or two.
__host__ __device__ inline int ens_rows(int P) {
    const int r = kEnsRows / ((P + 7) / 8) / 64 * 64;
    return r < 64 ? 64 : r;
}
// the LDS slice of one chain: T [4 P Kc] doubles, E [256] doubles, S [K P] int32; rounded up to 16 bytes
__host__ __device__ inline int64_t ens_slice_bytes(int P, int K, int Kc) {
    const int64_t b = ((int64_t)4 * P * Kc + 256) * 8 + (int64_t)K * P * 4;
    return (b + 15) / 16 * 16;
}

struct EnsArgs {
    const uint32_t* Xb;  // bit planes: word w of row i at Xb[w * N + i]
    int N, P, K, Kc, W;  // Kc = K (+ 1: the DP's new cluster); W: bmm_spec_group_width_for
    int chains, cpw;     // chains per workgroup
    int slice_bytes;
    int lo, hi;          // the rows of this launch; lo a multiple of 64; hi == N ends the sweep
    uint32_t sweep;
    double beta, gamma, a, b;
    int sample_alpha;
    uint64_t seed;       // chain c draws under seed + c
    int32_t* z;          // [chains][N] 0-based, -1 unassigned
    int32_t* Nk;         // [chains][K]
    int32_t* S;          // [chains][K * P], S[k * P + d]
    double* alpha;       // [chains]
    int row, rows;       // the kept row this sweep is recorded as (-1: none) of `rows`
    int32_t* z_tr;       // or null: [chains][N * rows], label (1-based) of row i at i * rows + row
    int32_t* nk_tr;      // [chains][rows * K]
    double* th_tr;       // [chains][rows * K * P], K x P column-major per row
    double* al_tr;       // [chains][rows]
};

__device__ __forceinline__ int ens_rl(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ double ens_rl(double v, int l) {
    const uint64_t u = dbits(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
    double r = dfrom(((uint64_t)hi << 32) | lo);
    asm volatile("" : "+v"(r));  // binary64 arithmetic is vector arithmetic: the pair need not stay scalar (ens_v)
    return r;
}
__device__ __forceinline__ int ens_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// A launch argument moved into a vector register where the kernel starts: the values read once a chunk, once a move or
// once a sweep -- pointers, priors, the seed -- would otherwise sit in scalar registers through the row loop, which has
// none to spare (the loop's own counters, masks and the row's words are scalar), and be spilled.
template <class V>
__device__ __forceinline__ V ens_v(V x) { asm volatile("" : "+v"(x)); return x; }

// The terms and constants of labels kA and kB (kB < 0: of kA alone) from the counts in LDS; nA, nB their sizes.
// Lanes 0..7 take the constants' logs (const_arg of bmm_spec.h under BUILD_SELF), one each; the (label, column, role)
// triples go round the lanes, one log_ each per pass.  cp, cm: updated on lanes kA and kB.
template <bool DP>
__device__ __forceinline__ void ens_build(int P, int Kc, double beta, double gamma, double* T, const int32_t* Sl, int lane,
                                          int kA, int nA, int kB, int nB, double ak, double ldN, double& cp, double& cm) {
    const double bg = beta + gamma;
    double v = 0.0;
    {
        const int n = lane < 4 ? nA : nB;
        const bool live = lane < 4 || (lane < 8 && kB >= 0);
        double arg = 1.0;
        bool need = false;
        switch (lane & 3) {
            case 0: arg = bg + (double)n; need = n > 0; break;
            case 1: arg = bg + (double)(n - 1); need = n > 1; break;
            case 2: arg = (double)n + ak; need = n > 0; break;
            default: arg = (double)(n - 1) + ak; need = n > 1; break;
        }
        need = need && live && lane < 8;
        v = need ? log_(arg) : 0.0;
    }
    const double denA_p = ens_rl(v, 0), denA_m = ens_rl(v, 1), denB_p = ens_rl(v, 4), denB_m = ens_rl(v, 5);
    {
        const double cpA = nA > 0 ? ens_rl(v, 2) - ldN : neg_inf(), cmA = nA > 1 ? ens_rl(v, 3) - ldN : neg_inf();
        const double cpB = nB > 0 ? ens_rl(v, 6) - ldN : neg_inf(), cmB = nB > 1 ? ens_rl(v, 7) - ldN : neg_inf();
        if (lane == kA) { cp = cpA; cm = cmA; }
        if (lane == kB) { cp = cpB; cm = cmB; }
    }
    const int per = 4 * P, total = kB >= 0 ? 2 * per : per;
    for (int idx = lane; idx < total; idx += 64) {
        const bool second = idx >= per;
        const int q = second ? idx - per : idx;
        const int d = q >> 2, role = q & 3;
        const int k = second ? kB : kA;
        const int64_t n = second ? nB : nA;
        const int64_t s = Sl[k * P + d];
        double arg;
        bool have;
        if (role == 0) { have = n > 0; arg = beta + (double)s; }
        else if (role == 1) { have = n > 0; arg = (gamma + (double)n) - (double)s; }
        else if (role == 2) { have = n > 1 && s >= 1; arg = beta + (double)(s - 1); }
        else { have = n > 1 && s <= n - 1; arg = (gamma + (double)(n - 1)) - (double)s; }
        const double raw = log_(have ? arg : 1.0);
        const double den = second ? (role < 2 ? denB_p : denB_m) : (role < 2 ? denA_p : denA_m);
        T[(d * 4 + role) * Kc + k] = have ? raw - den : 0.0;
    }
    __builtin_amdgcn_wave_barrier();
}

template <bool DP>
__global__ __launch_bounds__(kEnsWaves * 64) void k_ens_sweep(EnsArgs a) {
    extern __shared__ double ens_lds[];
    const int lane = threadIdx.x & 63;
    const int wv = ens_uniform((int)(threadIdx.x >> 6));
    const int c = blockIdx.x * a.cpw + wv;
    if (wv >= a.cpw || c >= a.chains) return;  // (a whole wave: nothing below waits for another wave)
    const int N = a.N, P = a.P, K = a.K, Kc = a.Kc;
    double* const T = reinterpret_cast<double*>(reinterpret_cast<char*>(ens_lds) + ens_v(wv * a.slice_bytes));
    double* const E = T + 4 * P * Kc;
    int32_t* const Sl = reinterpret_cast<int32_t*>(E + 256);
    int32_t* const zc = ens_v(a.z + (size_t)c * N);
    int32_t* const Sg = ens_v(a.S + (size_t)c * K * P);
    int32_t* const Nkg = ens_v(a.Nk + (size_t)c * K);
    double* const alg = ens_v(a.alpha + c);
    const uint32_t* const Xb = ens_v(a.Xb);
    const uint64_t seed = ens_v(a.seed + (uint64_t)c);
    const uint32_t sweep = ens_v(a.sweep);
    const double beta = ens_v(a.beta), gamma = ens_v(a.gamma), pa = ens_v(a.a), pb = ens_v(a.b);
    const int Nv = ens_v(N), sample_alpha = ens_v(a.sample_alpha), row = ens_v(a.row), rows_kept = ens_v(a.rows);
    const size_t slot = ens_v((size_t)c * a.rows + (a.row >= 0 ? a.row : 0));  // the chain's kept row among all
    int32_t* const z_tr = ens_v(a.z_tr && a.row >= 0 ? a.z_tr + (size_t)c * N * a.rows + (a.row >= 0 ? a.row : 0) : nullptr);
    int32_t* const nk_tr = ens_v(a.nk_tr);
    double* const th_tr = ens_v(a.th_tr);
    double* const al_tr = ens_v(a.al_tr);
    const int nw = (P + 31) >> 5;

    // stage: the exponential table, the counts, the sizes; the new cluster's zeros
    for (int j = lane; j < 256; j += 64) E[j] = exp256_table()[j];
    for (int j = lane; j < K * P; j += 64) Sl[j] = Sg[j];
    int nk = lane < K ? Nkg[lane] : 0;
    if (DP)
        for (int j = lane; j < 4 * P; j += 64) T[j * Kc + K] = 0.0;
    const double alpha = *alg;
    const double ak = DP ? 0.0 : div_(alpha, (double)K);
    const double ldN = log_((double)(Nv - 1) + alpha);
    double cp = neg_inf(), cm = neg_inf();
    __builtin_amdgcn_wave_barrier();
    for (int k = 0; k < K; k += 2) {
        const int kB = k + 1 < K ? k + 1 : -1;
        ens_build<DP>(P, Kc, beta, gamma, T, Sl, lane, k, ens_rl(nk, k), kB, kB >= 0 ? ens_rl(nk, kB) : 0, ak, ldN, cp, cm);
    }
    if (DP && lane == K) cp = (log_(alpha) - ldN) + (double)P * (log_(beta) - log_(beta + gamma));

    const bool cat = lane < Kc;
    const int hiv = ens_v(a.hi);
    for (int base = a.lo; base < a.hi; base += 64) {
        const int i_l = base + lane;
        const bool row_l = i_l < hiv;
        uint32_t xw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (row_l) xw[w] = Xb[(size_t)(w < nw ? w : nw - 1) * Nv + i_l];  // (a word past the last: the last again, not read)
        int zl = row_l ? zc[i_l] : -1;
        const double ul = row_l ? z_uniform(seed, (uint64_t)i_l, sweep) : 0.0;
        const int rows = a.hi - base < 64 ? a.hi - base : 64;
        for (int r = 0; r < rows; ++r) {
            const int zo = ens_rl(zl, r);
            const double u = ens_rl(ul, r);
            uint32_t xs[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) xs[w] = (uint32_t)ens_rl((int)xw[w], r);
            // ---- the scores
            const bool own = lane == zo;
            double acc = own ? cm : cp;
            {
                const int Wl = own ? kGroupWm : a.W;
                const double* const tb = T + (own ? 2 * Kc : 0) + (cat ? lane : 0);
                double t = 0.0;
                int cnt = 0;
                for (int w = 0; w < nw; ++w) {
                    const uint32_t word = xs[w];
                    const int nb = P - 32 * w < 32 ? P - 32 * w : 32;
                    for (int j = 0; j < nb; ++j) {
                        const int d = 32 * w + j;
                        const int bit = (int)((word >> j) & 1u);
                        const double e = cat ? tb[(d * 4 + 1 - bit) * Kc] : 0.0;
                        t = t + e;
                        ++cnt;
                        if (cnt == Wl || d == P - 1) { acc = acc + t; t = 0.0; cnt = 0; }
                    }
                }
            }
            const double score = cat ? acc : neg_inf();
            // ---- the draw: expw_(score - max), the running sum in label order, the count of t >= c_k
            double m = neg_inf();
            if (Kc <= 8) {
                for (int k = 0; k < Kc; ++k) { const double sk = ens_rl(score, k); m = sk > m ? sk : m; }
            } else {
                m = score;
                for (int o = 32; o > 0; o >>= 1) { const double ot = __shfl_xor(m, o); m = ot > m ? ot : m; }
                m = ens_rl(m, 0);
            }
            int pick = -1;
            if (m > neg_inf()) {
                const double wgt = expw_tab(score - m, E);
                double run = 0.0, cdf = 0.0;
                for (int k = 0; k < Kc; ++k) {
                    run = run + ens_rl(wgt, k);
                    cdf = lane == k ? run : cdf;
                }
                if (run > 0.0) {
                    const double t = u * run;
                    const int cnt = __popcll(__ballot(cat && t >= cdf));
                    pick = cnt < Kc ? cnt : -1;
                }
            }
            if (pick < 0) pick = zo >= 0 ? zo : 0;
            if (DP && pick == K) {  // a new cluster: the smallest free label, or the truncation rule (chain_batch)
                const unsigned long long used = __ballot(lane < K && nk > 0);
                const unsigned long long free_ = __ballot(lane < K && nk == 0);
                const int Kused = __popcll(used);
                const int new_label = free_ ? (int)__ffsll((long long)free_) - 1 : -1;
                const int own_single = zo >= 0 && ens_rl(nk, zo >= 0 ? zo : 0) == 1 ? 1 : 0;
                if (Kused - own_single < K - 1) {
                    pick = new_label;
                    if (own_single && (pick < 0 || zo < pick)) pick = zo;
                } else {
                    const int sz = nk - (own ? 1 : 0);
                    int key = lane < K && sz > 0 ? (sz << 8) | lane : 0x7fffffff;
                    for (int o = 32; o > 0; o >>= 1) { const int ot = __shfl_xor(key, o); key = ot < key ? ot : key; }
                    key = ens_rl(key, 0);
                    pick = key != 0x7fffffff ? key & 255 : (zo >= 0 ? zo : 0);
                }
            }
            pick = ens_uniform(pick);
            // ---- a move: the counts of the two labels, then their terms
            if (pick != zo) {
                for (int d = lane; d < P; d += 64) {
                    const int j = d >> 6;  // 0 or 1
                    const uint32_t word = lane < 32 ? (j ? xs[2] : xs[0]) : (j ? xs[3] : xs[1]);
                    const int bit = (int)((word >> (lane & 31)) & 1u);
                    if (zo >= 0) Sl[zo * P + d] -= bit;
                    Sl[pick * P + d] += bit;
                }
                nk += lane == pick ? 1 : 0;
                nk -= lane == zo ? 1 : 0;
                zl = lane == r ? pick : zl;
                __builtin_amdgcn_wave_barrier();
                const int kB = zo >= 0 ? zo : -1;  // (a row of the DP's first sweep leaves no label)
                ens_build<DP>(P, Kc, beta, gamma, T, Sl, lane, pick, ens_rl(nk, pick), kB, kB >= 0 ? ens_rl(nk, kB) : 0, ak, ldN, cp, cm);
            }
        }
        if (row_l) {
            zc[i_l] = zl;
            int32_t* const zt = ens_v(z_tr);  // (its test: made here, not kept as a mask through the loop)
            if (zt) zt[(size_t)i_l * rows_kept] = zl + 1;
        }
    }

    // ---- the state goes back; the last launch of a sweep ends it
    __builtin_amdgcn_wave_barrier();
    const int Kv = ens_v(K), KPv = ens_v(K * P);  // (vector copies: the masks below are not kept through the loop above)
    for (int j = lane; j < KPv; j += 64) Sg[j] = Sl[j];
    if (lane < Kv) Nkg[lane] = nk;
    if (a.hi < N) return;
    double al = alpha;
    if (sample_alpha) {
        const int Ka = DP ? __popcll(__ballot(lane < Kv && nk > 0)) : K;
        al = update_alpha_wave(alpha, pa, pb, (double)Nv, Ka, seed, sweep, lane);
        al = ens_rl(al, 0);
        if (lane == 0) *alg = al;
    }
    if (row >= 0) {
        if (lane == 0) al_tr[slot] = al;
        if (lane < Kv) nk_tr[slot * Kv + lane] = nk;
        double* const th = th_tr + slot * KPv;
        for (int base = 0; base < K * P; base += 64) {  // (the whole wave takes every trip: __shfl below)
            const int j = base + lane;
            const int k = j < KPv ? j % K : 0, d = j < KPv ? j / K : 0;
            const int n = __shfl(nk, k);
            if (j < KPv) th[j] = DP && n == 0 ? 0.0 : div_((double)Sl[k * P + d], (double)n);
        }
    }
}

// ---- k_ens_score: the stored state of every chain scored after a kept sweep ----
// The posterior predictive of new rows (LOO = false, BUILD_PREDICT) or the leave-one-out predictive of the fitted rows
// (LOO = true, BUILD_LOO) of the state the sweep left, folded into the chain's own accumulators: what k_state_tables and
// k_score do for one chain, for every chain of the ensemble in one launch.  Placement is k_ens_sweep's -- a wave per
// chain, cpw chains a workgroup, the same slice of LDS (ens_slice_bytes), no barrier between waves -- but the work is
// turned round:
//   the build              every category's constants on its own lane (the kRuleLogs logs of const_arg, one log_ per lane
//                          and pass; cat_consts), then the (column, role, category) terms round the lanes, one log_ each
//                          per pass, into T[(d * 4 + role) * Kc + k]: term_arg, term_of against the category's
//                          denominator, fetched from its lane.  Roles 2, 3 are built for LOO only
//   rows on lanes          lane l owns row base + l: its plane words, its label.  Nothing here is sequential.  The lane
//                          walks the categories and the columns; a category's constant is a v_readlane of a uniform
//                          index, a column's term is read from one of two addresses chosen by the row's bit, so a read
//                          is a broadcast of at most two words
//   the order of a score   k_score's: a group's terms added from 0.0 in ascending column order (group_entry), the constant
//                          added to group 0's sum as write_group_tables folds it in, the groups added from 0.0 in group
//                          order.  The own label's plain score counts -inf, exactly 0 after expw; its minus-self score,
//                          in groups of kGroupWm, is one more category, summed last
//   two passes             the maximum first, then expw_tab(score - max) summed in category order: a score is computed
//                          twice, the same additions in the same order, and no lane keeps Kc scores (an array indexed by a
//                          run-time category would be a private segment)
//   the fold               predict_fold / loo_fold on the chain's accumulators in global memory, a lane per row, no atomics
struct EnsFoldArgs {
    const uint32_t* Xb;  // bit planes of the scored rows: word w of row i at Xb[w * R + i]
    int R;               // scored rows: N (LOO) or the M new rows
    int N, P, K, Kc, W;  // the chains' shape, as EnsArgs
    int chains, cpw;
    int slice_bytes;
    double beta, gamma;
    const int32_t* z;     // [chains][N] (LOO)
    const int32_t* Nk;    // [chains][K]
    const int32_t* S;     // [chains][K * P]
    const double* alpha;  // [chains]: after the sweep's update
    double* acc;          // [chains][kLooAcc][N] (LOO) or [chains][2][M]: run_max, run_sum
    int n;                // states folded before this one
    double* trace;        // or null: [chains][rows][R]
    int row, rows;        // the kept row this state is recorded as, of `rows`
};

template <bool DP, bool LOO>
__global__ __launch_bounds__(kEnsWaves * 64) void k_ens_score(EnsFoldArgs a) {
    extern __shared__ double ens_lds[];
    const int lane = threadIdx.x & 63;
    const int wv = ens_uniform((int)(threadIdx.x >> 6));
    const int c = blockIdx.x * a.cpw + wv;
    if (wv >= a.cpw || c >= a.chains) return;  // (a whole wave: nothing below waits for another wave)
    const int N = a.N, P = a.P, K = a.K, Kc = a.Kc, R = a.R;
    double* const T = reinterpret_cast<double*>(reinterpret_cast<char*>(ens_lds) + wv * a.slice_bytes);
    double* const E = T + 4 * P * Kc;
    int32_t* const Sl = reinterpret_cast<int32_t*>(E + 256);
    const int32_t* const Sg = a.S + (size_t)c * K * P;
    const int nw = (P + 31) >> 5;

    // stage: the exponential table, the counts, the sizes
    for (int j = lane; j < 256; j += 64) E[j] = exp256_table()[j];
    for (int j = lane; j < K * P; j += 64) Sl[j] = Sg[j];
    const int nk = lane < K ? a.Nk[(size_t)c * K + lane] : 0;
    const CountRule r{LOO ? BUILD_LOO : BUILD_PREDICT, DP, K, (int64_t)N, a.beta, a.gamma, a.alpha[c]};
    // the constants of category `lane`
    double cp, cm, den_p, den_m;
    {
        const double ak = rule_ak(r);
        double v[kRuleLogs];
#pragma unroll
        for (int j = 0; j < kRuleLogs; ++j) {
            double arg;
            const bool need = const_arg(r, ak, lane, nk, j, arg) && (j == 4 || lane < Kc);
            const double raw = log_(need ? arg : 1.0);
            v[j] = need ? raw : 0.0;
        }
        const CatConsts cc = cat_consts(r, lane, nk, v);
        cp = cc.cp; cm = cc.cm; den_p = cc.den_p; den_m = cc.den_m;
    }
    __builtin_amdgcn_wave_barrier();
    // the terms: (column, role) by category, a category's neighbours on neighbouring lanes
    {
        constexpr int kRoles = LOO ? 4 : 2;
        const int total = P * kRoles * Kc;
        for (int base = 0; base < total; base += 64) {  // (the whole wave takes every trip: __shfl below)
            const int idx = base + lane;
            const bool in = idx < total;
            const int q = in ? idx / Kc : 0;
            const int k = in ? idx - q * Kc : 0;
            const int d = q / kRoles, role = q % kRoles;
            const int64_t n = __shfl(nk, k);
            const double dp_ = __shfl(den_p, k), dm_ = __shfl(den_m, k);
            const int64_t s = k < K ? Sl[k * P + d] : 0;
            double arg;
            const bool have = term_arg(r, k, role, n, s, arg);
            const double raw = log_(have ? arg : 1.0);
            if (in) T[(d * 4 + role) * Kc + k] = term_of(have, raw, term_den(role) ? dm_ : dp_);
        }
    }
    __builtin_amdgcn_wave_barrier();

    const int32_t* const zc = a.z + (size_t)c * N;
    double* const accc = a.acc + (size_t)c * (LOO ? kLooAcc : 2) * R;
    double* const tr = a.trace ? a.trace + ((size_t)c * a.rows + a.row) * R : nullptr;
    const int W = a.W;
    for (int base = 0; base < R; base += 64) {
        const int i = base + lane;
        const bool valid = i < R;
        const int ic = valid ? i : R - 1;
        uint32_t xw[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) xw[w] = a.Xb[(size_t)(w < nw ? w : nw - 1) * R + ic];  // (a word past the last: the last again, not read)
        const int z = LOO ? zc[ic] : -1;
        const bool seated = !LOO || (unsigned)z < (unsigned)K;
        // the row's own label from the minus-self terms, in groups of kGroupWm
        double ownv = neg_inf();
        if (LOO) {
            const int zs = seated ? z : 0;
            const double cmz = __shfl(cm, zs);
            const double* const tb = T + 2 * Kc + zs;
            double own = 0.0, t = 0.0;
            int cnt = 0;
            bool first = true;
            for (int w = 0; w < nw; ++w) {
                const uint32_t word = xw[w];
                const int nb = P - 32 * w < 32 ? P - 32 * w : 32;
                for (int j = 0; j < nb; ++j) {
                    const int d = 32 * w + j;
                    const int bit = (int)((word >> j) & 1u);
                    t = t + tb[(d * 4 + 1 - bit) * Kc];
                    ++cnt;
                    if (cnt == kGroupWm || d == P - 1) { own = own + (first ? cmz + t : t); t = 0.0; cnt = 0; first = false; }
                }
            }
            ownv = seated ? own : neg_inf();
        }
        // category k's plain score of this lane's row; k uniform
        auto score = [&](int k) -> double {
            const double ck = ens_rl(cp, k);
            const double* const tb = T + k;
            double acc = 0.0, t = 0.0;
            int cnt = 0;
            bool first = true;
            for (int w = 0; w < nw; ++w) {
                const uint32_t word = xw[w];
                const int nb = P - 32 * w < 32 ? P - 32 * w : 32;
                for (int j = 0; j < nb; ++j) {
                    const int d = 32 * w + j;
                    const int bit = (int)((word >> j) & 1u);
                    t = t + tb[(d * 4 + 1 - bit) * Kc];
                    ++cnt;
                    if (cnt == W || d == P - 1) { acc = acc + (first ? ck + t : t); t = 0.0; cnt = 0; first = false; }
                }
            }
            return LOO && k == z ? neg_inf() : acc;
        };
        double mx = ownv;
        for (int k = 0; k < Kc; ++k) mx = __builtin_fmax(mx, score(k));
        double tot = 0.0;
        for (int k = 0; k < Kc; ++k) tot = tot + expw_tab(score(k) - mx, E);
        if (LOO) tot = tot + expw_tab(ownv - mx, E);
        const double ld = seated ? mx + log_(tot) : qnan();
        if (valid) {
            if (tr) tr[i] = ld;
            ScoreArgs sa{};
            sa.rows = R;
            sa.n = a.n;
            if (LOO) {
                // A vector copy of the pointer.  With the scalar pair, AMD clang 22.0.0git (ROCm 7.2.0) dies compiling the LOO
                // instantiations: a segmentation fault in the greedy register allocator (VirtRegAuxInfo::isRematerializable,
                // from calculateSpillWeightsAndHints).  A toolchain that compiles `sa.acc = accc` no longer needs this
                sa.acc = ens_v(accc);
                loo_fold(sa, i, ld, E);
            } else {
                sa.run_max = accc;
                sa.run_sum = accc + R;
                predict_fold(sa, i, ld, E);
            }
        }
    }
}

}  // namespace bmm
