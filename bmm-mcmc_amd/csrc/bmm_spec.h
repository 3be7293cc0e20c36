// bmm_spec.h -- the numerics of the allocation path, written once for host and device.
//
// Everything the categorical draw of z_n depends on is defined here with IEEE-754
// binary64 add / mul / fma / div / sqrt / floor and integer bit operations only, in a
// fixed order, so that a gfx950 wave and an x86 core produce the same bits (the build
// passes -ffp-contract=off to both compilers; every fused operation is an explicit
// bmm::fma_). No libm transcendental is called: log/exp are implemented below.
// tests/test_gpu_math.py checks device-vs-host bit equality of every function here;
// oracle/bmm_oracle.c restates the same arithmetic independently in plain C.
//
// Reference arithmetic being restated (all /root/reference):
//   collapsed conditional   src/collapsed_gibbs.cpp:99-137
//   DP conditional          src/collapsed_gibbs_dp.cpp:71,102-106,140-186
//   stick-breaking z-step   src/stickbreaking.cpp:75-105
//   alpha update            src/utils.cpp:6-14
// The reference draws through R's Mersenne-Twister (rmultinom / rbeta / rgamma); this
// build draws through Philox (counter-based, Salmon et al. 2011): Philox2x32-10 for the one
// uniform per observation and sweep that decides z_n, Philox4x32-10 for the parameter variates;
// see DESIGN.md.
#pragma once
#include <stdint.h>

#include "bmm_exp256.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BMM_HD __host__ __device__ __forceinline__
#else
#define BMM_HD inline
#endif

namespace bmm {

// ---------------------------------------------------------------- constants
// Features per lookup group.  The tables against the full statistics use groups of kGroupW features
// (32-entry tables: 20 % fewer lookups and adds per observation than groups of four) whenever the table
// image of the shape fits in the 160 KiB of LDS that way, and groups of kGroupWAlt otherwise
// (group_width_for: a pure function of sampler, K and P, part of the arithmetic because it fixes the order
// of the sums).  The own-cluster ("minus self") tables are read once per observation, not once per
// category, so they use narrow groups (small tables) throughout.
constexpr int kGroupW = 5;
constexpr int kGroupWAlt = 4;
constexpr int kGroupWm = 3;
constexpr int kGroupMm = 1 << kGroupWm;
constexpr int kOwnSub = 6;  // the own-cluster tables are padded with zero groups to a multiple of this

// Philox stream ids (counter word 3)
enum : uint32_t {
    kStreamZ = 0,        // (reserved: the per-observation uniform is Philox2x32 under its own key, z_uniform)
    kStreamStickA = 1,   // v_k ~ Beta: first gamma;  c0 = k, c1 = block counter, c2 = sweep
    kStreamStickB = 2,   // v_k ~ Beta: second gamma
    kStreamThetaA = 3,   // theta_kd ~ Beta: first gamma; c0 = k*P+d
    kStreamThetaB = 4,
    kStreamAlphaEta = 5, // eta ~ Beta(alpha+1, N): first gamma (c0 = 0), second gamma (c0 = 1)
    kStreamAlphaG1 = 6,  // Gamma(a+K)
    kStreamAlphaG2 = 7,  // Gamma(a+K-1)
    kStreamSplitMerge = 8,  // a split-merge move: c0 = move index, c1 = block counter, c2 = sweep (sm_move_draws)
    kStreamFeatureSelect = 9,  // the inclusion indicator of feature d after sweep j: c0 = d, c1 = block counter, c2 = j (fs_uniform)
    kStreamInit = 10,    // the pick of centre j of the k-modes++ start: c0 = j, c1 = block counter, c2 = 0 (init_uniform)
    kStreamAlloc = 11,     // an eject / absorb move: c0 = move index, c1 = block counter, c2 = sweep (ea_move_draws)
    kStreamAllocPeA = 12,  // its p_E ~ Beta(e, e): first gamma; c0 = move index, c2 = sweep
    kStreamAllocPeB = 13,  // ... second gamma
    kStreamTemper = 14,    // the uniform of a replica exchange: c0 = pair index r, c1 = block counter, c2 = exchange point t (temper_uniform)
    kStreamMissing = 15,   // the uniform of missing cell (i, j) behind sweep t: c0, c1 = the low and high word of i * P + j, c2 = t (na_uniform; t = 0: the starting fill)
    kStreamMissingA = 16,  // phi_kj ~ Beta of the imputation step of a counting chain: first gamma; c0 = k*P+j, c1 = block counter, c2 = sweep (na_phi)
    kStreamMissingB = 17,  // ... second gamma
    kStreamAllocSplit = 18,  // a split-merge move of the allocation chain: c0 = move index, c1 = block counter, c2 = sweep (as_move_draws)
};

// ---------------------------------------------------------------- bit helpers
BMM_HD uint64_t dbits(double x) {
    union { double d; uint64_t u; } c; c.d = x; return c.u;
}
BMM_HD double dfrom(uint64_t u) {
    union { double d; uint64_t u; } c; c.u = u; return c.d;
}
BMM_HD double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
BMM_HD double floor_(double a) { return __builtin_floor(a); }
// IEEE correctly-rounded on both sides (checked bitwise on the GPU by test_gpu_math).
BMM_HD double div_(double a, double b) { return a / b; }
BMM_HD double sqrt_(double a) { return __builtin_sqrt(a); }

BMM_HD double neg_inf() { return dfrom(0xfff0000000000000ull); }
BMM_HD double pos_inf() { return dfrom(0x7ff0000000000000ull); }
BMM_HD double qnan() { return dfrom(0x7ff8000000000000ull); }

// ---------------------------------------------------------------- Philox4x32-10
struct U4 { uint32_t x, y, z, w; };

BMM_HD uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

BMM_HD U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = mulhi32(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = mulhi32(M1, c2), lo1 = M1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += W0; k1 += W1;
    }
    U4 o; o.x = c0; o.y = c1; o.z = c2; o.w = c3; return o;
}

// Philox2x32-10: one 32x32->64 multiply per round; two output words = the one uniform a
// categorical draw needs (a 4x32 block would throw half of its four multiplies per round away).
BMM_HD void philox2x32_10(uint32_t c0, uint32_t c1, uint32_t k, uint32_t& o0, uint32_t& o1) {
    const uint32_t M = 0xD256D193u, W = 0x9E3779B9u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t pr = (uint64_t)M * (uint64_t)c0;
        c0 = (uint32_t)(pr >> 32) ^ k ^ c1;
        c1 = (uint32_t)pr;
        k += W;
    }
    o0 = c0; o1 = c1;
}

// 52-bit uniform in [0,1): the words fill the mantissa of a double in [1,2), minus 1 (no
// integer-to-double conversions).  Its largest value is 1 - 2^-52, and u * t < t then holds in
// binary64 for every finite t > 0, so an inverse-CDF walk against t = u * total always ends inside.
BMM_HD double u52(uint32_t a, uint32_t b) {
    const uint32_t hi = 0x3ff00000u | (a >> 12);
    const uint32_t lo = (a << 20) | (b >> 12);
    return dfrom(((uint64_t)hi << 32) | lo) - 1.0;
}

// 53-bit uniform in [0,1) from two 32-bit words (parameter variates).
BMM_HD double u01(uint32_t a, uint32_t b) {
    const double hi = (double)(a >> 5), lo = (double)(b >> 6);
    return (hi * 67108864.0 + lo) * 1.1102230246251565404e-16;  // 2^-53
}
// uniform in (0,1]: 1 - u01
BMM_HD double u01_open0(uint32_t a, uint32_t b) { return 1.0 - u01(a, b); }

// A counted stream of Philox blocks: (c0, block counter, c2, stream id) under one key.
struct Stream {
    uint32_t c0, ctr, c2, sid, k0, k1;
    BMM_HD U4 next() { U4 r = philox4x32_10(c0, ctr, c2, sid, k0, k1); ++ctr; return r; }
};
BMM_HD Stream make_stream(uint64_t seed, uint32_t c0, uint32_t c2, uint32_t sid) {
    Stream s; s.c0 = c0; s.ctr = 0; s.c2 = c2; s.sid = sid;
    s.k0 = (uint32_t)seed; s.k1 = (uint32_t)(seed >> 32); return s;
}

// The uniform that decides z_i in sweep j: Philox2x32-10 at counter (i mod 2^32, sweep) under a
// 32-bit key folded from the 64-bit seed (and from the high word of i, zero below 2^32 observations).
BMM_HD uint32_t z_key(uint64_t seed, uint64_t i) {
    const uint32_t h = (uint32_t)(i >> 32);
    return ((uint32_t)seed ^ ((uint32_t)(seed >> 32) * 0x85EBCA6Bu)) ^ ((h << 16) | (h >> 16));
}
BMM_HD double z_uniform(uint64_t seed, uint64_t i, uint32_t sweep) {
    uint32_t a, b;
    philox2x32_10((uint32_t)i, sweep, z_key(seed, i), a, b);
    return u52(a, b);
}

// The draws of split-merge move number `move` ahead of sweep `sweep` (include/bmm_mcmc.h "split-merge"), a pure
// function of (seed, sweep, move): two Philox4x32 blocks of a stream of their own.  Block 0: the anchors, row i
// uniform over N and row j uniform over the other N - 1; block 1: the uniform of the accept step and a 32-bit salt.
// The members' uniforms are Philox2x32 at counter (row mod 2^32, 2^31 + scan) under the salt (with the high word of
// the row folded in as z_key does): the sweeps' own uniforms have a counter word 1 below 2^31 (the sweep index), so
// no (key, counter) pair of theirs is ever reused, whatever the salt.  Scan 0 is the launch state.
struct SmDraws { int64_t i, j; double u; uint32_t salt; };
BMM_HD SmDraws sm_move_draws(uint64_t seed, uint32_t sweep, uint32_t move, int64_t N) {
    Stream st = make_stream(seed, move, sweep, kStreamSplitMerge);
    const U4 r0 = st.next(), r1 = st.next();
    SmDraws d;
    d.i = (int64_t)(u01(r0.x, r0.y) * (double)N);
    d.i = d.i > N - 1 ? N - 1 : d.i;
    int64_t j = (int64_t)(u01(r0.z, r0.w) * (double)(N - 1));
    j = j > N - 2 ? N - 2 : j;
    d.j = j >= d.i ? j + 1 : j;
    d.u = u01_open0(r1.x, r1.y);
    d.salt = r1.z;
    return d;
}
BMM_HD double sm_member_uniform(uint32_t salt, uint64_t i, uint32_t scan) {
    const uint32_t h = (uint32_t)(i >> 32);
    uint32_t a, b;
    philox2x32_10((uint32_t)i, 0x80000000u | scan, salt ^ ((h << 16) | (h >> 16)), a, b);
    return u52(a, b);
}

// The uniform that decides the inclusion indicator of feature d behind sweep `sweep` (include/bmm_mcmc.h "feature
// selection"): the first block of a stream of its own, so it shares no (key, counter) pair with any other draw.
BMM_HD double fs_uniform(uint64_t seed, uint32_t d, uint32_t sweep) {
    Stream st = make_stream(seed, d, sweep, kStreamFeatureSelect);
    const U4 r = st.next();
    return u01(r.x, r.y);
}

// The uniform that picks centre j of the k-modes++ initial allocation (include/bmm_mcmc.h "initial allocation"): the
// first block of a stream of its own, so it shares no (key, counter) pair with any other draw.
BMM_HD double init_uniform(uint64_t seed, uint32_t j) {
    Stream st = make_stream(seed, j, 0, kStreamInit);
    const U4 r = st.next();
    return u01(r.x, r.y);
}

// The uniform that decides missing cell `cell` = i * P + j behind sweep `sweep` (include/bmm_mcmc.h "missing data"; sweep
// 0 is the starting fill): one Philox block under a stream id of its own, keyed by the cell's identity and the sweep and
// by nothing else -- not the grid, not the order of the cell list.  Counter word 1 carries the high word of the cell
// where the counted streams carry their block counter; the stream id is in no other use, so no (key, counter) pair is shared.
BMM_HD double na_uniform(uint64_t seed, uint64_t cell, uint32_t sweep) {
    const U4 r = philox4x32_10((uint32_t)cell, (uint32_t)(cell >> 32), sweep, kStreamMissing, (uint32_t)seed, (uint32_t)(seed >> 32));
    return u01(r.x, r.y);
}
// the valid bits of word w of a row of P features (every word but the last one is full)
BMM_HD uint32_t init_word_mask(int P, int w) {
    const int rest = P - 32 * w;
    return rest >= 32 ? 0xffffffffu : ((1u << rest) - 1u);
}

// ---------------------------------------------------------------- log / exp
// log(x): argument reduced to m in [sqrt(1/2), sqrt(2)), f = m-1, s = f/(2+f),
// log(1+f) = f - f^2/2 + s*(f^2/2 + R(s^2)), R an even minimax polynomial of degree 14
// (coefficients: the classic Remez set for this reduction). Error < 1 ulp.
BMM_HD double log_(double x) {
    uint64_t ix = dbits(x);
    if (x == 0.0) return neg_inf();
    if ((int64_t)ix < 0) return qnan();
    if ((ix >> 52) == 0x7ffull) return x;  // +inf, nan
    int e = 0;
    if ((ix >> 52) == 0) {  // subnormal: scale by 2^54
        x = x * 18014398509481984.0; ix = dbits(x); e = -54;
    }
    e += (int)(ix >> 52) - 1023;
    uint64_t m = (ix & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    if (m >= 0x3ff6a09e667f3bcdull) { m -= 0x0010000000000000ull; e += 1; }
    const double f = dfrom(m) - 1.0;
    const double s = div_(f, 2.0 + f);
    const double z = s * s, w = z * z;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01,
                 Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                 Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    const double t1 = w * fma_(w, fma_(w, Lg6, Lg4), Lg2);
    const double t2 = z * fma_(w, fma_(w, fma_(w, Lg7, Lg5), Lg3), Lg1);
    const double R = t2 + t1;
    const double hfsq = 0.5 * f * f;
    const double dk = (double)e;
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
}

// exp(x) = 2^k * 2^(j/64) * e^r with 64k + j = round(x * 64/ln2), r = x - (64k+j) ln2/64
// (two-part), |r| <= ln2/128: e^r - 1 by a degree-5 Taylor polynomial (truncation < 2^-54),
// 2^(j/64) from a 64-entry table of correctly rounded doubles (tools/gen_exp_table.py).
// Error < 1 ulp.  Results below 2^-1021 are flushed to 0 (x < -708); the sampler never needs them.
#define BMM_EXP2_64_TABLE \
    0x1.0000000000000p+0, 0x1.02c9a3e778061p+0, 0x1.059b0d3158574p+0, 0x1.0874518759bc8p+0, \
    0x1.0b5586cf9890fp+0, 0x1.0e3ec32d3d1a2p+0, 0x1.11301d0125b51p+0, 0x1.1429aaea92de0p+0, \
    0x1.172b83c7d517bp+0, 0x1.1a35beb6fcb75p+0, 0x1.1d4873168b9aap+0, 0x1.2063b88628cd6p+0, \
    0x1.2387a6e756238p+0, 0x1.26b4565e27cddp+0, 0x1.29e9df51fdee1p+0, 0x1.2d285a6e4030bp+0, \
    0x1.306fe0a31b715p+0, 0x1.33c08b26416ffp+0, 0x1.371a7373aa9cbp+0, 0x1.3a7db34e59ff7p+0, \
    0x1.3dea64c123422p+0, 0x1.4160a21f72e2ap+0, 0x1.44e086061892dp+0, 0x1.486a2b5c13cd0p+0, \
    0x1.4bfdad5362a27p+0, 0x1.4f9b2769d2ca7p+0, 0x1.5342b569d4f82p+0, 0x1.56f4736b527dap+0, \
    0x1.5ab07dd485429p+0, 0x1.5e76f15ad2148p+0, 0x1.6247eb03a5585p+0, 0x1.6623882552225p+0, \
    0x1.6a09e667f3bcdp+0, 0x1.6dfb23c651a2fp+0, 0x1.71f75e8ec5f74p+0, 0x1.75feb564267c9p+0, \
    0x1.7a11473eb0187p+0, 0x1.7e2f336cf4e62p+0, 0x1.82589994cce13p+0, 0x1.868d99b4492edp+0, \
    0x1.8ace5422aa0dbp+0, 0x1.8f1ae99157736p+0, 0x1.93737b0cdc5e5p+0, 0x1.97d829fde4e50p+0, \
    0x1.9c49182a3f090p+0, 0x1.a0c667b5de565p+0, 0x1.a5503b23e255dp+0, 0x1.a9e6b5579fdbfp+0, \
    0x1.ae89f995ad3adp+0, 0x1.b33a2b84f15fbp+0, 0x1.b7f76f2fb5e47p+0, 0x1.bcc1e904bc1d2p+0, \
    0x1.c199bdd85529cp+0, 0x1.c67f12e57d14bp+0, 0x1.cb720dcef9069p+0, 0x1.d072d4a07897cp+0, \
    0x1.d5818dcfba487p+0, 0x1.da9e603db3285p+0, 0x1.dfc97337b9b5fp+0, 0x1.e502ee78b3ff6p+0, \
    0x1.ea4afa2a490dap+0, 0x1.efa1bee615a27p+0, 0x1.f50765b6e4540p+0, 0x1.fa7c1819e90d8p+0,
static const double kExp2Host[64] = {BMM_EXP2_64_TABLE};
#if defined(__HIPCC__)
__constant__ double kExp2Dev[64] = {BMM_EXP2_64_TABLE};
#endif
BMM_HD const double* exp2_table() {
#if defined(__HIP_DEVICE_COMPILE__)
    return kExp2Dev;
#else
    return kExp2Host;
#endif
}

// core for an argument already known to be in [-708, 709.79]; Tab is any pointer-like to the table
template <class Tab>
BMM_HD double exp_core(double xs, Tab T, int& k_out) {
    const double kd = floor_(fma_(xs, 9.23324826168936567e+01, 0.5));   // 64/ln2
    double r = fma_(-kd, 1.08304246962491454e-02, xs);                   // ln2/64, high part
    r = fma_(-kd, 3.62351064663484299e-19, r);                           // low part
    const int ki = (int)kd;
    const int j = ki & 63;
    k_out = ki >> 6;
    double c = fma_(r, 8.3333333333333332177e-03, 4.1666666666666664354e-02);  // 1/120, 1/24
    c = fma_(r, c, 1.6666666666666665741e-01);                                  // 1/6
    c = fma_(r, c, 0.5);
    const double q = fma_(r * r, c, r);
    const double t = T[j];
    return fma_(t, q, t);
}

template <class Tab>
BMM_HD double exp_tab(double x, Tab T) {
    // written select-style (no early returns) so that the device code is branch-free
    const bool is_nan = x != x;
    const bool over = x > 709.782712893384;
    const bool under = x < -708.0;
    const double xs = (is_nan || over || under) ? 0.0 : x;
    int k;
    double p = exp_core(xs, T, k);
    const bool top = k > 1023;
    p = top ? p * 2.0 : p;
    k = top ? k - 1 : k;
    const double y = p * dfrom((uint64_t)(k + 1023) << 52);
    return is_nan ? x : (over ? pos_inf() : (under ? 0.0 : y));
}
BMM_HD double exp_(double x) { return exp_tab(x, exp2_table()); }

// The weight exponential of the draw: expw_(x) for x <= 0 (max-shifted scores; -inf and NaN
// arguments give exactly 0).  256 k + j = round-to-nearest-even(x * 256/ln2) by the 1.5 * 2^52
// trick (the integer is read from the low word of the sum: no floor, no conversion),
// r = x - (256 k + j) ln2/256 in two parts, |r| <= ln2/512: e^r - 1 by a degree-4 polynomial
// (truncation < 2^-54), 2^(j/256) from a 256-entry table of correctly rounded doubles
// (bmm_exp256.h), the scale 2^k by ldexp.  Arguments below -745.2 underflow to 0 through ldexp's
// own IEEE rounding; nothing is flushed by a comparison.  Error < 1 ulp in the normal range.
static const double kExp256Host[256] = {BMM_EXP2_256_TABLE};
#if defined(__HIPCC__)
__constant__ double kExp256Dev[256] = {BMM_EXP2_256_TABLE};
#endif
BMM_HD const double* exp256_table() {
#if defined(__HIP_DEVICE_COMPILE__)
    return kExp256Dev;
#else
    return kExp256Host;
#endif
}
BMM_HD double ldexp_(double p, int k) { return __builtin_ldexp(p, k); }
template <class Tab>
BMM_HD double expw_tab(double x, Tab T) {
    const double xs = __builtin_fmax(x, -1000.0);                        // NaN -> -1000
    const double km = fma_(xs, 0x1.71547652b82fep+8, 6755399441055744.0);  // 256/ln2, 1.5 * 2^52
    const int32_t ki = (int32_t)(uint32_t)dbits(km);
    const double kd = km - 6755399441055744.0;
    double r = fma_(-kd, 0x1.62e42fefa39efp-9, xs);                       // ln2/256, high part
    r = fma_(-kd, 0x1.abc9e3b39803fp-64, r);                             // low part
    const int j = ki & 255;
    const int k = ki >> 8;
    double c = fma_(r, 4.1666666666666664354e-02, 1.6666666666666665741e-01);  // 1/24, 1/6
    c = fma_(r, c, 0.5);
    const double q = fma_(r * r, c, r);
    const double t = T[j];
    return ldexp_(fma_(t, q, t), k);
}
BMM_HD double expw_(double x) { return expw_tab(x, exp256_table()); }

// The exchange of parallel tempering (include/bmm_mcmc.h "parallel tempering"): the uniform that decides pair r
// (rungs r and r + 1) at exchange point t is the first block of a stream of its own under the ladder's seed; with
// d = (b_r - b_{r+1}) * (L_{r+1} - L_r) the exchange is accepted iff d >= 0 or u < expw_(d); a NaN d rejects.
BMM_HD double temper_uniform(uint64_t seed, uint32_t r, uint32_t t) {
    Stream st = make_stream(seed, r, t, kStreamTemper);
    const U4 x = st.next();
    return u52(x.x, x.y);
}
BMM_HD double temper_log_ratio(double b_r, double b_r1, double L_r, double L_r1) { return (b_r - b_r1) * (L_r1 - L_r); }
BMM_HD bool temper_accepts(double d, double u) { return d >= 0.0 || (d < 0.0 && u < expw_(d)); }

// ---------------------------------------------------------------- lgamma
// log Gamma(x) for x > 0 (the split-merge move's arguments: a prior plus an integer, up to about 1e7).  The
// argument is shifted up to y >= 8 by the recurrence, Gamma(x) = Gamma(y) / (x (x+1) ... (y-1)) with the product
// (at most eight factors, below 4e5) in binary64, then Stirling's series in 1/y with eight Bernoulli terms (the
// first one left out is 43867/(244188 y^17) < 8e-17 at y = 8) on log_.  Absolute error a few 1e-16 * max(1, |result|);
// near the zeros at x = 1 and x = 2 the result is small and the error is not (tests/test_split_merge_ref.py
// records the largest error found, in ulps of max(1, |result|)).
BMM_HD double lgamma_(double x) {
    double prod = 1.0, y = x;
    while (y < 8.0) { prod = prod * y; y = y + 1.0; }
    const double r = div_(1.0, y), r2 = r * r;
    double s = fma_(r2, -2.9550653594771241e-02, 6.4102564102564100e-03);   // -3617/122400, 1/156
    s = fma_(r2, s, -1.9175269175269176e-03);                                // -691/360360
    s = fma_(r2, s, 8.4175084175084171e-04);                                 // 1/1188
    s = fma_(r2, s, -5.9523809523809529e-04);                                // -1/1680
    s = fma_(r2, s, 7.9365079365079365e-04);                                 // 1/1260
    s = fma_(r2, s, -2.7777777777777779e-03);                                // -1/360
    s = fma_(r2, s, 8.3333333333333329e-02);                                 // 1/12
    const double stirling = (((y - 0.5) * log_(y) - y) + 9.1893853320467278e-01) + r * s;  // log(2 pi)/2
    return stirling - log_(prod);
}

// ---------------------------------------------------------------- the draw, decided in binary32 where that is safe
// The draw of z_n is ONE integer: cnt = #{k : u * tot >= cdf_k}, cdf_k the binary64 running sum of
// expw_(score_k - m) in label order, tot = cdf_K (the definition; draw_spec below).  draw_tier1 computes the same
// count from binary32 weights and says whether that count is PROVEN equal to the definition's: it is whenever
// u~ * tot~ stays further than kTier1Eps * tot~ from every binary32 CDF entry.  A caller that gets `false` runs the
// definition; so the two tiers together are exact, not approximate.
//
// Why kTier1Eps = 2^-16 suffices, for up to kTier1MaxCats = 64 categories.  Both tiers start from the same binary64
// d_k = score_k - m <= 0 (0 for the maximum, so the exact total T = sum_k e^(d_k) is >= 1).  Write h = 2^-24 (half an
// ulp of binary32).  Against the exact e^(d_k), partial sums C_k and u * T, tier 1 is off by at most, in units of T:
//   narrowing d_k to binary32, the binary32 constant log2(e) and their rounded product: the argument of exp2 is
//     d_k log2(e) (1 + delta), |delta| <= 3.01 h, which moves the weight w_k by w_k ln(1/w_k) |delta|; summed,
//     sum_k w_k ln(1/w_k) = T (H(w / T) - ln T) <= T ln K (H the entropy, <= ln K)      <= 3.01 ln(64) h = 12.6 h
//   the hardware exp2 (v_exp_f32: 1 ulp = 2 h of each weight, the ISA's documented bound; results below 2^-126
//     are flushed to 0, an absolute 2^-126 each)                                          <=  2.0 h
//   the binary32 running sum: K - 1 additions, each within h of a partial sum <= T          <= 63.0 h
//   u narrowed to binary32 (h) and the rounded product u~ * tot~ (h)                        <=  2.0 h
//   second-order terms of all of the above ((1 + 63 h)^2 and the like)                      <   0.1 h
// and the definition itself by its own rounding: expw_ < 1 ulp of binary64, 63 binary64 additions and one product,
// < 2^-45.  The difference t - cdf_k that either tier takes the sign of therefore differs between the tiers by
// less than E * T with E = 79.7 h + 2^-45 < 2^-17.6 = 4.8e-6, and tot~ >= T (1 - E).  The test is
// |t~ - c~_k| > 2^-16 tot~ >= 2^-16 (1 - E) T > 3.2 E T: the sign cannot differ, with a factor three to spare.  Equal
// consecutive CDF entries (categories of weight zero) and u = 0 need no case of their own: a tie t~ = c~_k is
// never "further than", and a non-tie is decided by the same bound.  A lane whose scores hold a NaN or whose
// maximum is not finite gets NaN into tot~ (the running sum carries it to the end) or fails the test on m: never
// certain.  exp2 is a parameter so that the host test can run the function with the exponential pushed to either
// end of its documented error.
constexpr float kTier1Eps = 0x1p-16f;
constexpr int kTier1MaxCats = 64;
struct Exp2Fast {
    BMM_HD float operator()(float x) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_amdgcn_exp2f(x);  // v_exp_f32
#else
        return __builtin_exp2f(x);
#endif
    }
};
// sc[0..KT): the scores (the own-cluster substitution done), m their maximum, u the draw's uniform.  Returns
// whether cnt is proven to be the definition's count.
template <int KT, class Exp2 = Exp2Fast>
BMM_HD bool draw_tier1(const double (&sc)[KT], double m, double u, float eps, int& cnt, Exp2 ex2 = Exp2()) {
    static_assert(KT <= kTier1MaxCats, "kTier1Eps is derived for at most kTier1MaxCats categories");
    float c[KT];
    float run = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < KT; ++k) {
        const float d = (float)(sc[k] - m);
        run = run + ex2(d * 0x1.715476p+0f);  // log2(e)
        c[k] = run;
    }
    const float t = (float)u * run;
    float nearest = __builtin_inff();
    int n = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < KT; ++k) {
        const float diff = t - c[k];
        n += diff >= 0.0f ? 1 : 0;
        nearest = __builtin_fminf(nearest, __builtin_fabsf(diff));  // (a NaN here is a NaN in `run` too)
    }
    cnt = n;
    return nearest > eps * run && m > neg_inf() && m < pos_inf();  // false when `run` is NaN
}
// The definition, for the host: the count the draw is.  (The kernels carry it inline, around their emitting
// and lane-sharing forms.)
template <int KT>
BMM_HD int draw_spec(const double (&sc)[KT], double m, double u) {
    double cdf[KT];
    double run = 0.0;
    for (int k = 0; k < KT; ++k) { run = run + expw_(sc[k] - m); cdf[k] = run; }
    const double t = u * run;
    int n = 0;
    for (int k = 0; k < KT; ++k) n += t >= cdf[k] ? 1 : 0;
    return n;
}

// ---------------------------------------------------------------- the draw from scores summed in binary32
// The packed tier (k_resample_pk): the scores themselves come from binary32 copies of the table entries, two categories
// to a 64-bit lookup, summed in binary32 in group order; the own-cluster score the same way from a binary32 image of
// its own (Tm32: the "observation removed" terms grouped at the shape's width, each binary64 entry narrowed once).
// draw_pk takes those scores s~_k and their maximum m~ and is draw_tier1 from there on, with a band that also covers
// what the scores lost.  As there, `true` means the count is PROVEN to be the definition's.
//
// The band, per lane: kPkEpsUnit * (80 + (G + 2) (|m~| + ln 64 + 1)) * tot~, G the number of lookup groups.  With
// h = 2^-24 and s_k, m, d_k = s_k - m <= 0, w_k = e^(d_k), T = sum w_k >= 1 the exact quantities of the definition:
//   every table entry is <= 0 (a log of a probability; the constant term log(n_k + alpha/K) - log(N - 1 + alpha) of a
//     category that is not the observation's own has n_k <= N - 1), so the partial sums of a score only grow in
//     magnitude and every one of them is <= |s_k|.  An entry narrowed to binary32 is within h of itself, each of the
//     G - 1 binary32 additions within h of a partial sum: |s~_k - s_k| <= G h |s_k| (1 + G h).  (The host test pushes
//     every narrowed entry a further ulp = 2 h: (G + 2) h |s_k|, which is why the band says G + 2.)
//   the own score is summed like every other, from narrowed entries in group order, and its entries are <= 0 too: the
//     constant is log(n_k - 1 + alpha/K) - log(N - 1 + alpha) (or -inf for a cluster of one row), each term
//     log(beta + s - 1) - log(beta + gamma + n - 1) or its x = 0 twin log(gamma + n - 1 - s) - log(beta + gamma + n - 1),
//     with s - 1 <= n - 1 and s >= 0.  So |s~_k - s'_k| <= G h |s'_k| (1 + G h), s'_k the exact sum of the width-W
//     entries.  The definition's own score s_k sums the same P terms and the constant grouped three at a time (Gm
//     groups) where the tier's entries group them W at a time, each entry a binary64 sum of at most W terms: the two
//     differ by the binary64 roundings of at most P + G + Gm additions of partial sums no larger than |s_k|,
//     |s'_k - s_k| <= (P + G + Gm) 2^-53 |s_k| < 2^-45 |s_k| for P <= 128 -- 2^-21 of one h |s_k|, well inside the
//     two h |s_k| that G + 2 carries beyond the summation's G.  A -inf entry (it sits in group 0 of both images, with
//     the constant) narrows to -inf and makes both sums -inf: the category weighs exactly 0 on both sides.
//   a shift common to all categories cancels in the sign of t - cdf_k, so m~ need not be m: tier and definition are
//     compared on the weights e^(s_k - m~), which are the w_k times one common factor.  The argument of exp2 is
//     (s~_k - m~) log2(e) (1 + delta), |delta| <= 3.01 h as in draw_tier1 (the subtraction's rounding in place of the
//     narrowing there), so the weight of category k is off by the factor e^x, |x| <= (G + 2) h |s_k| + 3.01 h |d_k|,
//     |x| < 6e-3 for G <= 26 and scores down to -3000 -- deeper than the resident kernels' shapes reach: P <= 128
//     feature terms of at least log(beta / (beta + gamma + N)) each, about -22 at N = 1e9 with the default priors --
//     so e^x - 1 <= 1.003 |x|.  With |s_k| = |m| + |d_k| and sum_k w_k |d_k| = T (H(w / T) - ln T) <= T ln K, the
//     weights together are off by at most 1.003 h ((G + 2)(|m| + ln K) + 3.01 ln K) T
//   exp2 itself (2 h), the binary32 running sum ((K - 1) h), u narrowed and the product (2 h), second order (0.1 h)
//     and the definition's own rounding (2^-45): as in draw_tier1, 67.1 h + 2^-45 for K <= 64.
// In all E <= h (79.7 + 1.003 (G + 2)(|m| + ln 64)) + 2^-45 in units of T (E < 6e-3 over that range), and
// |m~| >= |m| (1 - G h); the band is 3.2 h (80 + (G + 2)(|m~| + ln 64 + 1)) tot~ with tot~ >= T (1 - E), more than
// three times E T.  (Beyond -3000 the factor 1.003 grows with |s|, and the margin of three still covers it to 1e5.)  Ties, u = 0, NaN
// and a maximum that is not finite: as in draw_tier1 (never certain).  Impossible categories (-inf, the padding
// included) weigh exactly 0 on both sides.
constexpr float kPkEpsUnit = 3.2f * 0x1p-24f;
constexpr float kPkLnCats = 4.1588831f;  // ln kTier1MaxCats
BMM_HD float pk_band(float m, int G, float unit) {
    return unit * (80.0f + (float)(G + 2) * (__builtin_fabsf(m) + kPkLnCats + 1.0f));
}
// sc[0..KT): the binary32 scores (own-cluster substitution done), m their maximum, u the draw's uniform, G the lookup
// groups each score is the sum of, unit = kPkEpsUnit (0: no band, for the tests that show what the band is for).
template <int KT, class Exp2 = Exp2Fast>
BMM_HD bool draw_pk(const float (&sc)[KT], float m, double u, int G, float unit, int& cnt, Exp2 ex2 = Exp2()) {
    static_assert(KT <= kTier1MaxCats, "the band is derived for at most kTier1MaxCats categories");
    float c[KT];
    float run = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < KT; ++k) {
        run = run + ex2((sc[k] - m) * 0x1.715476p+0f);  // log2(e); -inf - -inf = NaN stays in `run`
        c[k] = run;
    }
    const float t = (float)u * run;
    float nearest = __builtin_inff();
    int n = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < KT; ++k) {
        const float diff = t - c[k];
        n += diff >= 0.0f ? 1 : 0;
        nearest = __builtin_fminf(nearest, __builtin_fabsf(diff));
    }
    cnt = n;
    return nearest > pk_band(m, G, unit) * run && m > -__builtin_inff() && m < __builtin_inff();  // false when `run` is NaN
}

// ---------------------------------------------------------------- the draw from the binary32 entries, summed in binary64
// The middle tier (k_resample_pk, for the lanes draw_pk leaves uncertain): the same binary32 entries the packed loop
// reads -- Tq for every category, Tm32 for the observation's own label, padding groups included -- each widened to
// binary64 and added in binary64, then the definition's own steps on those scores: the maximum m^, d_k = s^_k - m^,
// expw_, a binary64 running sum in label order, t = u c^_K and the count.  What is left of the packed tier's error is
// what the entries themselves lost when they were narrowed; the summation, the exponential and the running sum no
// longer add to it.  As for draw_pk, `true` means the count is PROVEN to be the definition's.
//
// The band, per observation: kMidEpsUnit * (kMidC0 + 2 (|m^| + ln 64 + 1)) * c^_K.  With h = 2^-24 and s_k, m,
// d_k = s_k - m <= 0, w_k = e^(d_k), T = sum w_k >= 1 the definition's quantities, as in draw_pk's derivation:
//   an entry narrowed to binary32 is within half an ulp of itself, at most h relative; the host test pushes every
//     narrowed entry a further whole ulp, at most 2 h relative (an ulp of binary32 is between h and 2 h of the value).
//     Entries are <= 0, so sum |entry| = |s_k|: the exact sum of the entries is within h |s_k| of s_k as the kernel
//     has them and within 3 h |s_k| as the test pushes them.  The band is sized for the pushed ones.
//   the binary64 sum of G widened entries, in any order: each addition within 2^-53 of a partial sum no larger than
//     |s_k|, at most G 2^-53 |s_k|.  The own score: the entries group the terms W at a time where the definition
//     groups them three at a time, a further (P + G + Gm) 2^-53 |s_k| < 2^-45 |s_k| (draw_pk).  Together
//     |s^_k - s_k| <= (3 h + 2^-44) |s_k| < 3.0001 h |s_k|.
//   a shift common to all categories cancels in the sign of t - cdf_k, so m^ need not be m.  The weight of category k
//     is off by the factor e^x, |x| <= 3.0001 h |s_k| + 2^-52 |d_k| (the subtraction's rounding) < 4e-4 down to scores
//     of -2000, so e^x - 1 <= 1.0002 |x|.  With |s_k| = |m| + |d_k| and sum_k w_k |d_k| <= T ln K the weights together
//     are off by at most 3.001 h (|m| + ln 64) T.
//   expw_ (< 2^-52 of each weight), the running sum (K - 1 binary64 additions, or ceil(log2 K) levels of a log-step
//     scan where the kernel takes one: at most 63 * 2^-53 either way), the product u c^_K (2^-53) and the definition's
//     own rounding (2^-45): together < 2^-44 = 2^-20 h.
// In all E <= h (3.001 (|m| + ln 64) + 2^-20) in units of T, |m^| >= |m| (1 - 3.0001 h) and c^_K >= T (1 - E).  With
// kMidEpsUnit = 4.8 h and kMidC0 = 1 the band is 4.8 h (1 + 2 (|m^| + ln 64 + 1)) c^_K > 3.19 E T: the packed band's
// factor of more than three, against entries an ulp further off than the kernel ever has them (against the kernel's
// own h per entry the factor is above nine).  Next to the packed band at C5 (G = 20, |m| about 60):
// 4.8 (1 + 2 * 65.2) / (3.2 (80 + 22 * 65.2)) = 0.13.
// Ties and categories of weight zero are never "further than"; a NaN among the scores, a maximum that is not finite
// (+inf, or every category impossible) and a NaN total are never certain: draw_tier1's rules.
constexpr double kMidEpsUnit = 4.8 * 0x1p-24;
constexpr double kMidC0 = 1.0;
constexpr double kMidLnCats = 4.1588830833596715;  // ln kTier1MaxCats
BMM_HD double mid_band(double m, double unit) {
    return unit * (kMidC0 + 2.0 * (__builtin_fabs(m) + kMidLnCats + 1.0));
}
// e[g][k]: the binary32 entry of group g < G for category k (the own label's column from Tm32), u the draw's uniform,
// unit = kMidEpsUnit (0: no band, for the tests that show what the band is for).
template <int KT, int GMAX>
BMM_HD bool draw_mid(const float (&e)[GMAX][KT], int G, double u, double unit, int& cnt) {
    static_assert(KT <= kTier1MaxCats, "the band is derived for at most kTier1MaxCats categories");
    double sc[KT], c[KT];
    double m = neg_inf();
    bool nan = false;
    for (int k = 0; k < KT; ++k) {
        double a = 0.0;
        for (int g = 0; g < G; ++g) a = a + (double)e[g][k];
        sc[k] = a;
        nan = nan || a != a;
        m = __builtin_fmax(m, a);
    }
    double run = 0.0;
    for (int k = 0; k < KT; ++k) { run = run + expw_(sc[k] - m); c[k] = run; }
    const double t = u * run;
    const double band = mid_band(m, unit) * run;
    bool clear = true;
    int n = 0;
    for (int k = 0; k < KT; ++k) {
        n += t >= c[k] ? 1 : 0;
        clear = clear && __builtin_fabs(t - c[k]) > band;  // false for a NaN
    }
    cnt = n;
    return clear && !nan && m > neg_inf() && m < pos_inf();
}

// ---------------------------------------------------------------- variates
// Standard normal by the Marsaglia polar method (log and sqrt only).
BMM_HD double rnorm_(Stream& st) {
    for (;;) {
        const U4 r = st.next();
        const double v1 = 2.0 * u01(r.x, r.y) - 1.0, v2 = 2.0 * u01(r.z, r.w) - 1.0;
        const double s = v1 * v1 + v2 * v2;
        if (s < 1.0 && s > 0.0) return v1 * sqrt_(div_(-2.0 * log_(s), s));
    }
}

// Gamma(shape, scale 1), Marsaglia & Tsang (2000); shape < 1 by the u^(1/shape) boost.  The boost flushes to 0 once
// log(u) / shape < -708 (exp_), so a small shape returns exactly 0 where the variate is below the binary64 range, as
// R's rgamma does (about half the draws at shape 1e-3, one in 2000 at 1e-2).  LOGGED = true is the same draw from the
// same Philox blocks that returns, in place of such a 0, the variate's logarithm log(d v) + log(u) / shape: below
// -690 wherever the product flushed, -inf for a shape that is not positive, so any value <= 0 is a logarithm and any
// value > 0 the variate itself, with the bits rgamma_ gives it (rbeta_join_ below reads the two apart).
template <bool LOGGED>
BMM_HD double rgamma_draw_(double shape, Stream& st) {
    if (!(shape > 0.0)) return LOGGED ? neg_inf() : 0.0;  // R::rgamma(0, .) is 0
    double boost = 1.0, lboost = 0.0;
    if (shape < 1.0) {
        const U4 r = st.next();
        lboost = div_(log_(u01_open0(r.x, r.y)), shape);
        boost = exp_(lboost);
        shape = shape + 1.0;
    }
    const double d = shape - 0.33333333333333331483;
    const double c = div_(1.0, sqrt_(9.0 * d));
    for (;;) {
        const double x = rnorm_(st);
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        const U4 r = st.next();
        const double u = u01_open0(r.x, r.y);
        const double x2 = x * x;
        if (log_(u) < 0.5 * x2 + d - d * v + d * log_(v)) {
            const double g = d * v * boost;
            if (LOGGED && !(g > 0.0)) return log_(d * v) + lboost;
            return g;
        }
    }
}
BMM_HD double rgamma_(double shape, Stream& st) { return rgamma_draw_<false>(shape, st); }

// Beta(p, q) = X / (X + Y) from two logged gamma draws (rgamma_draw_<true>; the halves may come from different
// threads).  Where neither gamma flushed to 0 this is the plain quotient.  Where one did -- p or q below 0.052 -- the
// quotient would be 0/0 (both), or exactly 0 or 1 although the flushed variate may be the larger part of the sum (one:
// a boost just below e^-708 against one just above it); the same two variates are then compared through their
// logarithms lx, ly (log_ of a variate that did not flush): X / (X + Y) = 1 / (1 + exp(ly - lx)), the same random
// variable continued below the binary64 range, so the law stays Beta(p, q).  Nearly all of its mass is then beyond
// e^-37 of 0 or 1 and the result rounds to what the quotient gave.  Two logarithms of -inf (p and q below 2.5e-307,
// where log(u) / p overflows) leave nothing to compare: 1/2.  Never NaN, always in [0, 1], for every p, q > 0.
BMM_HD double rbeta_join_(double xs, double ys) {
    if (xs > 0.0 && ys > 0.0) return div_(xs, xs + ys);
    const double lx = xs > 0.0 ? log_(xs) : xs, ly = ys > 0.0 ? log_(ys) : ys;
    const double t = ly - lx;
    if (t != t) return 0.5;
    return div_(1.0, 1.0 + exp_(t));
}
// X ~ Gamma(p), Y ~ Gamma(q) on two separate streams.
BMM_HD double rbeta_(double p, double q, Stream& sa, Stream& sb) {
    const double xs = rgamma_draw_<true>(p, sa), ys = rgamma_draw_<true>(q, sb);
    return rbeta_join_(xs, ys);
}

// The auxiliary rate of label k and feature j in the imputation step of a counting chain behind sweep `sweep`
// (include/bmm_mcmc.h "missing data"): phi ~ Beta(beta + s, gamma + n - s) from the observed-only counts -- n of the
// label's rows have the feature observed, s of them hold a 1; n = 0 is the prior.  kj = k * P + j.
BMM_HD double na_phi(uint64_t seed, double beta, double gamma, uint32_t kj, uint32_t sweep, int64_t s, int64_t n) {
    Stream sa = make_stream(seed, kj, sweep, kStreamMissingA);
    Stream sb = make_stream(seed, kj, sweep, kStreamMissingB);
    return rbeta_(beta + (double)s, (gamma + (double)n) - (double)s, sa, sb);
}

// The draws of eject / absorb move number `move` ahead of sweep `sweep` (include/bmm_mcmc.h "allocation sampler"), a
// pure function of (seed, sweep, move) and of the chain's K and maxK: three Philox4x32 blocks of a stream of their own.
// Block 0: the kind (eject iff u < pe_K; pe_1 = 1, pe_maxK = 0, 1/2 otherwise) and j1 uniform over the K labels;
// block 1: the uniform of the accept step and the 32-bit salt of the members' uniforms (sm_member_uniform at scan 0:
// a second counter word of 2^31); block 2: an absorb's j2, uniform over the other K - 1 labels.  An eject's j2 is K,
// the appended label, and its p_E ~ Beta(e, e) comes from two more streams (rbeta_); an absorb draws no p_E (NaN).
enum : int { kEaEject = 0, kEaAbsorb = 1 };
struct EaDraws { int kind, j1, j2; double u, pe; uint32_t salt; };
BMM_HD EaDraws ea_move_draws(uint64_t seed, uint32_t sweep, uint32_t move, int K, int maxK, double e) {
    Stream st = make_stream(seed, move, sweep, kStreamAlloc);
    const U4 r0 = st.next(), r1 = st.next(), r2 = st.next();
    EaDraws d;
    d.kind = K <= 1 ? kEaEject : (K >= maxK ? kEaAbsorb : (u01(r0.x, r0.y) < 0.5 ? kEaEject : kEaAbsorb));
    int j1 = (int)(u01(r0.z, r0.w) * (double)K);
    d.j1 = j1 > K - 1 ? K - 1 : j1;
    d.u = u01_open0(r1.x, r1.y);
    d.salt = r1.z;
    if (d.kind == kEaEject) {
        d.j2 = K;
        Stream sa = make_stream(seed, move, sweep, kStreamAllocPeA);
        Stream sb = make_stream(seed, move, sweep, kStreamAllocPeB);
        d.pe = rbeta_(e, e, sa, sb);
    } else {
        int t = (int)(u01(r2.x, r2.y) * (double)(K - 1));
        t = t > K - 2 ? K - 2 : t;
        d.j2 = t >= d.j1 ? t + 1 : t;
        d.pe = qnan();
    }
    return d;
}
// lbeta(x, y) and the closed-form log proposal density of an eject that leaves n1 rows and moves n2, p_E ~ Beta(e, e)
// integrated out: log q = lbeta(e + n1, e + n2) - lbeta(e, e).
BMM_HD double lbeta_(double x, double y) { return (lgamma_(x) + lgamma_(y)) - lgamma_(x + y); }
BMM_HD double ea_log_q(double e, int64_t n1, int64_t n2) {
    return lbeta_(e + (double)n1, e + (double)n2) - lbeta_(e, e);
}

// The draws of split-merge move number `move` of the allocation chain ahead of sweep `sweep` (include/bmm_mcmc.h
// "split-merge moves of the allocation sampler"): sm_move_draws on a stream of its own, so an armed chain's eject /
// absorb moves and these share no (key, counter) pair.  The members' uniforms are sm_member_uniform under the salt.
BMM_HD SmDraws as_move_draws(uint64_t seed, uint32_t sweep, uint32_t move, int64_t N) {
    Stream st = make_stream(seed, move, sweep, kStreamAllocSplit);
    const U4 r0 = st.next(), r1 = st.next();
    SmDraws d;
    d.i = (int64_t)(u01(r0.x, r0.y) * (double)N);
    d.i = d.i > N - 1 ? N - 1 : d.i;
    int64_t j = (int64_t)(u01(r0.z, r0.w) * (double)(N - 1));
    j = j > N - 2 ? N - 2 : j;
    d.j = j >= d.i ? j + 1 : j;
    d.u = u01_open0(r1.x, r1.y);
    d.salt = r1.z;
    return d;
}
// The prior part of that move's log ratio on the lumped state (K, partition), written once: host and device add in this
// order.  K is the number of open labels before the move, N the rows of the whole chain, lpk[k] = log p(K = k + 1).  A
// split takes a block of n rows into n0 and n1 at K -> K + 1; a merge of blocks n0 and n1 into n at K -> K - 1 is the
// exact negative of the split from K - 1.  log(Kl + 1) is the lumping factor (Kl + 1)! / (Kl - t)! over Kl! / (Kl - t)!.
BMM_HD double as_log_prior(int K, double N, double a, const double* lpk, int64_t n, int64_t n0, int64_t n1, bool split) {
    const int Kl = split ? K : K - 1;  // the smaller K
    const double ka = (double)Kl * a, kb = (double)(Kl + 1) * a;
    const double prior = ((((lpk[Kl] - lpk[Kl - 1]) + log_((double)(Kl + 1))) +
                           ((lgamma_(kb) - lgamma_(kb + N)) - (lgamma_(ka) - lgamma_(ka + N)))) +
                          ((lgamma_(a + (double)n0) + lgamma_(a + (double)n1)) - lgamma_(a + (double)n))) - lgamma_(a);
    return split ? prior : -prior;
}

// Escobar & West auxiliary-variable update of the concentration (utils.cpp:6-14).
BMM_HD double update_alpha_(double alpha_old, double a, double b, double N, int K,
                            uint64_t seed, uint32_t sweep) {
    Stream s0 = make_stream(seed, 0, sweep, kStreamAlphaEta);
    Stream s1 = make_stream(seed, 1, sweep, kStreamAlphaEta);
    const double eta = rbeta_(alpha_old + 1.0, N, s0, s1);
    const double b_eps = b - log_(eta);
    const double pi1 = a + (double)K - 1.0;
    const double pi2 = N * b_eps;
    const double pi = div_(pi1, pi1 + pi2);
    Stream g1 = make_stream(seed, 0, sweep, kStreamAlphaG1);
    Stream g2 = make_stream(seed, 0, sweep, kStreamAlphaG2);
    const double scale = div_(1.0, b_eps);
    const double ga = rgamma_(a + (double)K, g1) * scale;
    const double gb = rgamma_(a + (double)K - 1.0, g2) * scale;
    return pi * ga + (1.0 - pi) * gb;
}

// ---------------------------------------------------------------- conditional tables
// Per-feature log terms of the Beta-Bernoulli predictive of one cluster holding n
// observations with s1 of them 1 in this feature when the scored observation has x=1,
// s0 when it has x=0 (collapsed_gibbs.cpp:116-120; the "minus self" variant passes
// n-1, s-1 and s). `den` = log(beta+gamma+n) is hoisted by the caller.
BMM_HD double term_x1(double beta, int64_t s1, double den) { return log_(beta + (double)s1) - den; }
BMM_HD double term_x0(double gamma, int64_t n, int64_t s0, double den) {
    return log_((gamma + (double)n) - (double)s0) - den;
}

// One group-table entry: features [g*W, g*W+W) of one cluster under bit pattern m.
BMM_HD double group_entry(const double* e1, const double* e0, int g, int P, unsigned m, int W) {
    double t = 0.0;
    for (int j = 0; j < W; ++j) {
        const int d = g * W + j;
        if (d < P) t = t + (((m >> j) & 1u) ? e1[d] : e0[d]);
    }
    return t;
}

// ---------------------------------------------------------------- count-table rules
// The log terms of a counting chain's table image -- which category scores, the argument of each log_ and when it is
// needed -- for the three builds that call these functions: build_tables_self (BUILD_SELF) and
// k_state_tables (BUILD_PREDICT, BUILD_LOO).  A builder takes the raw log_ of every argument that is needed and
// subtracts the denominators afterwards (term_of, cat_consts).  The sweep's own launch, k_count_tables in its five
// flavours, is NOT among the callers: it keeps a body of its own (kernels.hip.h says why), and whoever changes a rule
// of the finite sweep changes it there and here.
//   BUILD_SELF     the finite sampler's z-step image as k_count_tables writes it: a label scores when it holds a row,
//                  the scored row's own label from the minus-self set when it holds another; denominator log(N - 1 + alpha)
//   BUILD_PREDICT  a new row against a stored state: no minus-self set, denominator log(N + alpha); the finite sampler's
//                  empty labels score at prior weight, the DP's are -inf (their terms are written all the same), the
//                  DP's new cluster, category K, is log(alpha) - log(N + alpha) with the prior terms as a per-feature table
//   BUILD_LOO      a fitted row against a stored state: BUILD_PREDICT over N - 1 rows plus the minus-self set of every
//                  label that holds a row (a row that sat alone: prior weight, finite; -inf, DP)
enum : int { BUILD_SELF = 0, BUILD_PREDICT = 1, BUILD_LOO = 2 };
struct CountRule {
    int build;     // BUILD_*
    bool dp;       // the CRP chain (stored-state builds only): a label weighs n, category K is the new cluster
    int K;         // labels
    int64_t N;     // fitted rows of the whole chain
    double beta, gamma, alpha;
};
BMM_HD bool rule_dp_new(const CountRule& r, int k) { return r.dp && k == r.K; }
BMM_HD int64_t rule_rows(const CountRule& r) { return r.build == BUILD_PREDICT ? r.N : r.N - 1; }
// category k of n rows has plain terms / a finite plain constant by its weight / minus-self terms / a minus-self constant
BMM_HD bool rule_scores(const CountRule& r, int k, int64_t n) {
    return r.build == BUILD_SELF ? k < r.K && n > 0 : k < r.K || rule_dp_new(r, k);
}
BMM_HD bool rule_weighs(const CountRule& r, int k, int64_t n) {
    return r.build == BUILD_SELF ? rule_scores(r, k, n) : k < r.K && (!r.dp || n > 0);
}
BMM_HD bool rule_minus(const CountRule& r, int k, int64_t n) {
    return r.build == BUILD_SELF ? k < r.K && n > 1 : r.build == BUILD_LOO && k < r.K && n >= 1;
}
BMM_HD bool rule_minus_weighs(const CountRule& r, int k, int64_t n) {
    return r.build == BUILD_LOO && r.dp ? k < r.K && n > 1 : rule_minus(r, k, n);
}

// The constants of category k holding n rows need up to kRuleLogs logs; log j has argument `arg` and is needed when
// this returns true (a log that is not needed counts 0).  ak: what a label's weight adds to its size, rule_ak, passed
// in so that a caller divides once.
//   0, 1  log(beta + gamma + n), ... with the scored row removed: the two denominators of the terms
//   2, 3  the label's weight log(n + ak), ... with the scored row removed
//   4     the denominator of the weights      5  log(alpha), the DP's new cluster
constexpr int kRuleLogs = 6;
BMM_HD double rule_ak(const CountRule& r) { return r.dp ? 0.0 : div_(r.alpha, (double)r.K); }
BMM_HD bool const_arg(const CountRule& r, double ak, int k, int64_t n, int j, double& arg) {
    const double bg = r.beta + r.gamma;
    switch (j) {
        case 0: arg = bg + (double)n; return rule_scores(r, k, n);
        case 1: arg = bg + (double)(n - 1); return rule_minus(r, k, n);
        case 2: arg = (double)n + ak; return rule_weighs(r, k, n);
        case 3: arg = (double)(n - 1) + ak; return rule_minus_weighs(r, k, n);
        case 4: arg = (double)rule_rows(r) + r.alpha; return true;
        case 5: arg = r.alpha; return rule_dp_new(r, k);
        default: arg = 1.0; return false;
    }
}
struct CatConsts { double cp, cm, den_p, den_m; };  // the constants of the plain and the minus-self set, the denominators
BMM_HD CatConsts cat_consts(const CountRule& r, int k, int64_t n, const double* v) {
    CatConsts c{neg_inf(), neg_inf(), v[0], v[1]};
    if (rule_weighs(r, k, n)) c.cp = v[2] - v[4];
    else if (rule_dp_new(r, k)) c.cp = v[5] - v[4];
    if (rule_minus_weighs(r, k, n)) c.cm = v[3] - v[4];
    return c;
}
// The term of a feature with s ones among the category's n rows, in role 0, 1 (x = 1, x = 0 against the full
// statistics: term_x1 / term_x0) or 2, 3 (the same with the scored row removed: it had x = 1, so s >= 1; x = 0, so
// s <= n - 1): the argument of its one log_, and whether the term exists.  term_den: which of the two denominators
// (logs 0 and 1 of const_arg) it is taken against.  term_of: the term from that raw log, 0 for one that does not exist.
BMM_HD bool term_arg(const CountRule& r, int k, int role, int64_t n, int64_t s, double& arg) {
    switch (role) {
        case 0: arg = r.beta + (double)s; return rule_scores(r, k, n);
        case 1: arg = (r.gamma + (double)n) - (double)s; return rule_scores(r, k, n);
        case 2: arg = r.beta + (double)(s - 1); return rule_minus(r, k, n) && s >= 1;
        default: arg = (r.gamma + (double)(n - 1)) - (double)s; return rule_minus(r, k, n) && s <= n - 1;
    }
}
BMM_HD int term_den(int role) { return role < 2 ? 0 : 1; }
BMM_HD double term_of(bool have, double raw, double den) { return have ? raw - den : 0.0; }

// Categorical features of the finite sweep (BUILD_SELF's conditions; k_count_tables<TAB_CAT>).
// A feature of L >= 2 levels is a block of L neighbouring one-hot columns under a symmetric Dirichlet(beta, ..., beta):
// a row has exactly one 1 in the block, so the predictive (beta + c_l) / (L beta + n) of its level is the block's
// whole factor, and it rides on the x = 1 term of that level's column.  For a column of such a block with s ones among
// the label's n rows:
//   roles 0, 2   log(beta + s) - log(L beta + n), log(beta + (s - 1)) - log(L beta + (n - 1)): the numerator's log is
//                that of a Bernoulli column (term_arg), the denominator the block's own (cat_den_arg) -- L beta is formed
//                as (double)L * beta and the count added to it
//   roles 1, 3   0: a level the row does not have says nothing more
// A term exists when the Bernoulli term of its role exists, role 2 when n > 1 && s >= 1.  The DP's new cluster takes the
// plain constant over the Bernoulli columns alone and then, block by block in ascending column order, cat_new_block
// (1 / L, the prior predictive of any level).  No block: the plain build, bit for bit.  The stored-state builds
// (BUILD_PREDICT, BUILD_LOO) and build_tables_self know the Bernoulli cell only: a categorical chain is offered neither.
BMM_HD bool cat_term_arg(const CountRule& r, int k, int role, int64_t n, int64_t s, double& arg) {
    if (role == 1 || role == 3) { arg = 1.0; return false; }
    return term_arg(r, k, role, n, s, arg);
}
BMM_HD bool cat_den_arg(const CountRule& r, int k, int L, int role, int64_t n, double& arg) {
    const double lbeta = (double)L * r.beta;
    arg = role < 2 ? lbeta + (double)n : lbeta + (double)(n - 1);
    return role < 2 ? rule_scores(r, k, n) : rule_minus(r, k, n);
}
BMM_HD double cat_new_block(double lb, double beta, int L) { return lb - log_((double)L * beta); }

// ---------------------------------------------------------------- log joint of a state
// log p(x, z, alpha, mask) of the state after a sweep from its folded counts (include/bmm_mcmc.h "log joint trace";
// DESIGN.md section 20): the pieces k_log_joint and k_log_joint_finish call, and log_joint_spec, the whole statement
// in their order for the host.  THE ORDER, a pure function of (K, P, mask):
//   a label's likelihood   kLjLanes partial sums, included feature d in partial d mod kLjLanes, ascending in d, each
//                          from 0; the partials folded by a binary tree (partial t takes partial t + o, o = kLjLanes/2
//                          .. 1); lgamma_(beta + gamma + n_k) once per label, subtracted per cell
//   the pooled term        (a mask only) the excluded features the same way, feature d against (N, T_d)
//   the totals             from 0, ascending in k: the likelihood of every label that holds a row, then the pooled term;
//                          the labels' prior terms the same way, then the model's head added to that sum
//   the row                {log_lik, log_prior, log_hyper, (log_lik + log_prior) + log_hyper}
constexpr int kLjLanes = 256;
enum : int { LJ_FINITE = 0, LJ_DP = 1, LJ_SB = 2, LJ_ALLOC = 3 };
struct LjModel {
    int kind;            // LJ_*: which prior on z (the collapsed and the full sampler share LJ_FINITE)
    int K;               // labels (K or maxK)
    int k_open;          // LJ_ALLOC: the open labels; else K
    int P;
    int64_t N;
    double beta, gamma;
    double alpha;        // the concentration after the sweep; LJ_ALLOC: a, the per-component parameter
    int sample_alpha;    // the chain samples alpha: its Gamma(a, b) prior enters log_hyper
    double a, b;
    double log_pk;       // LJ_ALLOC: log p(K = k_open)
    int masked;          // the chain has a feature mask: the pooled term and the mask's prior enter
    double rho;
    int p_in;            // included features (P without a mask)
};
BMM_HD bool lj_included(const uint32_t* mask, int d) { return !mask || ((mask[d >> 5] >> (d & 31)) & 1u); }
BMM_HD double lj_lb0(double beta, double gamma) { return (lgamma_(beta) + lgamma_(gamma)) - lgamma_(beta + gamma); }
// one cell: s ones among the n rows of a label (or T_d among all N); lgden = lgamma_(beta + gamma + n)
BMM_HD double lj_cell(double beta, double gamma, int64_t n, int64_t s, double lgden, double lb0) {
    return ((lgamma_(beta + (double)s) + lgamma_((gamma + (double)n) - (double)s)) - lgden) - lb0;
}
// whether label k of n rows enters the sums, and its prior term; n_after: the rows of the labels above k (LJ_SB)
BMM_HD bool lj_label_lik(const LjModel& m, int k, int64_t n) { return k < m.k_open && n > 0; }
BMM_HD bool lj_label_prior(const LjModel& m, int k, int64_t n) {
    return m.kind == LJ_SB ? k < m.K - 1 : lj_label_lik(m, k, n);
}
BMM_HD double lj_prior_term(const LjModel& m, int64_t n, int64_t n_after) {
    switch (m.kind) {
        case LJ_FINITE: { const double ak = div_(m.alpha, (double)m.K); return lgamma_(ak + (double)n) - lgamma_(ak); }
        case LJ_DP: return lgamma_((double)n);
        case LJ_SB: return lbeta_(1.0 + (double)n, m.alpha + (double)n_after) - lbeta_(1.0, m.alpha);
        default: return lgamma_(m.alpha + (double)n) - lgamma_(m.alpha);
    }
}
// the row from the per-label values: lik[k], prior[k] (read only where the label enters), nk[k], pooled (a mask only)
template <class NkOf>
BMM_HD void lj_finish(const LjModel& m, const double* lik, const double* prior, NkOf nk, double pooled, double out[4]) {
    double ll = 0.0, lp = 0.0;
    int used = 0;
    for (int k = 0; k < m.K; ++k) {
        const int64_t n = nk(k);
        if (lj_label_lik(m, k, n)) { ll = ll + lik[k]; ++used; }
        if (lj_label_prior(m, k, n)) lp = lp + prior[k];
    }
    if (m.masked) ll = ll + pooled;
    const double N = (double)m.N;
    if (m.kind == LJ_FINITE) lp = (lgamma_(m.alpha) - lgamma_(m.alpha + N)) + lp;
    else if (m.kind == LJ_DP) lp = ((double)used * log_(m.alpha) + lp) + (lgamma_(m.alpha) - lgamma_(m.alpha + N));
    else if (m.kind == LJ_ALLOC) {
        const double ka = (double)m.k_open * m.alpha;
        lp = (m.log_pk + (lgamma_(ka) - lgamma_(ka + N))) + lp;
    }
    double lh = 0.0;
    if (m.sample_alpha) lh = ((m.a * log_(m.b) - lgamma_(m.a)) + (m.a - 1.0) * log_(m.alpha)) - m.b * m.alpha;
    if (m.masked) lh = lh + ((double)m.p_in * log_(m.rho) + (double)(m.P - m.p_in) * log_(1.0 - m.rho));
    out[0] = ll; out[1] = lp; out[2] = lh; out[3] = (ll + lp) + lh;
}
// The whole statement for the host: Nk[K], S[K * P] (S[k * P + d]), mask words or null; scratch: 2 K doubles.
inline void log_joint_spec(const LjModel& m, const int32_t* Nk, const int32_t* S, const uint32_t* mask, double* scratch,
                           double out[4]) {
    const double lb0 = lj_lb0(m.beta, m.gamma), bg = m.beta + m.gamma;
    double* const lik = scratch;
    double* const prior = scratch + m.K;
    double part[kLjLanes];
    auto tree = [&part]() {
        for (int o = kLjLanes / 2; o > 0; o >>= 1)
            for (int t = 0; t < o; ++t) part[t] = part[t] + part[t + o];
        return part[0];
    };
    for (int k = 0; k < m.K; ++k) {
        const int64_t n = Nk[k];
        lik[k] = 0.0; prior[k] = 0.0;
        if (lj_label_lik(m, k, n)) {
            const double lgden = lgamma_(bg + (double)n);
            for (int t = 0; t < kLjLanes; ++t) part[t] = 0.0;
            for (int d = 0; d < m.P; ++d)
                if (lj_included(mask, d)) part[d % kLjLanes] = part[d % kLjLanes] + lj_cell(m.beta, m.gamma, n, S[(size_t)k * m.P + d], lgden, lb0);
            lik[k] = tree();
        }
        if (lj_label_prior(m, k, n)) {
            int64_t after = 0;
            for (int l = k + 1; l < m.K; ++l) after += Nk[l];
            prior[k] = lj_prior_term(m, n, after);
        }
    }
    double pooled = 0.0;
    if (m.masked) {
        const double lgden = lgamma_(bg + (double)m.N);
        for (int t = 0; t < kLjLanes; ++t) part[t] = 0.0;
        for (int d = 0; d < m.P; ++d) {
            if (lj_included(mask, d)) continue;
            int64_t T = 0;
            for (int k = 0; k < m.K; ++k) T += S[(size_t)k * m.P + d];
            part[d % kLjLanes] = part[d % kLjLanes] + lj_cell(m.beta, m.gamma, m.N, T, lgden, lb0);
        }
        pooled = tree();
    }
    lj_finish(m, lik, prior, [Nk](int k) { return (int64_t)Nk[k]; }, pooled, out);
}

// ---------------------------------------------------------------- pairwise local-dependence check of a state
// The bivariate residuals of a state (include/bmm_mcmc.h "pairwise local-dependence check").
// Given the labels and each label's margins the co-occurrence count c_k(d, e) is Hypergeometric(n_k, s_kd, s_ke);
// per pair the labels are taken in ascending order, labels of fewer than two rows skipped, and every integer below is
// formed in int64 and converted to binary64 once.  pc_label adds one label to the running sums; pc_z closes the pair.
// k_pc_stats and the host statement (pair_check_spec) call these and nothing else.
constexpr int kPcMaxM = 128;
struct PcSums {
    double A, V, X2;  // sum of (c - E), of the variances, of the per-label chi-squares
    int32_t df;       // labels with a positive variance
};
BMM_HD PcSums pc_zero() { PcSums s; s.A = 0.0; s.V = 0.0; s.X2 = 0.0; s.df = 0; return s; }
BMM_HD void pc_label(PcSums& t, int64_t c, int64_t n, int64_t sd, int64_t se) {
    if (n < 2) return;
    const int64_t num = c * n - sd * se, pd = sd * (n - sd), pe = se * (n - se), nn = n * n;
    const double a = div_((double)num, (double)n);
    const double v = div_((double)pd * (double)pe, (double)nn * (double)(n - 1));
    t.A = t.A + a;
    t.V = t.V + v;
    if (v > 0.0) { t.X2 = t.X2 + div_(a * a, v); t.df += 1; }
}
// Z of the pair, or NaN when no label has a positive variance
BMM_HD double pc_z(const PcSums& t) { return t.V > 0.0 ? div_(t.A, sqrt_(t.V)) : qnan(); }
// pairs (i < j) of positions in the feature list, numbered as numpy.triu_indices(M, 1) numbers them
BMM_HD int64_t pc_pair_index(int i, int j, int M) { return (int64_t)i * M - (int64_t)i * (i + 1) / 2 + (j - i - 1); }
BMM_HD int64_t pc_npairs(int M) { return (int64_t)M * (M - 1) / 2; }
BMM_HD void pc_pair_ij(int64_t q, int M, int& i, int& j) {
    int r = 0;
    while (q >= M - 1 - r) { q -= M - 1 - r; ++r; }
    i = r; j = r + 1 + (int)q;
}
// The whole statement for the host: cnt[Kc][npairs], nk[Kc], marg[Kc][M]; z, x2 [npairs] doubles, df [npairs] int32.
inline void pair_check_spec(int Kc, int M, const uint32_t* cnt, const uint32_t* nk, const uint32_t* marg, double* z,
                            double* x2, int32_t* df) {
    const int64_t np = pc_npairs(M);
    for (int64_t q = 0; q < np; ++q) {
        int i = 0, j = 0;
        pc_pair_ij(q, M, i, j);
        PcSums t = pc_zero();
        for (int k = 0; k < Kc; ++k)
            pc_label(t, (int64_t)cnt[(size_t)k * np + q], (int64_t)nk[k], (int64_t)marg[(size_t)k * M + i], (int64_t)marg[(size_t)k * M + j]);
        z[q] = pc_z(t); x2[q] = t.X2; df[q] = t.df;
    }
}

}  // namespace bmm
