// The own-cluster score of k_resample_pk on the host (bmm-mcmc_amd/csrc/bmm_spec.h, kernels.hip.h): the kernel sums it
// in binary32, in group order, from Tm32 -- the "observation removed" terms grouped at the SHAPE's width, the constant
// folded into group 0, each binary64 entry narrowed once -- where the definition sums the width-3 entries of Tm in
// binary64.  The other scores come from Tq as before, and draw_pk decides.  Whenever draw_pk says "certain" its count
// must be draw_spec's on the definition's binary64 scores.
//
// Tables are built with the count-table rules of bmm_spec.h (BUILD_SELF: const_arg, cat_consts, term_arg, term_of,
// group_entry) at both group widths:
//   C5's generator at steady state (K = 20, P = 100, N = 1e7, statistics N_k theta);
//   adversarial counts: clusters of one and of two rows, features with s = 0 and with s = n, N up to 1e9, at
//   P = 1, 37, 100 and 128 and 4, 8 and 20 labels.
// Every observation is scored with the narrowed entries as they are, an ulp up, an ulp down and alternately; uniforms
// walk one 2^-52 step at a time around every CDF boundary, sit around the band's edge, at random, at 0 and 1 - 2^-52.
// Also: every entry of both own images is <= 0 (or -inf), and the share of C5's observations that come back uncertain
// is at most 0.5 % (200 000 observations; printed, `pk_check` of the parent commit measured 0.058 %).
//
//   own32_check          all of the above
//   own32_check quick    a tenth of the observations (the run under the sanitizers)
//
// Prints "ok" and exits 0, or lists the first failures and exits 1.  Counters go to stderr.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bmm_spec.h"

namespace {

struct Rng {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double unit() { return (double)(next() >> 11) * 0x1p-53; }
    double u52() { return (double)(next() >> 12) * 0x1p-52; }
};

// a narrowed table entry, pushed: 0 as narrowed, 1 an ulp up, 2 an ulp down, 3 alternately (by its bits)
float narrow(double t, int push) {
    float q = (float)t;
    if (!(q == q) || std::isinf(q) || push == 0) return q;
    uint32_t b;
    __builtin_memcpy(&b, &q, 4);
    const int dir = push == 1 ? 1 : push == 2 ? -1 : (((b * 2654435761u) >> 31) ? 1 : -1);
    return std::nextafterf(q, dir > 0 ? INFINITY : -INFINITY);
}

struct Tally {
    long long draws = 0, certain = 0, wrong = 0, positive = 0;
    int reported = 0;
} T;

// The images of one allocation, as k_count_tables writes them: Tp [G][K][M] and the own image To [G][K][M] at the
// shape's width W (binary64 here; the kernel's Tq and Tm32 are these narrowed), Tm [GmPad][K][8] at kGroupWm.
struct Images {
    int K, P, W, G, M, Gm, GmPad;
    std::vector<double> Tp, To, Tm;
    void build(int K_, int P_, int W_, const std::vector<long long>& n, const std::vector<long long>& s, long long N, double alpha,
               double beta, double gamma) {
        K = K_; P = P_; W = W_;
        M = 1 << W;
        G = (P + W - 1) / W;
        Gm = (P + bmm::kGroupWm - 1) / bmm::kGroupWm;
        GmPad = (Gm + bmm::kOwnSub - 1) / bmm::kOwnSub * bmm::kOwnSub;
        Tp.assign((size_t)G * K * M, 0.0);
        To.assign((size_t)G * K * M, 0.0);
        Tm.assign((size_t)GmPad * K * bmm::kGroupMm, 0.0);
        const bmm::CountRule r{bmm::BUILD_SELF, false, K, N, beta, gamma, alpha};
        const double ak = bmm::rule_ak(r);
        std::vector<double> t[4];
        for (auto& v : t) v.assign(P, 0.0);
        for (int k = 0; k < K; ++k) {
            double v[bmm::kRuleLogs];
            for (int j = 0; j < bmm::kRuleLogs; ++j) {
                double arg;
                v[j] = bmm::const_arg(r, ak, k, n[k], j, arg) ? bmm::log_(arg) : 0.0;
            }
            const bmm::CatConsts cc = bmm::cat_consts(r, k, n[k], v);
            for (int role = 0; role < 4; ++role)
                for (int d = 0; d < P; ++d) {
                    double arg;
                    const bool have = bmm::term_arg(r, k, role, n[k], s[(size_t)k * P + d], arg);
                    t[role][d] = bmm::term_of(have, have ? bmm::log_(arg) : 0.0, v[bmm::term_den(role)]);
                }
            for (int g = 0; g < G; ++g)
                for (unsigned m = 0; m < (unsigned)M; ++m) {
                    const double e = bmm::group_entry(t[0].data(), t[1].data(), g, P, m, W);
                    const double o = bmm::group_entry(t[2].data(), t[3].data(), g, P, m, W);
                    Tp[((size_t)g * K + k) * M + m] = g == 0 ? cc.cp + e : e;
                    To[((size_t)g * K + k) * M + m] = g == 0 ? cc.cm + o : o;
                }
            for (int g = 0; g < Gm; ++g)
                for (unsigned m = 0; m < (unsigned)bmm::kGroupMm; ++m) {
                    const double o = bmm::group_entry(t[2].data(), t[3].data(), g, P, m, bmm::kGroupWm);
                    Tm[((size_t)g * K + k) * bmm::kGroupMm + m] = g == 0 ? cc.cm + o : o;
                }
        }
    }
    // (b): every entry of both own images is <= 0 or -inf
    long long positive_entries() const {
        long long bad = 0;
        for (double e : To) bad += !(e <= 0.0);
        for (double e : Tm) bad += !(e <= 0.0);
        for (double e : To) bad += !((float)e <= 0.0f);
        return bad;
    }
};

unsigned field(const std::vector<int>& x, int P, int g, int W) {
    unsigned m = 0;
    for (int j = 0; j < W; ++j) if (g * W + j < P && x[g * W + j]) m |= 1u << j;
    return m;
}

template <int K>
double max_of(const double (&sc)[K]) {
    double m = bmm::neg_inf();
    for (int k = 0; k < K; ++k) m = __builtin_fmax(m, sc[k]);
    return m;
}

// the definition's scores of observation x with label zo: Tp in group order, the own cluster from the width-3 Tm in
// group order, padding groups included
template <int K>
void scores64(const Images& im, const std::vector<int>& x, int zo, double (&sc)[K]) {
    double own = 0.0;
    for (int g = 0; g < im.GmPad; ++g) own = own + im.Tm[((size_t)g * K + zo) * bmm::kGroupMm + (g < im.Gm ? field(x, im.P, g, bmm::kGroupWm) : 0u)];
    for (int k = 0; k < K; ++k) {
        double a = 0.0;
        for (int g = 0; g < im.G; ++g) a = a + im.Tp[((size_t)g * K + k) * im.M + field(x, im.P, g, im.W)];
        sc[k] = k == zo ? own : a;
    }
}
// the kernel's: every score a binary32 sum of narrowed width-W entries in group order, the own cluster's from To
template <int K>
float scores32(const Images& im, const std::vector<int>& x, int zo, int push, float (&sc)[K]) {
    float m = -INFINITY;
    for (int k = 0; k < K; ++k) {
        const std::vector<double>& tab = k == zo ? im.To : im.Tp;
        float a = 0.0f;
        for (int g = 0; g < im.G; ++g) a = a + narrow(tab[((size_t)g * K + k) * im.M + field(x, im.P, g, im.W)], push);
        sc[k] = a;
        m = __builtin_fmaxf(m, a);
    }
    return m;
}

template <int K>
bool check(const Images& im, const std::vector<int>& x, int zo, double u, const double (&sc)[K], int pushes = 4) {
    const int want = bmm::draw_spec<K>(sc, max_of(sc), u);
    bool all_certain = true;
    for (int push = 0; push < pushes; ++push) {
        float s32[K];
        const float m32 = scores32<K>(im, x, zo, push, s32);
        int cnt = -1;
        const bool certain = bmm::draw_pk<K>(s32, m32, u, im.G, bmm::kPkEpsUnit, cnt);
        ++T.draws;
        T.certain += certain;
        all_certain = all_certain && certain;
        if (certain && cnt != want) {
            ++T.wrong;
            if (T.reported++ < 10) {
                std::printf("FAIL K=%d P=%d W=%d own=%d entries=%d u=%a packed=%d definition=%d scores:", K, im.P, im.W, zo, push, u, cnt, want);
                for (int k = 0; k < K; ++k) std::printf(" %a", sc[k]);
                std::printf("\n");
            }
        }
    }
    return all_certain;
}

double clamp_u(double u) { return u < 0.0 ? 0.0 : (u > 1.0 - 0x1p-52 ? 1.0 - 0x1p-52 : u); }

// uniforms at 0, at the top, at random, one grid step at a time around every CDF boundary and around the band's edge
template <int K>
void walk(const Images& im, const std::vector<int>& x, int zo, Rng& r) {
    double sc[K];
    scores64<K>(im, x, zo, sc);
    const double m = max_of(sc);
    check<K>(im, x, zo, 0.0, sc);
    check<K>(im, x, zo, 1.0 - 0x1p-52, sc);
    for (int i = 0; i < 2; ++i) check<K>(im, x, zo, r.u52(), sc);
    if (!(m > bmm::neg_inf())) return;
    double cdf[K];
    double run = 0.0;
    for (int k = 0; k < K; ++k) { run = run + bmm::expw_(sc[k] - m); cdf[k] = run; }
    const double band = (double)bmm::pk_band((float)m, im.G, bmm::kPkEpsUnit);
    static const double off[] = {0.25, 0.9, 1.1, 2.0, 16.0};
    for (int k = 0; k < K; ++k) {
        if (k > 0 && cdf[k] == cdf[k - 1]) continue;  // an impossible category: the boundary of the one before
        const double b = std::floor(cdf[k] / run * 0x1p52) * 0x1p-52;
        for (int j = -2; j <= 2; ++j) check<K>(im, x, zo, clamp_u(b + j * 0x1p-52), sc);
        for (double f : off) {
            check<K>(im, x, zo, clamp_u(b + f * band), sc);
            check<K>(im, x, zo, clamp_u(b - f * band), sc);
        }
    }
}

// an observation that can sit in cluster zo: x_d = 0 where none of its rows has a 1, 1 where all have
void draw_x(Rng& r, int P, const std::vector<long long>& n, const std::vector<long long>& s, int zo, const double* theta, std::vector<int>& x) {
    for (int d = 0; d < P; ++d) {
        const long long sd = s[(size_t)zo * P + d];
        x[d] = sd == 0 ? 0 : sd == n[zo] ? 1 : (r.unit() < (theta ? theta[d] : 0.5) ? 1 : 0);
    }
}

// adversarial counts: label 0 holds one row, label 1 two, one label none, the rest share N; features with s = 0 and
// with s = n in every label
template <int K>
void adversarial(Rng& r, int P, int W, long long N, int obs) {
    std::vector<long long> n(K), s((size_t)K * P);
    n[0] = 1; n[1] = 2; n[2] = 0;
    long long left = N - 3;
    for (int k = 3; k < K; ++k) { n[k] = k == K - 1 ? left : left / (2 + (long long)(r.next() % 5)); left -= n[k]; }
    for (int k = 0; k < K; ++k)
        for (int d = 0; d < P; ++d) {
            const unsigned c = (unsigned)(r.next() % 8);
            s[(size_t)k * P + d] = c == 0 ? 0 : c == 1 ? n[k] : c == 2 ? (n[k] > 0 ? 1 : 0) : c == 3 ? (n[k] > 0 ? n[k] - 1 : 0)
                                   : (long long)std::llround((double)n[k] * r.unit());
        }
    Images im;
    im.build(K, P, W, n, s, N, 1.0, 0.5, 0.5);
    T.positive += im.positive_entries();
    std::vector<int> x(P);
    for (int i = 0; i < obs; ++i) {
        int zo = i < 3 * (obs / 4) ? (int)(i % K) : (int)(r.next() % K);
        if (n[zo] == 0) zo = 0;  // nobody sits in an empty cluster
        draw_x(r, P, n, s, zo, nullptr, x);
        walk<K>(im, x, zo, r);
    }
}

// C5's generator at steady state: weights proportional to K..1, theta = 0.1 + 0.8 U, N = 1e7, statistics N_k theta
bool c5(int W, int walked, int obs) {
    constexpr int K = 20;
    const int P = 100;
    const long long N = 10000000;
    Rng r{21};
    std::vector<double> theta((size_t)K * P);
    for (double& t : theta) t = 0.1 + 0.8 * r.unit();
    std::vector<long long> n(K), s((size_t)K * P);
    for (int k = 0; k < K; ++k) n[k] = (long long)std::llround((double)N * (K - k) / (K * (K + 1) / 2));
    for (int k = 0; k < K; ++k) for (int d = 0; d < P; ++d) s[(size_t)k * P + d] = std::llround((double)n[k] * theta[(size_t)k * P + d]);
    Images im;
    im.build(K, P, W, n, s, N, 1.0, 0.5, 0.5);
    T.positive += im.positive_entries();
    std::vector<int> x(P);
    long long uncertain = 0, uncertain_before = 0;
    const long long wrong0 = T.wrong;
    for (int i = 0; i < obs; ++i) {
        double v = r.unit() * (K * (K + 1) / 2);
        int z = 0;
        while (z < K - 1 && v >= (double)(K - z)) { v -= (double)(K - z); ++z; }
        for (int d = 0; d < P; ++d) x[d] = r.unit() < theta[(size_t)z * P + d];
        if (i < walked) walk<K>(im, x, z, r);
        double sc[K];
        scores64<K>(im, x, z, sc);
        const double u = r.u52();
        uncertain += !check<K>(im, x, z, u, sc, 1);  // (c): the entries as narrowed, one uniform
        // the same observation and uniform with the own score narrowed from the definition's binary64 sum, as before
        float s32[K];
        scores32<K>(im, x, z, 0, s32);
        s32[z] = (float)sc[z];
        float m32 = -INFINITY;
        for (int k = 0; k < K; ++k) m32 = __builtin_fmaxf(m32, s32[k]);
        int cnt;
        uncertain_before += !bmm::draw_pk<K>(s32, m32, u, im.G, bmm::kPkEpsUnit, cnt);
    }
    const double share = (double)uncertain / obs;
    std::fprintf(stderr, "C5 tables at steady state, groups of %d: %lld of %d observations uncertain (%.4f %%; with the own score narrowed from its binary64 "
                 "sum, same observations: %lld, %.4f %%; pk_check of the parent commit, other observations: 0.058 %%), %lld certain and wrong\n",
                 W, uncertain, obs, 100.0 * share, uncertain_before, 100.0 * (double)uncertain_before / obs, T.wrong - wrong0);
    if (share > 0.005) {
        std::printf("FAIL the band is too wide to be of use: %.4f %% of C5's observations uncertain at width %d (at most 0.5 %%)\n", 100.0 * share, W);
        return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const bool quick = argc > 1 && !std::strcmp(argv[1], "quick");
    const int div = quick ? 10 : 1;
    Rng r{20260301};
    bool ok = true;
    for (int W : {bmm::kGroupW, bmm::kGroupWAlt}) {
        ok = c5(W, 400 / div, 200000 / div) && ok;
        for (long long N : {40LL, 100000LL, 1000000000LL})
            for (int P : {1, 37, 100, 128}) {
                adversarial<4>(r, P, W, N, 60 / div);
                adversarial<8>(r, P, W, N, 60 / div);
                adversarial<20>(r, P, W, N, 40 / div);
            }
    }
    std::fprintf(stderr, "draws %lld certain %lld (%.2f%%) wrong %lld | own-image entries above 0: %lld\n", T.draws, T.certain,
                 100.0 * T.certain / T.draws, T.wrong, T.positive);
    ok = ok && T.wrong == 0 && T.positive == 0;
    if (T.positive) std::printf("FAIL %lld entries of the own-cluster images are above 0 or NaN\n", T.positive);
    if (T.certain * 10 < T.draws) { std::printf("FAIL the packed tier is certain of too little for the test to mean anything\n"); ok = false; }
    if (ok) std::printf("ok\n");
    return ok ? 0 : 1;
}
