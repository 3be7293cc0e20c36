// The middle settle tier of k_resample_pk on the host (bmm-mcmc_amd/csrc/bmm_spec.h): draw_mid -- the binary32 table
// entries the packed loop reads (Tq for every category, Tm32 for the observation's own label), widened and summed in
// binary64, then the definition's steps -- against draw_spec, the definition on the binary64 scores.  Whenever draw_mid
// says "certain" its count must be the definition's: for every category count from 2 to 32, for 1, 7, 20 and 26 lookup
// groups, scores from about -2 down to about -700, with every binary32 entry as narrowed, pushed an ulp up, an ulp
// down and alternately.  Uniforms sit on the grid of u52, one step at a time around every CDF entry and around the
// edge of the band.
//
//   mid_check          the cases above, then on tables of C5's generator at steady state (K = 20, P = 100, statistics
//                      N_k theta, the construction of tests/score_pk/pk_check.cpp with the own-cluster entries at the
//                      lookup width beside it) the share of the draws draw_pk leaves uncertain that draw_mid leaves
//                      uncertain too: must be at most 20 %
//
// Prints "ok" and exits 0, or lists the first failures and exits 1.  Counters go to stderr.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "bmm_spec.h"

namespace {

// a narrowed table entry, pushed: 0 as narrowed, 1 an ulp up, 2 an ulp down, 3 alternately (by its bits)
float narrow(double t, int push) {
    float q = (float)t;
    if (!(q == q) || std::isinf(q) || push == 0) return q;
    uint32_t b;
    __builtin_memcpy(&b, &q, 4);
    const int dir = push == 1 ? 1 : push == 2 ? -1 : (((b * 2654435761u) >> 31) ? 1 : -1);
    return std::nextafterf(q, dir > 0 ? INFINITY : -INFINITY);
}

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

struct Tally {
    long long draws = 0, certain = 0, wrong = 0;
    long long boundary = 0, boundary_certain = 0;
    long long never = 0, never_certain = 0;
    long long eps0_boundary_wrong = 0;
    int reported = 0;
} T;

enum Kind { kAny, kBoundary, kNever };
constexpr int kMaxG = 26;
constexpr int kPushes = 4;

// One observation: entries t[g][k] <= 0 of its K categories (binary64, as the table holds them); the category `own`
// is scored from entries of its own, om[g] (the "observation removed" image).  The definition's own score own64 is
// the same terms grouped otherwise: here the sum taken in the opposite order.
template <int K>
struct Obs {
    double t[kMaxG][K];
    double om[kMaxG];
    int G, own;
    double sc[K], m;                  // the definition's scores and their maximum
    float e[kPushes][kMaxG][K];       // the middle tier's entries, per push
    void prepare() {
        m = bmm::neg_inf();
        for (int k = 0; k < K; ++k) {
            double a = 0.0;
            if (k == own) for (int g = G - 1; g >= 0; --g) a = a + om[g];
            else for (int g = 0; g < G; ++g) a = a + t[g][k];
            sc[k] = a;
            m = __builtin_fmax(m, a);
        }
        for (int p = 0; p < kPushes; ++p)
            for (int g = 0; g < G; ++g)
                for (int k = 0; k < K; ++k) e[p][g][k] = narrow(k == own ? om[g] : t[g][k], p);
    }
};

template <int K>
void check(const Obs<K>& o, double u, Kind kind) {
    const int want = bmm::draw_spec<K>(o.sc, o.m, u);
    for (int ep = 0; ep < kPushes; ++ep) {
        int cnt = -1;
        const bool certain = bmm::draw_mid<K, kMaxG>(o.e[ep], o.G, u, bmm::kMidEpsUnit, cnt);
        ++T.draws;
        T.certain += certain;
        if (kind == kBoundary) { ++T.boundary; T.boundary_certain += certain; }
        if (kind == kNever) { ++T.never; T.never_certain += certain; }
        const bool bad = certain && (cnt != want || kind != kAny);
        if (certain && cnt != want) ++T.wrong;
        if (bad && T.reported < 10) {
            ++T.reported;
            std::printf("FAIL K=%d G=%d entries=%d kind=%d u=%a certain=%d middle=%d definition=%d scores:", K, o.G, ep, (int)kind, u,
                        (int)certain, cnt, want);
            for (int k = 0; k < K; ++k) std::printf(" %a", o.sc[k]);
            std::printf("\n");
        }
        int c0 = -1;
        const bool cert0 = bmm::draw_mid<K, kMaxG>(o.e[ep], o.G, u, 0.0, c0);
        if (kind == kBoundary && cert0 && c0 != want) ++T.eps0_boundary_wrong;
    }
}

double clamp_u(double u) { return u < 0.0 ? 0.0 : (u > 1.0 - 0x1p-52 ? 1.0 - 0x1p-52 : u); }

template <int K>
void sweep_uniforms(Obs<K>& o, Rng& r, Kind vec_kind) {
    o.prepare();
    check(o, 0.0, vec_kind);
    check(o, 1.0 - 0x1p-52, vec_kind == kAny ? kBoundary : vec_kind);
    for (int i = 0; i < 4; ++i) check(o, r.u52(), vec_kind);
    if (vec_kind == kNever) return;
    double cdf[K];
    double run = 0.0;
    for (int k = 0; k < K; ++k) { run = run + bmm::expw_(o.sc[k] - o.m); cdf[k] = run; }
    // the band of this observation, in units of tot: its edge and beyond
    const double band = bmm::mid_band(o.m, bmm::kMidEpsUnit);
    static const double off[] = {0.25, 0.9, 1.1, 2.0, 16.0};
    for (int k = 0; k < K; ++k) {
        const double b = std::floor(cdf[k] / run * 0x1p52) * 0x1p-52;  // the exact boundary, on the grid of u52
        for (int j = -2; j <= 2; ++j) check(o, clamp_u(b + j * 0x1p-52), kBoundary);
        for (double f : off) {
            check(o, clamp_u(b + f * band), kAny);
            check(o, clamp_u(b - f * band), kAny);
        }
    }
}

template <int K>
void run_kg(Rng& r, int G) {
    // the magnitude of a whole score, and how far the categories lie apart
    static const double depth[] = {2.0, 20.0, 60.0, 250.0, 700.0};
    static const double spread[] = {0.02, 0.5, 3.0, 12.0, 60.0};
    static Obs<K> o;
    o.G = G;
    for (int v = 0; v < 25; ++v) {
        const double D = depth[v % 5], S = spread[v / 5];
        for (int k = 0; k < K; ++k) {
            // entries <= 0: the category's share of the depth, spread unevenly over its groups
            const double total = D * (0.5 + 0.5 * r.unit()) + S * r.unit();
            double wsum = 0.0, w[kMaxG];
            for (int g = 0; g < G; ++g) { w[g] = 0.05 + r.unit(); wsum += w[g]; }
            for (int g = 0; g < G; ++g) o.t[g][k] = -total * w[g] / wsum;
        }
        if (v % 7 == 3)  // ties: a few distinct categories only
            for (int k = 1; k < K; ++k) if (r.next() % 2) for (int g = 0; g < G; ++g) o.t[g][k] = o.t[g][0];
        if (v % 7 == 5)  // impossible categories among possible ones (-inf sits in group 0, with the constant term)
            for (int k = 1; k < K; ++k) if (r.next() % 3 == 0) o.t[0][k] = bmm::neg_inf();
        o.own = (int)(r.next() % K);
        // the own label's entries: those of its column, each a little off (one row fewer in the cluster); a cluster of
        // one row now and then: -inf in group 0
        const double f = 0.8 + 0.4 * r.unit();
        for (int g = 0; g < G; ++g) o.om[g] = std::isinf(o.t[g][o.own]) ? -D / G : o.t[g][o.own] * f;
        if (v % 11 == 7) o.om[0] = bmm::neg_inf();
        sweep_uniforms(o, r, kAny);
    }
    // never certain: every category impossible; a NaN among the scores; +inf
    for (int k = 0; k < K; ++k) for (int g = 0; g < G; ++g) o.t[g][k] = g == 0 ? bmm::neg_inf() : -1.0;
    o.own = 0;
    for (int g = 0; g < G; ++g) o.om[g] = g == 0 ? bmm::neg_inf() : -1.0;
    sweep_uniforms(o, r, kNever);
    for (int k = 0; k < K; ++k) for (int g = 0; g < G; ++g) o.t[g][k] = -r.unit();
    o.own = K - 1;
    for (int g = 0; g < G; ++g) o.om[g] = -r.unit();
    o.om[G / 2] = bmm::qnan();
    sweep_uniforms(o, r, kNever);
    o.own = 0;
    for (int g = 0; g < G; ++g) o.om[g] = -1.0 / G;
    o.t[G - 1][K - 1] = bmm::pos_inf();
    sweep_uniforms(o, r, kNever);
}

template <int... I>
void run_all(Rng& r, std::integer_sequence<int, I...>) {
    for (int G : {1, 7, 20, 26}) (run_kg<I + 2>(r, G), ...);
}

// ---- tables of a mixture's statistics, as k_count_tables writes them (the finite sampler, alpha = 1): Tp and the
// width-3 Tm of the definition as tests/score_pk/pk_check.cpp builds them, and TmW, the "observation removed" terms
// grouped at the lookup width, which Tm32 is the binary32 image of
struct Tables {
    int K, P, G, Gm;
    std::vector<double> Tp, Tm, TmW;  // [G][K][32], [Gm][K][8], [G][K][32]
    void build(const std::vector<long long>& n, const std::vector<long long>& s, long long N, double alpha, double beta, double gamma) {
        G = (P + bmm::kGroupW - 1) / bmm::kGroupW;
        Gm = (P + bmm::kGroupWm - 1) / bmm::kGroupWm;
        Tp.assign((size_t)G * K * 32, 0.0);
        Tm.assign((size_t)Gm * K * 8, 0.0);
        TmW.assign((size_t)G * K * 32, 0.0);
        std::vector<double> e1(P), e0(P), m1(P), m0(P);
        const double ldN = bmm::log_((double)(N - 1) + alpha);
        for (int k = 0; k < K; ++k) {
            const long long nk = n[k];
            const double ak = bmm::div_(alpha, (double)K);
            const double cp = nk > 0 ? bmm::log_((double)nk + ak) - ldN : bmm::neg_inf();
            const double cm = nk > 1 ? bmm::log_((double)(nk - 1) + ak) - ldN : bmm::neg_inf();
            const double den_p = nk > 0 ? bmm::log_(beta + gamma + (double)nk) : 0.0, den_m = nk > 1 ? bmm::log_(beta + gamma + (double)(nk - 1)) : 0.0;
            for (int d = 0; d < P; ++d) {
                const long long sd = s[(size_t)k * P + d];
                e1[d] = nk > 0 ? bmm::log_(beta + (double)sd) - den_p : 0.0;
                e0[d] = nk > 0 ? bmm::log_((gamma + (double)nk) - (double)sd) - den_p : 0.0;
                m1[d] = nk > 1 && sd >= 1 ? bmm::log_(beta + (double)(sd - 1)) - den_m : 0.0;
                m0[d] = nk > 1 && sd <= nk - 1 ? bmm::log_((gamma + (double)(nk - 1)) - (double)sd) - den_m : 0.0;
            }
            for (int g = 0; g < G; ++g)
                for (unsigned m = 0; m < 32; ++m) {
                    const double t = bmm::group_entry(e1.data(), e0.data(), g, P, m, bmm::kGroupW);
                    Tp[((size_t)g * K + k) * 32 + m] = g == 0 ? cp + t : t;
                    const double tw = bmm::group_entry(m1.data(), m0.data(), g, P, m, bmm::kGroupW);
                    TmW[((size_t)g * K + k) * 32 + m] = g == 0 ? cm + tw : tw;
                }
            for (int g = 0; g < Gm; ++g)
                for (unsigned m = 0; m < 8; ++m) {
                    const double t = bmm::group_entry(m1.data(), m0.data(), g, P, m, bmm::kGroupWm);
                    Tm[((size_t)g * K + k) * 8 + m] = g == 0 ? cm + t : t;
                }
        }
    }
};
unsigned field(const std::vector<int>& x, int P, int g, int W) {
    unsigned m = 0;
    for (int j = 0; j < W; ++j) if (g * W + j < P && x[g * W + j]) m |= 1u << j;
    return m;
}

// C5's generator at steady state: weights proportional to K..1, theta = 0.1 + 0.8 U, N = 1e7, statistics N_k theta.
// Every observation is scored once and drawn with kDraws uniforms: the packed tier as the kernel has it (binary32 sums
// in group order, the own score from the binary32 own entries), and where that is uncertain the middle tier on the
// same entries and the definition.
bool c5_share() {
    constexpr int K = 20, kDraws = 16;
    const int P = 100;
    const long long N = 10000000;
    Rng r{21};
    std::vector<double> theta((size_t)K * P);
    for (double& t : theta) t = 0.1 + 0.8 * r.unit();
    std::vector<long long> n(K), s((size_t)K * P);
    for (int k = 0; k < K; ++k) n[k] = (long long)std::llround((double)N * (K - k) / (K * (K + 1) / 2));
    for (int k = 0; k < K; ++k) for (int d = 0; d < P; ++d) s[(size_t)k * P + d] = std::llround((double)n[k] * theta[(size_t)k * P + d]);
    Tables tb;
    tb.K = K; tb.P = P;
    tb.build(n, s, N, 1.0, 0.5, 0.5);
    if (tb.G > kMaxG) return false;
    const int obs = 200000;
    long long draws = 0, pk_uncertain = 0, mid_uncertain = 0, wrong = 0;
    std::vector<int> x(P);
    static float e[kMaxG][K];
    for (int i = 0; i < obs; ++i) {
        // an observation of the mixture, labelled with its component
        double v = r.unit() * (K * (K + 1) / 2);
        int z = 0;
        while (z < K - 1 && v >= (double)(K - z)) { v -= (double)(K - z); ++z; }
        for (int d = 0; d < P; ++d) x[d] = r.unit() < theta[(size_t)z * P + d];
        double sc[K], own = 0.0, m = bmm::neg_inf();
        float s32[K], m32 = -INFINITY;
        for (int g = 0; g < tb.Gm; ++g) own = own + tb.Tm[((size_t)g * K + z) * 8 + field(x, P, g, bmm::kGroupWm)];
        for (int k = 0; k < K; ++k) {
            double a = 0.0;
            float f = 0.0f;
            for (int g = 0; g < tb.G; ++g) {
                const size_t at = ((size_t)g * K + k) * 32 + field(x, P, g, bmm::kGroupW);
                a = a + tb.Tp[at];
                e[g][k] = (float)(k == z ? tb.TmW[at] : tb.Tp[at]);
                f = f + e[g][k];
            }
            sc[k] = k == z ? own : a;
            s32[k] = f;
            m = __builtin_fmax(m, sc[k]);
            m32 = __builtin_fmaxf(m32, f);
        }
        for (int j = 0; j < kDraws; ++j) {
            const double u = r.u52();
            int got = -1;
            ++draws;
            if (bmm::draw_pk<K>(s32, m32, u, tb.G, bmm::kPkEpsUnit, got)) continue;
            ++pk_uncertain;
            const bool certain = bmm::draw_mid<K, kMaxG>(e, tb.G, u, bmm::kMidEpsUnit, got);
            mid_uncertain += !certain;
            wrong += certain && got != bmm::draw_spec<K>(sc, m, u);
        }
    }
    const double share = pk_uncertain ? (double)mid_uncertain / (double)pk_uncertain : 1.0;
    std::fprintf(stderr,
                 "C5 tables at steady state: %lld draws, %lld uncertain in the packed tier (%.4f %%), of them %lld uncertain in the middle tier "
                 "(%.2f %%), %lld certain and wrong\n",
                 draws, pk_uncertain, 100.0 * (double)pk_uncertain / (double)draws, mid_uncertain, 100.0 * share, wrong);
    if (wrong) { std::printf("FAIL a certain draw of the middle tier was wrong on C5's tables\n"); return false; }
    if (pk_uncertain < 500) { std::printf("FAIL too few uncertain draws (%lld) for the share to mean anything\n", pk_uncertain); return false; }
    if (share > 0.20) { std::printf("FAIL the middle band is too wide to be of use: %.2f %% of the packed tier's uncertain draws stay uncertain (at most 20 %%)\n", 100.0 * share); return false; }
    return true;
}

}  // namespace

int main() {
    Rng r{20261021};
    run_all(r, std::make_integer_sequence<int, 31>{});  // K = 2 .. 32
    std::fprintf(stderr,
                 "draws %lld certain %lld (%.2f%%) wrong %lld | boundary cases %lld certain %lld | never-certain cases %lld certain %lld | "
                 "zero band: wrong at the boundaries %lld\n",
                 T.draws, T.certain, 100.0 * T.certain / T.draws, T.wrong, T.boundary, T.boundary_certain, T.never, T.never_certain,
                 T.eps0_boundary_wrong);
    bool ok = T.wrong == 0 && T.boundary_certain == 0 && T.never_certain == 0;
    if (T.certain * 10 < T.draws) { std::printf("FAIL the middle tier is certain of too little for the test to mean anything\n"); ok = false; }
    if (T.eps0_boundary_wrong == 0) { std::printf("FAIL a band of width zero was never wrong at the boundaries: the test cannot fail\n"); ok = false; }
    ok = c5_share() && ok;
    if (ok) std::printf("ok\n");
    return ok ? 0 : 1;
}
