// The packed tier of k_resample_pk on the host (bmm-mcmc_amd/csrc/bmm_spec.h): draw_pk -- scores summed in binary32
// from narrowed table entries, the own-cluster score narrowed from its binary64 sum, binary32 weights through exp2 --
// against draw_spec, the definition on the binary64 scores.  Whenever draw_pk says "certain" its count must be the
// definition's: for every category count from 2 to 32, for 1, 7, 20 and 26 lookup groups, scores down to about -700,
// with every binary32 entry as narrowed, pushed an ulp up, an ulp down and alternately, and the exponential pushed as
// tests/draw_tier1 pushes it.  Uniforms sit on the grid of u52, one step at a time around every CDF entry.
//
//   pk_check                 the cases above, then the share of uncertain observations on tables of C5's generator at
//                            steady state (K = 20, P = 100, statistics N_k theta): must be at most 0.5 %
//   pk_check rate X z K M    how often a band of width zero draws wrongly, per draw, averaged over the allocations in z
//                            (S x N labels 1..K, the allocations a chain passed through) of the 0/1 matrix X (one row of
//                            digits per line), M uniforms to a CDF boundary (rate_k below) -- what sizes the zero-band
//                            chain of tests/test_gpu_score_pk.py
//
// Prints "ok" and exits 0, or lists the first failures and exits 1.  Counters go to stderr.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "bmm_spec.h"

namespace {

enum Push { kNominal, kUp, kDown, kMixed, kFlush, kPushes };
struct Exp2Pushed {
    int push;
    float operator()(float x) const {
        float y = (float)std::exp2((double)x);
        uint32_t xb;
        __builtin_memcpy(&xb, &x, 4);
        const int dir = push == kUp ? 1 : push == kDown ? -1 : push == kMixed ? (((xb * 2654435761u) >> 31) ? 1 : -1) : 0;
        if (dir > 0 && y == y && y < INFINITY) y = std::nextafterf(y, INFINITY);
        if (dir < 0 && y > 0.0f) y = std::nextafterf(y, 0.0f);
        if (push == kFlush && y < 0x1p-126f) y = 0.0f;
        return y;
    }
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

// One observation: entries t[g][k] <= 0 of its K categories (binary64, as the table holds them), the category `own`
// scored by own64 instead.
template <int K>
struct Obs {
    double t[kMaxG][K];
    int G, own;
    double own64;
    // the definition's scores: binary64 sums in group order
    void scores64(double (&sc)[K]) const {
        for (int k = 0; k < K; ++k) {
            double a = 0.0;
            for (int g = 0; g < G; ++g) a = a + t[g][k];
            sc[k] = k == own ? own64 : a;
        }
    }
    // the packed tier's: binary32 sums of the narrowed entries, in group order
    float scores32(float (&sc)[K], int push) const {
        float m = -INFINITY;
        for (int k = 0; k < K; ++k) {
            float a = 0.0f;
            for (int g = 0; g < G; ++g) a = a + narrow(t[g][k], push);
            sc[k] = k == own ? narrow(own64, push) : a;
            m = __builtin_fmaxf(m, sc[k]);
        }
        return m;
    }
};

template <int K>
double max_of(const double (&sc)[K]) {
    double m = bmm::neg_inf();
    for (int k = 0; k < K; ++k) m = __builtin_fmax(m, sc[k]);
    return m;
}

template <int K>
void check(const Obs<K>& o, double u, Kind kind) {
    double sc[K];
    o.scores64(sc);
    const int want = bmm::draw_spec<K>(sc, max_of(sc), u);
    for (int ep = 0; ep < 4; ++ep) {
        float s32[K];
        const float m32 = o.scores32(s32, ep);
        for (int push = 0; push < kPushes; ++push) {
            int cnt = -1;
            const bool certain = bmm::draw_pk<K>(s32, m32, u, o.G, bmm::kPkEpsUnit, cnt, Exp2Pushed{push});
            ++T.draws;
            T.certain += certain;
            if (kind == kBoundary) { ++T.boundary; T.boundary_certain += certain; }
            if (kind == kNever) { ++T.never; T.never_certain += certain; }
            const bool bad = certain && (cnt != want || kind != kAny);
            if (certain && cnt != want) ++T.wrong;
            if (bad && T.reported < 10) {
                ++T.reported;
                std::printf("FAIL K=%d G=%d entries=%d exp=%d kind=%d u=%a certain=%d packed=%d definition=%d scores:", K, o.G, ep,
                            push, (int)kind, u, (int)certain, cnt, want);
                for (int k = 0; k < K; ++k) std::printf(" %a", sc[k]);
                std::printf("\n");
            }
            int c0 = -1;
            const bool cert0 = bmm::draw_pk<K>(s32, m32, u, o.G, 0.0f, c0, Exp2Pushed{push});
            if (kind == kBoundary && cert0 && c0 != want) ++T.eps0_boundary_wrong;
        }
    }
}

double clamp_u(double u) { return u < 0.0 ? 0.0 : (u > 1.0 - 0x1p-52 ? 1.0 - 0x1p-52 : u); }

template <int K>
void sweep_uniforms(const Obs<K>& o, Rng& r, Kind vec_kind) {
    double sc[K];
    o.scores64(sc);
    const double m = max_of(sc);
    check(o, 0.0, vec_kind);
    check(o, 1.0 - 0x1p-52, vec_kind == kAny ? kBoundary : vec_kind);
    for (int i = 0; i < 4; ++i) check(o, r.u52(), vec_kind);
    if (vec_kind == kNever) return;
    double cdf[K];
    double run = 0.0;
    for (int k = 0; k < K; ++k) { run = run + bmm::expw_(sc[k] - m); cdf[k] = run; }
    // the band of this observation, in units of tot: its edge and beyond
    const double band = (double)bmm::pk_band((float)m, o.G, bmm::kPkEpsUnit);
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
    Obs<K> o;
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
        double a = 0.0;
        for (int g = 0; g < G; ++g) a = a + o.t[g][o.own];
        o.own64 = std::isinf(a) ? -D : a * (0.8 + 0.4 * r.unit());
        sweep_uniforms(o, r, kAny);
    }
    // never certain: every category impossible; a NaN among the scores; +inf
    for (int k = 0; k < K; ++k) for (int g = 0; g < G; ++g) o.t[g][k] = g == 0 ? bmm::neg_inf() : -1.0;
    o.own = 0; o.own64 = bmm::neg_inf();
    sweep_uniforms(o, r, kNever);
    for (int k = 0; k < K; ++k) for (int g = 0; g < G; ++g) o.t[g][k] = -r.unit();
    o.own = K - 1; o.own64 = bmm::qnan();
    sweep_uniforms(o, r, kNever);
    o.own = 0; o.own64 = -1.0; o.t[G - 1][K - 1] = bmm::pos_inf();
    sweep_uniforms(o, r, kNever);
}

template <int... I>
void run_all(Rng& r, std::integer_sequence<int, I...>) {
    for (int G : {1, 7, 20, 26}) (run_kg<I + 2>(r, G), ...);
}

// ---- tables of a mixture's statistics, as k_count_tables writes them (the finite sampler, alpha = 1)
struct Tables {
    int K, P, G, Gm;
    std::vector<double> Tp, Tm;  // [G][K][32], [Gm][K][8]
    void build(const std::vector<long long>& n, const std::vector<long long>& s, long long N, double alpha, double beta, double gamma) {
        G = (P + bmm::kGroupW - 1) / bmm::kGroupW;
        Gm = (P + bmm::kGroupWm - 1) / bmm::kGroupWm;
        Tp.assign((size_t)G * K * 32, 0.0);
        Tm.assign((size_t)Gm * K * 8, 0.0);
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
// one observation x with label zo against the tables: the definition's count, the packed tier's answer at `unit`
template <int K, class Exp2 = bmm::Exp2Fast>
void draw_both(const Tables& tb, const std::vector<int>& x, int zo, double u, float unit, int& want, int& got, bool& certain,
               Exp2 ex2 = Exp2()) {
    double sc[K];
    float s32[K];
    float m32 = -INFINITY;
    double own = 0.0;
    for (int g = 0; g < tb.Gm; ++g) own = own + tb.Tm[((size_t)g * K + zo) * 8 + field(x, tb.P, g, bmm::kGroupWm)];
    for (int k = 0; k < K; ++k) {
        double a = 0.0;
        float f = 0.0f;
        for (int g = 0; g < tb.G; ++g) {
            const double t = tb.Tp[((size_t)g * K + k) * 32 + field(x, tb.P, g, bmm::kGroupW)];
            a = a + t;
            f = f + (float)t;
        }
        sc[k] = k == zo ? own : a;
        s32[k] = k == zo ? (float)own : f;
        m32 = __builtin_fmaxf(m32, s32[k]);
    }
    want = bmm::draw_spec<K>(sc, max_of(sc), u);
    certain = bmm::draw_pk<K>(s32, m32, u, tb.G, unit, got, ex2);
}

// C5's generator at steady state: weights proportional to K..1, theta = 0.1 + 0.8 U, N = 1e7, statistics N_k theta
bool c5_share() {
    constexpr int K = 20;
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
    const int obs = 200000;
    long long uncertain = 0, wrong = 0;
    std::vector<int> x(P);
    for (int i = 0; i < obs; ++i) {
        // an observation of the mixture, labelled with its component
        double v = r.unit() * (K * (K + 1) / 2);
        int z = 0;
        while (z < K - 1 && v >= (double)(K - z)) { v -= (double)(K - z); ++z; }
        for (int d = 0; d < P; ++d) x[d] = r.unit() < theta[(size_t)z * P + d];
        int want, got;
        bool certain;
        draw_both<K>(tb, x, z, r.u52(), bmm::kPkEpsUnit, want, got, certain);
        uncertain += !certain;
        wrong += certain && got != want;
    }
    const double share = (double)uncertain / obs;
    std::fprintf(stderr, "C5 tables at steady state: %lld of %d observations uncertain (%.4f %%), %lld certain and wrong\n", uncertain, obs,
                 100.0 * share, wrong);
    if (wrong) { std::printf("FAIL a certain draw was wrong on C5's tables\n"); return false; }
    if (share > 0.005) { std::printf("FAIL the band is too wide to be of use: %.4f %% of C5's observations uncertain (at most 0.5 %%)\n", 100.0 * share); return false; }
    return true;
}

// The zero-band wrong-draw rate per draw of a chain, averaged over the allocations z[0..S) it passed through (the
// chain rebuilds its tables every batch, so it meets a new set of CDFs each time; one allocation of K3_N1000_P5 has
// only 32 patterns x 3 labels of them).  A zero band can be wrong only where the full band is not certain, i.e. for
// u within 1.5 bands of an exact boundary cdf_k / tot (the band is more than three times the tier's error), so the
// uniforms are drawn there only, M to a boundary, and weighted by the window's width: per allocation
// rate = sum over (pattern, label) of its share of the observations x sum over boundaries of 2 w x wrong / M.
template <int K>
int rate_k(const std::vector<std::vector<int>>& X, const std::vector<int>& zall, int M) {
    const int P = (int)X[0].size();
    const long long N = (long long)X.size();
    const long long S = (long long)zall.size() / N;
    Rng r{7};
    double rate_sum = 0.0, rate_pushed_sum = 0.0;
    long long banded_wrong = 0, samples = 0, cdfs = 0;
    for (long long a = 0; a < S; ++a) {
        const int* z = zall.data() + a * N;
        std::vector<long long> n(K, 0), s((size_t)K * P, 0);
        for (long long i = 0; i < N; ++i) {
            ++n[z[i]];
            for (int d = 0; d < P; ++d) s[(size_t)z[i] * P + d] += X[i][d];
        }
        Tables tb;
        tb.K = K; tb.P = P;
        tb.build(n, s, N, 1.0, 0.5, 0.5);
        // the distinct (pattern, label) pairs of this allocation: first occurrence stands for all
        std::vector<long long> seen((size_t)K << P, -1), count((size_t)K << P, 0);
        for (long long i = 0; i < N; ++i) {
            size_t key = (size_t)z[i] << P;
            for (int d = 0; d < P; ++d) key |= (size_t)X[i][d] << d;
            if (seen[key] < 0) seen[key] = i;
            ++count[key];
        }
        for (size_t key = 0; key < seen.size(); ++key) {
            if (seen[key] < 0) continue;
            const long long i = seen[key];
            ++cdfs;
            // the definition's CDF of this observation
            double sc[K], cdf[K], own = 0.0, run = 0.0;
            for (int g = 0; g < tb.Gm; ++g) own = own + tb.Tm[((size_t)g * K + z[i]) * 8 + field(X[i], P, g, bmm::kGroupWm)];
            for (int k = 0; k < K; ++k) {
                double t = 0.0;
                for (int g = 0; g < tb.G; ++g) t = t + tb.Tp[((size_t)g * K + k) * 32 + field(X[i], P, g, bmm::kGroupW)];
                sc[k] = k == z[i] ? own : t;
            }
            const double m = max_of(sc);
            for (int k = 0; k < K; ++k) { run = run + bmm::expw_(sc[k] - m); cdf[k] = run; }
            const double w = 1.5 * (double)bmm::pk_band((float)m, tb.G, bmm::kPkEpsUnit);
            for (int k = 0; k + 1 < K; ++k) {
                if (!(cdf[k] < run) || (k > 0 && cdf[k] == cdf[k - 1])) continue;
                const double b = cdf[k] / run;
                long long wrong = 0, pushed = 0;
                for (int j = 0; j < M; ++j) {
                    const double u = std::floor(clamp_u(b + w * (2.0 * r.unit() - 1.0)) * 0x1p52) * 0x1p-52;
                    int want, got;
                    bool certain;
                    draw_both<K>(tb, X[i], z[i], u, 0.0f, want, got, certain);
                    wrong += certain && got != want;
                    draw_both<K>(tb, X[i], z[i], u, 0.0f, want, got, certain, Exp2Pushed{kMixed});
                    pushed += certain && got != want;
                    draw_both<K>(tb, X[i], z[i], u, bmm::kPkEpsUnit, want, got, certain);
                    banded_wrong += certain && got != want;
                    ++samples;
                }
                const double share = (double)count[key] / (double)N;
                rate_sum += share * 2.0 * w * (double)wrong / M;
                rate_pushed_sum += share * 2.0 * w * (double)pushed / M;
            }
        }
    }
    std::printf("zero band: %.3e wrong draws per draw (%.3e with the exponential an ulp off either way), over %lld allocations, %lld CDFs, "
                "%lld uniforms within 1.5 bands of a boundary; with the band: %lld wrong\n",
                rate_sum / (double)S, rate_pushed_sum / (double)S, S, cdfs, samples, banded_wrong);
    return banded_wrong ? 1 : 0;
}

int rate(int argc, char** argv) {
    if (argc < 6) return 2;
    std::vector<std::vector<int>> X;
    std::vector<int> z;
    char line[4096];
    FILE* f = std::fopen(argv[2], "r");
    if (!f) return 2;
    while (std::fgets(line, sizeof line, f)) {
        std::vector<int> row;
        for (char* c = line; *c; ++c) if (*c == '0' || *c == '1') row.push_back(*c - '0');
        if (!row.empty()) X.push_back(row);
    }
    std::fclose(f);
    f = std::fopen(argv[3], "r");
    if (!f) return 2;
    int v;
    while (std::fscanf(f, "%d", &v) == 1) z.push_back(v - 1);
    std::fclose(f);
    const int K = std::atoi(argv[4]);
    const int M = std::atoi(argv[5]);
    if (X.empty() || z.empty() || z.size() % X.size() != 0 || X[0].size() > 16 || M < 1) return 2;
    for (int l : z) if (l < 0 || l >= K) return 2;
    return K == 3 ? rate_k<3>(X, z, M) : K == 12 ? rate_k<12>(X, z, M) : 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "rate")) return rate(argc, argv);
    Rng r{20250301};
    run_all(r, std::make_integer_sequence<int, 31>{});  // K = 2 .. 32
    std::fprintf(stderr,
                 "draws %lld certain %lld (%.2f%%) wrong %lld | boundary cases %lld certain %lld | never-certain cases %lld certain %lld | "
                 "zero band: wrong at the boundaries %lld\n",
                 T.draws, T.certain, 100.0 * T.certain / T.draws, T.wrong, T.boundary, T.boundary_certain, T.never, T.never_certain,
                 T.eps0_boundary_wrong);
    bool ok = T.wrong == 0 && T.boundary_certain == 0 && T.never_certain == 0;
    if (T.certain * 10 < T.draws) { std::printf("FAIL the packed tier is certain of too little for the test to mean anything\n"); ok = false; }
    if (T.eps0_boundary_wrong == 0) { std::printf("FAIL a band of width zero was never wrong at the boundaries: the test cannot fail\n"); ok = false; }
    ok = c5_share() && ok;
    if (ok) std::printf("ok\n");
    return ok ? 0 : 1;
}
