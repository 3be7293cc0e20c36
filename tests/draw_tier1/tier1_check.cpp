// The two-tier draw of k_resample on the host (bmm-mcmc_amd/csrc/bmm_spec.h): draw_tier1, the binary32 tier, against
// draw_spec, the definition (expw_, binary64 running sum, count).  Whenever tier 1 says "certain" its count must be
// the definition's -- for every category count from 2 to 56 (and 64, the most the bound is derived for), with the
// binary32 exponential at its nominal value, pushed up and down by an ulp (more than v_exp_f32's documented
// error: the nominal value here is itself within half an ulp), pushed alternately, and with results below 2^-126
// flushed to zero as the hardware does.  Uniforms sit on the grid of u52 (multiples of 2^-52).
//
// Prints "ok" and exits 0, or lists the first failures and exits 1.  Counters go to stderr.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "bmm_spec.h"

namespace {

// ---- the exponential under test
enum Push { kNominal, kUp, kDown, kMixed, kFlush, kPushes };
struct Exp2Pushed {
    int push;
    float operator()(float x) const {
        float y = (float)std::exp2((double)x);  // correctly rounded but for double rounding: within 0.5 ulp + 2^-29
        uint32_t xb;
        __builtin_memcpy(&xb, &x, 4);
        const int dir = push == kUp ? 1 : push == kDown ? -1 : push == kMixed ? (((xb * 2654435761u) >> 31) ? 1 : -1) : 0;
        if (dir > 0 && y == y && y < INFINITY) y = std::nextafterf(y, INFINITY);
        if (dir < 0 && y > 0.0f) y = std::nextafterf(y, 0.0f);
        if (push == kFlush && y < 0x1p-126f) y = 0.0f;
        return y;
    }
};

// ---- random numbers (splitmix64)
struct Rng {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double unit() { return (double)(next() >> 11) * 0x1p-53; }
    double u52() { return (double)(next() >> 12) * 0x1p-52; }  // the grid of bmm::u52
    double normal() { return std::sqrt(-2.0 * std::log(1.0 - unit())) * std::cos(6.283185307179586 * unit()); }
};

struct Tally {
    long long draws = 0, certain = 0, wrong = 0;          // at kTier1Eps: wrong must stay 0
    long long boundary = 0, boundary_certain = 0;         // constructed boundary cases: certain must stay 0
    long long never = 0, never_certain = 0;               // impossible / NaN lanes: certain must stay 0
    long long eps0_boundary_wrong = 0;                    // a band of width zero at the same boundaries: must be > 0
    long long eps0_random = 0, eps0_random_wrong = 0;     // (information: how often a zero band is wrong at random)
    int reported = 0;
} T;

enum Kind { kAny, kBoundary, kNever };

template <int K>
double max_of(const double (&sc)[K]) {
    double m = bmm::neg_inf();
    for (int k = 0; k < K; ++k) m = __builtin_fmax(m, sc[k]);  // as the kernel takes it: a NaN is passed over
    return m;
}

template <int K>
void check(const double (&sc)[K], double u, Kind kind) {
    const double m = max_of(sc);
    const int want = bmm::draw_spec<K>(sc, m, u);
    for (int push = 0; push < kPushes; ++push) {
        int cnt = -1;
        const bool certain = bmm::draw_tier1<K>(sc, m, u, bmm::kTier1Eps, cnt, Exp2Pushed{push});
        ++T.draws;
        T.certain += certain;
        if (kind == kBoundary) { ++T.boundary; T.boundary_certain += certain; }
        if (kind == kNever) { ++T.never; T.never_certain += certain; }
        const bool bad = (certain && cnt != want) || (certain && kind != kAny);
        if (certain && cnt != want) ++T.wrong;
        if (bad && T.reported < 10) {
            ++T.reported;
            std::printf("FAIL K=%d push=%d kind=%d u=%a certain=%d tier1=%d definition=%d scores:", K, push, (int)kind, u, (int)certain, cnt, want);
            for (int k = 0; k < K; ++k) std::printf(" %a", sc[k]);
            std::printf("\n");
        }
        // the same with a band of width zero: what the band is for
        int c0 = -1;
        const bool cert0 = bmm::draw_tier1<K>(sc, m, u, 0.0f, c0, Exp2Pushed{push});
        if (kind == kBoundary && cert0 && c0 != want) ++T.eps0_boundary_wrong;
        if (kind == kAny) { ++T.eps0_random; T.eps0_random_wrong += cert0 && c0 != want; }
    }
}

double clamp_u(double u) { return u < 0.0 ? 0.0 : (u > 1.0 - 0x1p-52 ? 1.0 - 0x1p-52 : u); }

// every uniform of interest for one score vector
template <int K>
void sweep_uniforms(const double (&sc)[K], Rng& r, Kind vec_kind) {
    const double m = max_of(sc);
    check(sc, 0.0, vec_kind);
    check(sc, 1.0 - 0x1p-52, vec_kind == kAny ? kBoundary : vec_kind);  // u~ = 1: a tie with the last CDF entry
    for (int i = 0; i < 12; ++i) check(sc, r.u52(), vec_kind);
    if (vec_kind == kNever) return;
    // the definition's CDF, as draw_spec builds it
    double cdf[K];
    double run = 0.0;
    for (int k = 0; k < K; ++k) { run = run + bmm::expw_(sc[k] - m); cdf[k] = run; }
    static const double off[] = {0.5, 0.9, 1.0, 1.1, 1.5, 2.0, 4.0, 64.0};
    for (int k = 0; k < K; ++k) {
        const double b = std::floor(cdf[k] / run * 0x1p52) * 0x1p-52;  // the exact boundary, on the grid of u52
        // at, just below and just above it, one step of the grid at a time
        for (int j = -3; j <= 3; ++j) check(sc, clamp_u(b + j * 0x1p-52), kBoundary);
        // around the edge of the band and beyond
        for (double o : off) {
            check(sc, clamp_u(b + o * 0x1p-16), kAny);
            check(sc, clamp_u(b - o * 0x1p-16), kAny);
        }
    }
}

template <int K>
void run_k(Rng& r) {
    static const double spread[] = {0.05, 0.5, 2.0, 8.0, 15.0, 40.0, 200.0, 800.0};
    double sc[K];
    const int vectors = 96;
    for (int v = 0; v < vectors; ++v) {
        const double s = spread[v % 8];
        const double base = (v & 8) ? -3000.0 * r.unit() : 0.0;  // scores are sums of a hundred log terms
        for (int k = 0; k < K; ++k) sc[k] = base + s * r.normal();
        const int kind = (v / 16) % 3;
        if (kind == 1)  // ties: a few distinct values only
            for (int k = 0; k < K; ++k) sc[k] = base - s * (double)(r.next() % 3);
        if (kind == 2)  // impossible categories among possible ones
            for (int k = 0; k < K; ++k) if (r.next() % 3 == 0 && k != (v % K)) sc[k] = bmm::neg_inf();
        sweep_uniforms(sc, r, kAny);
    }
    // all equal; one possible category (first, last); runner-up a rounding distance behind
    for (int k = 0; k < K; ++k) sc[k] = -123.456;
    sweep_uniforms(sc, r, kAny);
    for (int pos : {0, K - 1}) {
        for (int k = 0; k < K; ++k) sc[k] = k == pos ? -77.0 : bmm::neg_inf();
        sweep_uniforms(sc, r, kAny);
    }
    for (int k = 0; k < K; ++k) sc[k] = -50.0 - (k == 0 ? 0.0 : 1e-300 * k);
    sweep_uniforms(sc, r, kAny);
    // never certain: every category impossible; a NaN among the scores (anywhere, also where the maximum would be); +inf
    for (int k = 0; k < K; ++k) sc[k] = bmm::neg_inf();
    sweep_uniforms(sc, r, kNever);
    for (int pos : {0, K / 2, K - 1}) {
        for (int k = 0; k < K; ++k) sc[k] = -3.0 * r.unit();
        sc[pos] = bmm::qnan();
        sweep_uniforms(sc, r, kNever);
    }
    for (int k = 0; k < K; ++k) sc[k] = bmm::qnan();
    sweep_uniforms(sc, r, kNever);
    for (int k = 0; k < K; ++k) sc[k] = -3.0 * r.unit();
    sc[K - 1] = bmm::pos_inf();
    sweep_uniforms(sc, r, kNever);
}

template <int... I>
void run_all(Rng& r, std::integer_sequence<int, I...>) { (run_k<I + 2>(r), ...); }

}  // namespace

int main() {
    Rng r{20240607};
    run_all(r, std::make_integer_sequence<int, 55>{});  // K = 2 .. 56
    run_k<64>(r);
    std::fprintf(stderr,
                 "draws %lld certain %lld (%.2f%%) wrong %lld | boundary cases %lld certain %lld | never-certain cases %lld certain %lld | "
                 "zero band: wrong at the boundaries %lld, wrong at random %lld of %lld\n",
                 T.draws, T.certain, 100.0 * T.certain / T.draws, T.wrong, T.boundary, T.boundary_certain, T.never, T.never_certain,
                 T.eps0_boundary_wrong, T.eps0_random_wrong, T.eps0_random);
    bool ok = T.wrong == 0 && T.boundary_certain == 0 && T.never_certain == 0;
    if (T.certain * 10 < T.draws) { std::printf("FAIL tier 1 is certain of too little for the test to mean anything\n"); ok = false; }
    if (T.eps0_boundary_wrong == 0) { std::printf("FAIL a band of width zero was never wrong at the boundaries: the test cannot fail\n"); ok = false; }
    if (ok) std::printf("ok\n");
    return ok ? 0 : 1;
}
