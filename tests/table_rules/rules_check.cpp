// The count-table rules of bmm-mcmc_amd/csrc/bmm_spec.h on the host, against the oracle's conditional of one row.
//
// The rules are what build_tables_self (BUILD_SELF, the finite sampler's sweep) and k_state_tables (BUILD_PREDICT,
// BUILD_LOO) evaluate on the device.  The oracle has the finite sweep's conditional, so that is the rule held here:
// for every row of a small data set the program builds the scores of the z-step the way a table image gives them --
// the raw logs of const_arg and term_arg, cat_consts and term_of, the entries through group_entry, the groups summed
// in image order with the category's constant in group 0, the row's own label from the minus-self set in groups of
// kGroupWm -- and compares them with score[] of oracle_collapsed_cond_spec (oracle/bmm_oracle.c).  The oracle's scores
// are that table arithmetic, so equality is exact (-inf equals -inf).  The stored-state rules share every function
// with this one; their values are held on the device (tests/test_gpu_predict.py, tests/test_gpu_loo.py, the pins).
// k_count_tables (any flavour) does not call these functions; the oracle chains hold it on the device
// (tests/test_gpu_parity.py, tests/test_gpu_alloc_sweep.py).
//
// The labels leave one label empty and one with a single row, one label has a feature nobody shows and a feature
// everybody shows (s = 0, s = n), P = 125 is among the shapes and both group widths occur.  Every guard counts how
// often it fired; a guard that never fired fails.
//
// Prints "ok" and exits 0, or lists the first failures and exits 1.  Counters go to stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bmm_oracle.h"
#include "bmm_spec.h"

namespace {

using namespace bmm;

struct Case { int N, P, K; double alpha, beta, gamma; };
enum Guard { gEmptyLabel, gSingleOwn, gSingleOther, gNobodyShows, gEverybodyShows, gGuards };
const char* const kGuardName[gGuards] = {"an empty label scores -inf", "a single-row label scored by its own row",
                                         "a single-row label scored by another row", "minus-self x = 1 where s = 0",
                                         "minus-self x = 0 where s = n"};
long fired[gGuards];
int failures = 0;

struct Rng {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
};

bool same(double a, double b) { return a == b; }  // (-inf == -inf; a NaN on either side fails)

// the score of row i for category k from the rule functions, as a table image would give it
double rule_score(const CountRule& r, int k, int64_t n, const int32_t* s, const int32_t* x, int P, int gw, bool own) {
    double v[kRuleLogs], arg;
    const double ak = rule_ak(r);
    for (int j = 0; j < kRuleLogs; ++j) v[j] = const_arg(r, ak, k, n, j, arg) ? log_(arg) : 0.0;
    const CatConsts c = cat_consts(r, k, n, v);
    std::vector<double> e1(P), e0(P);
    for (int d = 0; d < P; ++d)
        for (int x1 = 0; x1 < 2; ++x1) {
            const int role = (own ? 2 : 0) + (x1 ? 0 : 1);
            const bool have = term_arg(r, k, role, n, s[d], arg);
            (x1 ? e1 : e0)[d] = term_of(have, have ? log_(arg) : 0.0, term_den(role) ? c.den_m : c.den_p);
            if (own && !have && rule_minus(r, k, n)) fired[x1 ? gNobodyShows : gEverybodyShows]++;
        }
    const int W = own ? kGroupWm : gw, G = (P + W - 1) / W;
    double acc = 0.0;
    for (int g = 0; g < G; ++g) {
        unsigned m = 0;
        for (int j = 0; j < W; ++j)
            if (g * W + j < P) m |= (unsigned)(x[g * W + j] & 1) << j;
        const double t = group_entry(e1.data(), e0.data(), g, P, m, W);
        acc = acc + (g == 0 ? (own ? c.cm : c.cp) + t : t);
    }
    return acc;
}

void run(const Case& cs, int* widths_seen) {
    const int N = cs.N, P = cs.P, K = cs.K;
    Rng rng{(uint64_t)(7 * P + K)};
    std::vector<int32_t> X((size_t)N * P), z(N);
    for (int i = 0; i < N; ++i) {
        int lab;
        do lab = 1 + (int)(rng.next() % (uint64_t)K); while (lab == 3 || lab == 5);  // 3: a single row, 5: empty
        z[i] = i == 0 ? 3 : lab;
        for (int d = 0; d < P; ++d) X[i + (size_t)d * N] = (int32_t)(rng.next() & 1);
        if (z[i] == 1) { X[i] = 0; X[i + (size_t)N] = 1; }  // label 1: nobody shows feature 0, everybody feature 1
    }
    std::vector<int32_t> Nk(K, 0), S((size_t)K * P, 0), xi(P);
    for (int i = 0; i < N; ++i) {
        Nk[z[i] - 1]++;
        for (int d = 0; d < P; ++d) S[(size_t)(z[i] - 1) * P + d] += X[i + (size_t)d * N];
    }
    const int gw = oracle_group_width_for(0, K, P);
    *widths_seen |= gw == kGroupW ? 1 : 2;
    const CountRule r{BUILD_SELF, false, K, N, cs.beta, cs.gamma, cs.alpha};
    std::vector<double> want(K), norm(K);
    for (int i = 0; i < N; ++i) {
        oracle_collapsed_cond_spec(X.data(), N, P, z.data(), i, K, cs.alpha, cs.beta, cs.gamma, want.data(), norm.data());
        for (int d = 0; d < P; ++d) xi[d] = X[i + (size_t)d * N];
        for (int k = 0; k < K; ++k) {
            const bool own = k == z[i] - 1;
            const int64_t n = Nk[k];
            const double got = rule_score(r, k, n, &S[(size_t)k * P], xi.data(), P, gw, own);
            if (n == 0) fired[gEmptyLabel]++;
            else if (n == 1) fired[own ? gSingleOwn : gSingleOther]++;
            if (!same(got, want[k]) && failures++ < 10)
                std::printf("P %d K %d row %d category %d (n = %lld%s): rules %.17g, oracle %.17g\n", P, K,
                            i, k, (long long)n, own ? ", own" : "", got, want[k]);
        }
    }
}

}  // namespace

int main() {
    const Case cases[] = {{80, 20, 7, 1.3, 0.7, 0.4}, {80, 33, 12, 0.6, 0.5, 1.5}, {80, 125, 6, 1.0, 0.5, 0.5}, {80, 125, 20, 1.3, 0.5, 0.5}};
    int widths_seen = 0;
    for (const Case& c : cases) run(c, &widths_seen);
    for (int g = 0; g < gGuards; ++g) {
        std::fprintf(stderr, "%-60s %ld\n", kGuardName[g], fired[g]);
        if (fired[g] == 0) { std::printf("never reached: %s\n", kGuardName[g]); failures++; }
    }
    if (widths_seen != 3) { std::printf("not both group widths (%d)\n", widths_seen); failures++; }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
