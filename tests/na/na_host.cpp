// The imputation step of the missing cells (include/bmm_mcmc.h "missing data"), stated on the host over bmm_spec.h:
// the site list, the census, the observed-only Beta parameters, the draw, the S deltas and the folds of one step -- or
// of `reps` steps in a row under consecutive sweep indices -- from (labels, planes, counts, seed, sweep).  Built by
// tests/na_ref.py with g++ -ffp-contract=off; the CPU tests hold it to the NumPy restatement, the GPU tests hold the
// device to it bit for bit.
//
// input (a text file; doubles as 16 hex digits of their bits):
//   N P K explicit mode fold reps  beta gamma  seed sweep  n_cells
//   z[N]  (0-based, -1: no seat)        Xb[W * N] (plane word w of row i at w * N + i)
//   Nk[K]  S[K * P] (k * P + j)         theta[K * P] (k + j * K; explicit chains only)
//   rows[n_cells]  cols[n_cells]        sum_phi[n_cells]  ones[n_cells]
// mode 0: the starting fill (sweep 0, rate beta / (beta + gamma)); mode 1: the step.
// output: "site", "cnt" and "cell" lines of the first step, a "bits" line per step, then "S", "X", "sum", "ones".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bmm_spec.h"

using namespace bmm;

static uint64_t rd_hex(FILE* f) { unsigned long long v = 0; if (fscanf(f, "%llx", &v) != 1) exit(2); return v; }
static long long rd_int(FILE* f) { long long v = 0; if (fscanf(f, "%lld", &v) != 1) exit(2); return v; }

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 1;
    const int64_t N = rd_int(f);
    const int P = (int)rd_int(f), K = (int)rd_int(f), expl = (int)rd_int(f), mode = (int)rd_int(f), fold = (int)rd_int(f);
    const int reps = (int)rd_int(f);
    const double beta = dfrom(rd_hex(f)), gamma = dfrom(rd_hex(f));
    unsigned long long seed_in = 0;
    if (fscanf(f, "%llu", &seed_in) != 1) return 2;
    const uint64_t seed = seed_in;
    uint32_t sweep = (uint32_t)rd_int(f);
    const int64_t nc = rd_int(f);
    const int W = (P + 31) / 32;
    const size_t KP = (size_t)K * P;
    std::vector<int32_t> z((size_t)N), Nk((size_t)K), S(KP);
    std::vector<uint32_t> Xb((size_t)W * N);
    std::vector<double> theta(KP, 0.0), sum((size_t)nc);
    std::vector<int64_t> rows((size_t)nc);
    std::vector<int32_t> cols((size_t)nc);
    std::vector<uint32_t> ones((size_t)nc);
    for (auto& v : z) v = (int32_t)rd_int(f);
    for (auto& v : Xb) v = (uint32_t)rd_int(f);
    for (auto& v : Nk) v = (int32_t)rd_int(f);
    for (auto& v : S) v = (int32_t)rd_int(f);
    if (expl) for (auto& v : theta) v = dfrom(rd_hex(f));
    for (auto& v : rows) v = rd_int(f);
    for (auto& v : cols) v = (int32_t)rd_int(f);
    for (auto& v : sum) v = dfrom(rd_hex(f));
    for (auto& v : ones) v = (uint32_t)rd_int(f);
    fclose(f);

    // the sites: one per (row, plane word) with a hole, its cells consecutive in the list
    struct Site { int64_t row; int w; uint32_t mask; int64_t first; };
    std::vector<Site> sites;
    for (int64_t q = 0; q < nc; ++q) {
        const int w = cols[(size_t)q] >> 5;
        if (sites.empty() || sites.back().row != rows[(size_t)q] || sites.back().w != w) sites.push_back({rows[(size_t)q], w, 0u, q});
        sites.back().mask |= 1u << (cols[(size_t)q] & 31);
    }
    for (const Site& s : sites) printf("site %" PRId64 " %d %u %" PRId64 "\n", s.row, s.w, s.mask, s.first);

    std::vector<double> phi(KP, 0.0);
    const double rate = div_(beta, beta + gamma);
    for (int r = 0; r < reps; ++r, ++sweep) {
        const bool first = r == 0;
        if (mode == 1 && !expl) {  // census, then the auxiliary rates from the observed-only counts
            std::vector<int32_t> M(KP, 0), O(KP, 0);
            for (const Site& s : sites) {
                const int k = z[(size_t)s.row];
                if (k < 0) continue;
                const uint32_t x = Xb[(size_t)s.w * N + s.row];
                for (int b = 0; b < 32; ++b)
                    if (s.mask >> b & 1u) { M[(size_t)k * P + s.w * 32 + b]++; O[(size_t)k * P + s.w * 32 + b] += x >> b & 1u; }
            }
            for (size_t kj = 0; kj < KP; ++kj) {
                if (M[kj] <= 0) continue;
                const int k = (int)(kj / P), j = (int)(kj % P);
                const int64_t so = (int64_t)S[kj] - O[kj], no = (int64_t)Nk[(size_t)k] - M[kj];
                const double ph = na_phi(seed, beta, gamma, (uint32_t)kj, sweep, so, no);
                phi[(size_t)k + (size_t)j * K] = ph;
                if (first)
                    printf("cnt %zu %d %d %" PRId64 " %" PRId64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", kj, M[kj], O[kj], so, no,
                           dbits(beta + (double)so), dbits((gamma + (double)no) - (double)so), dbits(ph));
            }
        }
        std::string bits = "bits";
        for (const Site& s : sites) {
            const int k = z[(size_t)s.row];
            uint32_t& x = Xb[(size_t)s.w * N + s.row];
            int64_t cell = s.first;
            for (int b = 0; b < 32; ++b) {
                if (!(s.mask >> b & 1u)) continue;
                const int j = s.w * 32 + b;
                if (mode == 1 && k < 0) { bits += x >> b & 1u ? " 1" : " 0"; ++cell; continue; }
                const double ph = mode == 0 ? rate : (expl ? theta[(size_t)k + (size_t)j * K] : phi[(size_t)k + (size_t)j * K]);
                const double u = na_uniform(seed, (uint64_t)s.row * (uint64_t)P + (uint64_t)j, mode == 0 ? 0u : sweep);
                const uint32_t nb = u < ph ? 1u : 0u;
                const int d = (int)nb - (int)(x >> b & 1u);
                x = (x & ~(1u << b)) | (nb << b);
                if (k >= 0) S[(size_t)k * P + j] += d;
                if (mode == 1 && fold) { sum[(size_t)cell] = sum[(size_t)cell] + ph; ones[(size_t)cell] += nb; }
                if (first) printf("cell %" PRId64 " %016" PRIx64 " %016" PRIx64 " %u\n", cell, dbits(u), dbits(ph), nb);
                bits += nb ? " 1" : " 0";
                ++cell;
            }
        }
        printf("%s\n", bits.c_str());
    }
    printf("S");
    for (int32_t v : S) printf(" %d", v);
    printf("\nX");
    for (uint32_t v : Xb) printf(" %u", v);
    printf("\nsum");
    for (double v : sum) printf(" %016" PRIx64, dbits(v));
    printf("\nones");
    for (uint32_t v : ones) printf(" %u", v);
    printf("\n");
    return 0;
}
