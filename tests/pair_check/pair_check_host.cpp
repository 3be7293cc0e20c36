// The host statement of the pairwise local-dependence check (bmm_spec.h pc_label, pc_z, pair_check_spec;
// include/bmm_mcmc.h "pairwise local-dependence check") as a program: reads one state's counts from a text file and
// writes, per pair in the library's order, A, V, Z and X2 as the 16 hex digits of their bits, then df.
// tests/test_pair_check_ref.py holds it to the NumPy restatement; tests/test_gpu_pair_check.py holds the device to it bit
// for bit.
//
// Input, whitespace separated, all decimal:
//   Kc M
//   nk[0 .. Kc)
//   marg[0 .. Kc * M)            marg[k * M + m]
//   cnt[0 .. Kc * npairs)        cnt[k * npairs + pair]
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "bmm_spec.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s state.txt\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int Kc = 0, M = 0;
    if (fscanf(f, "%d %d", &Kc, &M) != 2 || Kc < 1 || M < 2 || M > bmm::kPcMaxM) return 3;
    const int64_t np = bmm::pc_npairs(M);
    std::vector<uint32_t> nk((size_t)Kc), marg((size_t)Kc * M), cnt((size_t)Kc * np);
    for (uint32_t& v : nk) if (fscanf(f, "%" SCNu32, &v) != 1) return 3;
    for (uint32_t& v : marg) if (fscanf(f, "%" SCNu32, &v) != 1) return 3;
    for (uint32_t& v : cnt) if (fscanf(f, "%" SCNu32, &v) != 1) return 3;
    fclose(f);
    std::vector<double> z((size_t)np), x2((size_t)np);
    std::vector<int32_t> df((size_t)np);
    bmm::pair_check_spec(Kc, M, cnt.data(), nk.data(), marg.data(), z.data(), x2.data(), df.data());
    for (int64_t q = 0; q < np; ++q) {
        int i = 0, j = 0;
        bmm::pc_pair_ij(q, M, i, j);
        if (bmm::pc_pair_index(i, j, M) != q) return 4;
        bmm::PcSums t = bmm::pc_zero();
        for (int k = 0; k < Kc; ++k)
            bmm::pc_label(t, (int64_t)cnt[(size_t)k * np + q], (int64_t)nk[k], (int64_t)marg[(size_t)k * M + i], (int64_t)marg[(size_t)k * M + j]);
        if (bmm::dbits(t.X2) != bmm::dbits(x2[(size_t)q]) || t.df != df[(size_t)q]) return 4;
        printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d\n", bmm::dbits(t.A), bmm::dbits(t.V), bmm::dbits(z[(size_t)q]),
               bmm::dbits(x2[(size_t)q]), (int)df[(size_t)q]);
    }
    return 0;
}
