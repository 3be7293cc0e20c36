// Host build of the arithmetic of the allocation sampler's split-merge move (bmm_spec.h): the draws of a move on stream
// 18 and the prior part of its log ratio.
//   alloc_split_host draws IN OUT   IN: lines "seed sweep move N";  OUT: "i j u_bits salt" per line
//   alloc_split_host prior IN OUT   IN: lines "K N a_bits n n0 n1 split maxK lpk_bits[maxK]" (doubles as their bits);
//                                   OUT: the bits of as_log_prior per line
// Stand-alone (its own main), so it can also be built with -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bmm_spec.h"

static double from_bits(uint64_t b) {
    double d;
    std::memcpy(&d, &b, sizeof d);
    return d;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: alloc_split_host draws|prior IN OUT\n"); return 2; }
    FILE* in = std::fopen(argv[2], "r");
    FILE* out = std::fopen(argv[3], "w");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    int rc = 0;
    if (std::strcmp(argv[1], "draws") == 0) {
        unsigned long long seed;
        unsigned sweep, move;
        long long N;
        while (std::fscanf(in, "%llu %u %u %lld", &seed, &sweep, &move, &N) == 4) {
            const bmm::SmDraws d = bmm::as_move_draws(seed, sweep, move, N);
            std::fprintf(out, "%lld %lld %" PRIu64 " %u\n", (long long)d.i, (long long)d.j, bmm::dbits(d.u), d.salt);
        }
    } else if (std::strcmp(argv[1], "prior") == 0) {
        int K, split, maxK;
        long long N, n, n0, n1;
        uint64_t ab;
        while (std::fscanf(in, "%d %lld %" SCNu64 " %lld %lld %lld %d %d", &K, &N, &ab, &n, &n0, &n1, &split, &maxK) == 8) {
            if (maxK < 1 || maxK > 4096) { rc = 2; break; }
            std::vector<double> lpk((size_t)maxK);
            bool ok = true;
            for (int k = 0; k < maxK; ++k) {
                uint64_t b;
                ok = ok && std::fscanf(in, "%" SCNu64, &b) == 1;
                lpk[(size_t)k] = ok ? from_bits(b) : 0.0;
            }
            const int Kl = split ? K : K - 1;
            if (!ok || Kl < 1 || Kl + 1 > maxK) { rc = 2; break; }
            const double v = bmm::as_log_prior(K, (double)N, from_bits(ab), lpk.data(), n, n0, n1, split != 0);
            std::fprintf(out, "%" PRIu64 "\n", bmm::dbits(v));
        }
    } else {
        rc = 2;
    }
    std::fclose(in);
    std::fclose(out);
    return rc;
}
