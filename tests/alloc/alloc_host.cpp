// Host build of the allocation sampler's arithmetic (bmm_spec.h): the draws of a move and the closed-form log q.
//   alloc_host draws IN OUT   IN: lines "seed sweep move K maxK e"; OUT: "kind j1 j2 u_bits pe_bits salt" per line
//   alloc_host logq IN OUT    IN: lines "e n1 n2";                 OUT: "lgamma_(e+n1) lbeta_(e+n1,e+n2) ea_log_q" as bits
// Stand-alone (its own main), so it can also be built with -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "bmm_spec.h"

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: alloc_host draws|logq IN OUT\n"); return 2; }
    FILE* in = std::fopen(argv[2], "r");
    FILE* out = std::fopen(argv[3], "w");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    int rc = 0;
    if (std::strcmp(argv[1], "draws") == 0) {
        unsigned long long seed;
        unsigned sweep, move;
        int K, maxK;
        double e;
        while (std::fscanf(in, "%llu %u %u %d %d %lf", &seed, &sweep, &move, &K, &maxK, &e) == 6) {
            const bmm::EaDraws d = bmm::ea_move_draws(seed, sweep, move, K, maxK, e);
            std::fprintf(out, "%d %d %d %" PRIu64 " %" PRIu64 " %u\n", d.kind, d.j1, d.j2, bmm::dbits(d.u), bmm::dbits(d.pe), d.salt);
        }
    } else if (std::strcmp(argv[1], "logq") == 0) {
        double e;
        long long n1, n2;
        while (std::fscanf(in, "%lf %lld %lld", &e, &n1, &n2) == 3) {
            const double lg = bmm::lgamma_(e + (double)n1), lb = bmm::lbeta_(e + (double)n1, e + (double)n2);
            std::fprintf(out, "%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", bmm::dbits(lg), bmm::dbits(lb), bmm::dbits(bmm::ea_log_q(e, n1, n2)));
        }
    } else {
        rc = 2;
    }
    std::fclose(in);
    std::fclose(out);
    return rc;
}
