// The host statement of the log joint (bmm_spec.h log_joint_spec; include/bmm_mcmc.h "log joint trace") as a program:
// reads one state's counts from a text file and writes the four doubles of its row, each as the 16 hex digits of its
// bits and in decimal.  tests/test_logpost_host_cpu.py holds it to the SciPy restatement; tests/test_gpu_logpost.py
// holds the device to it bit for bit.
//
// Input, whitespace separated; doubles as the 16 hex digits of their bits:
//   kind K k_open P N
//   beta gamma alpha a b log_pk rho
//   sample_alpha masked
//   Nk[0 .. K)
//   S[0 .. K * P)            S[k * P + d]
//   mask[0 .. ceil(P / 32))  words in hex, only when masked
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "bmm_spec.h"

static bool read_double(FILE* f, double& v) {
    uint64_t u = 0;
    if (fscanf(f, "%" SCNx64, &u) != 1) return false;
    v = bmm::dfrom(u);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s state.txt\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    bmm::LjModel m{};
    long long N = 0;
    if (fscanf(f, "%d %d %d %d %lld", &m.kind, &m.K, &m.k_open, &m.P, &N) != 5) return 3;
    m.N = N;
    if (!(read_double(f, m.beta) && read_double(f, m.gamma) && read_double(f, m.alpha) && read_double(f, m.a) &&
          read_double(f, m.b) && read_double(f, m.log_pk) && read_double(f, m.rho)))
        return 3;
    if (fscanf(f, "%d %d", &m.sample_alpha, &m.masked) != 2) return 3;
    if (m.K < 1 || m.P < 1 || m.k_open < 1 || m.k_open > m.K || m.kind < 0 || m.kind > 3) return 3;
    std::vector<int32_t> Nk((size_t)m.K), S((size_t)m.K * m.P);
    for (int32_t& v : Nk) if (fscanf(f, "%d", &v) != 1) return 3;
    for (int32_t& v : S) if (fscanf(f, "%d", &v) != 1) return 3;
    const int W = (m.P + 31) / 32;
    std::vector<uint32_t> mask((size_t)W, 0u);
    m.p_in = m.P;
    if (m.masked) {
        m.p_in = 0;
        for (int w = 0; w < W; ++w) {
            if (fscanf(f, "%x", &mask[(size_t)w]) != 1) return 3;
            m.p_in += __builtin_popcount(mask[(size_t)w] & bmm::init_word_mask(m.P, w));
        }
    }
    fclose(f);
    std::vector<double> scratch((size_t)2 * m.K);
    double out[4];
    bmm::log_joint_spec(m, Nk.data(), S.data(), m.masked ? mask.data() : nullptr, scratch.data(), out);
    for (int q = 0; q < 4; ++q) printf("%016" PRIx64 " %.17g\n", bmm::dbits(out[q]), out[q]);
    return 0;
}
