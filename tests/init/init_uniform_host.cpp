// The spec's init_uniform on the host: prints init_uniform(seed, j) for j = 0 .. n - 1 as the bits of the binary64
// value, one hexadecimal word per line (tests/test_init_ref.py).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "bmm_spec.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const uint64_t seed = std::strtoull(argv[1], nullptr, 10);
    const int n = std::atoi(argv[2]);
    for (int j = 0; j < n; ++j) std::printf("%016" PRIx64 "\n", bmm::dbits(bmm::init_uniform(seed, (uint32_t)j)));
    return 0;
}
