// The spec's lgamma_ on the host: reads binary64 arguments from the file named first, writes the results to the
// file named second (tests/test_split_merge_ref.py, tests/test_gpu_split_merge.py).
#include <cstdio>
#include <vector>

#include "bmm_spec.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<double> x;
    double v;
    while (std::fread(&v, sizeof v, 1, f) == 1) x.push_back(v);
    std::fclose(f);
    for (double& e : x) e = bmm::lgamma_(e);
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const size_t n = std::fwrite(x.data(), sizeof(double), x.size(), f);
    std::fclose(f);
    return n == x.size() ? 0 : 5;
}
