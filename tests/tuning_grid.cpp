// The grid of tests/test_tuning_cpu.py over titan_amd/csrc/tuning.hpp alone: every key in [-1, 40) x 24
// values through tuning_set on one Tuning, in that order; one JSON row per call, in the format of
// tests/golden/tuning_grid.json (the value kept is printed as the readers take it: i64 or f64).
#include <cstdio>
#include <limits>
#include "tuning.hpp"

int main() {
    const double vals[24] = {-2, -1, -0.5, 0, 0.5, 1, 1.5, 2, 15, 16, 1024, 1025, 4096, 4097, 1048576.0, 1048577.0,
                             2147483646.0, 2147483647.0, 9e15, 1e16, 1e18, 1e19,
                             std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()};
    tgo::Tuning t;
    std::string err;
    bool first = true;
    std::printf("[\n");
    for (int key = -1; key < 40; ++key)
        for (double value : vals) {
            const int rc = tgo::tuning_set(t, key, value, err);
            char stored[64];
            if (key < 1 || key >= tgo::kTuneKeys) std::snprintf(stored, sizeof stored, "none");
            else if (tgo::kTuneRows[key].num == tgo::TuneNum::real) std::snprintf(stored, sizeof stored, "%.17g", t.f64(key));
            else std::snprintf(stored, sizeof stored, "%lld", static_cast<long long>(t.i64(key)));
            std::printf("%s{\"key\": %d, \"value\": \"%.17g\", \"rc\": %d, \"err\": \"%s\", \"stored\": \"%s\"}",
                        first ? "" : ",\n", key, value, rc, rc ? err.c_str() : "", stored);
            first = false;
        }
    std::printf("\n]\n");
    return 0;
}
