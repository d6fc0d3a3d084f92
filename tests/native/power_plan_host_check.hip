// Host program for the count boundaries of csrc/fk_power_plan.h (pp_boundaries): plain __host__ __device__ C++, checked without a GPU
// and without the reference.
//   stdin, one case per line:   n critical_squared (a float in any form strtod reads; the test sends the hex of the bits)
//   stdout, per case, raw:      int32 lower[n + 1], then int32 upper[n + 1]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/farkle_hip.h"
#include "../../farkle_ii_amd/csrc/fk_power_plan.h"

int main() {
    int n;
    char text[64];
    while (scanf("%d %63s", &n, text) == 2) {
        if (n < 1 || n > FK_POWER_MAX_N) return 1;
        const double critical_squared = strtod(text, nullptr);
        std::vector<int32_t> lower((size_t)n + 1), upper((size_t)n + 1);
        for (int c1 = 0; c1 <= n; ++c1) fkpp::pp_boundaries(n, critical_squared, c1, lower[c1], upper[c1]);
        if (fwrite(lower.data(), 4, lower.size(), stdout) != lower.size() || fwrite(upper.data(), 4, upper.size(), stdout) != upper.size()) return 1;
    }
    return feof(stdin) ? 0 : 1;
}
