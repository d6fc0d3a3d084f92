// Host program for the two summation orders of csrc/fk_root_windows.h (walk_column, pairwise_column): plain __host__ __device__ C++,
// checked without a GPU against NumPy itself.
//   stdin, raw, per case:    uint64 R, int64 row_begin, uint64 n_snaps, n_snaps int64 row_end (ascending), then R int64 wins and R int64
//                            exposures of one column (completed = exposures, safety = 0)
//   stdout, raw, per snap:   int64 [6] totals, float64 [3] sums of the sequential walk, float64 [3] sums of the pairwise walk
#include <cstdint>
#include <cstdio>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../farkle_ii_amd/csrc/fk_root_windows.h"

int main() {
    uint64_t head[3];
    while (fread(head, 8, 3, stdin) == 3) {
        const uint64_t R = head[0], n_snaps = head[2];
        const int64_t row_begin = (int64_t)head[1];
        if (R > ((uint64_t)1 << 26) || n_snaps < 1 || n_snaps > 64) return 1;
        std::vector<int64_t> ends((size_t)n_snaps), w((size_t)R), e((size_t)R), zero((size_t)R, 0);
        if (fread(ends.data(), 8, ends.size(), stdin) != ends.size()) return 1;
        if (fread(w.data(), 8, w.size(), stdin) != w.size() || fread(e.data(), 8, e.size(), stdin) != e.size()) return 1;
        std::vector<fkw::Snap> snaps;
        for (size_t i = 0; i < ends.size(); ++i) {
            if (ends[i] <= row_begin || (uint64_t)ends[i] > R || (i && ends[i] < ends[i - 1])) return 1;
            snaps.push_back(fkw::Snap{ends[i], (uint32_t)i, 1u}); // one column, S = 1, pairwise_begin = 1: the walk stores its float sums
        }
        std::vector<long long> totals(snaps.size() * fkw::N_TOTALS);
        std::vector<double> sequential(snaps.size() * fkw::N_SUMS), pairwise(snaps.size() * fkw::N_SUMS);
        fkw::walk_column(w.data(), e.data(), e.data(), zero.data(), 1, 0, row_begin, snaps.data(), (uint32_t)snaps.size(), totals.data(), sequential.data());
        for (size_t i = 0; i < snaps.size(); ++i) {
            fkw::pairwise_column(w.data(), e.data(), 1, 0, row_begin, ends[i], (uint32_t)i, pairwise.data());
            if (fwrite(totals.data() + i * fkw::N_TOTALS, 8, fkw::N_TOTALS, stdout) != fkw::N_TOTALS) return 1;
            if (fwrite(sequential.data() + i * fkw::N_SUMS, 8, fkw::N_SUMS, stdout) != fkw::N_SUMS) return 1;
            if (fwrite(pairwise.data() + i * fkw::N_SUMS, 8, fkw::N_SUMS, stdout) != fkw::N_SUMS) return 1;
        }
    }
    return feof(stdin) ? 0 : 1;
}
