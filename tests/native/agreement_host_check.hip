// Host program for the per-element rules of csrc/fk_agreement.h (ag_pair_code, cc_row_counts): plain __host__ __device__ C++,
// checked without a GPU and without the oracle.
//   stdin, one case per line:   "p" class win_a win_b ts_a ts_b          -> stdout: the pair's code
//                               "c" m x_0 .. x_{m-1} y_0 .. y_{m-1}      -> stdout: the five counts, every tile of the upper
//                                                                           triangle walked row by row as the kernel walks it
#include <cstdio>
#include <vector>

#include "../../farkle_ii_amd/csrc/fk_kernels.h" // farkle_hip.h's types and what fk_round_robin.h's kernels use
#include "../../farkle_ii_amd/csrc/fk_round_robin.h"
#include "../../farkle_ii_amd/csrc/fk_agreement.h"

int main() {
    char kind[8];
    while (scanf("%7s", kind) == 1) {
        if (kind[0] == 'p') {
            unsigned cls;
            int wa, wb, ta, tb;
            if (scanf("%u %d %d %d %d", &cls, &wa, &wb, &ta, &tb) != 5) return 1;
            printf("%u\n", fkag::ag_pair_code(cls, wa, wb, ta, tb));
        } else if (kind[0] == 'c') {
            unsigned m;
            if (scanf("%u", &m) != 1 || m < 2u) return 1;
            std::vector<int32_t> x(m), y(m);
            for (auto &v : x)
                if (scanf("%d", &v) != 1) return 1;
            for (auto &v : y)
                if (scanf("%d", &v) != 1) return 1;
            const uint32_t T = fkag::CC_TILE, tiles = (m + T - 1u) / T;
            unsigned long long total[fkag::CC_COUNTS] = {0, 0, 0, 0, 0};
            for (uint32_t t = 0; t < tiles * (tiles + 1u) / 2u; ++t) {
                uint32_t bi, bj;
                fkrr::rr_unrank(tiles + 1u, t, bi, bj); // the kernel's tile numbering
                bj -= 1u;
                const uint32_t col0 = bj * T, cols = m - col0 < T ? m - col0 : T;
                for (uint32_t row = bi * T; row < bi * T + T && row < m; ++row) {
                    uint32_t mine[fkag::CC_COUNTS] = {0, 0, 0, 0, 0};
                    fkag::cc_row_counts(x[row], y[row], row, col0, cols, x.data() + col0, y.data() + col0, mine);
                    for (uint32_t k = 0; k < fkag::CC_COUNTS; ++k) total[k] += mine[k];
                }
            }
            printf("%llu %llu %llu %llu %llu\n", total[0], total[1], total[2], total[3], total[4]);
        } else {
            return 1;
        }
    }
    return feof(stdin) ? 0 : 1;
}
