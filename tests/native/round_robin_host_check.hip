// Host program for rr_unrank (csrc/fk_round_robin.h): the pair numbering of the round robin, checked without a GPU and without the oracle.
//   stdin, one table size per line:  n mode      mode 0: every pair of the table, by enumeration; mode 1: the first and last pair of every row
//   stdout, one line per table:      n pairs_checked mismatches
// A mismatch is a pair id whose rr_unrank differs from the enumeration's (i, j), i < j in lexicographic order.
#include <cstdio>

#include "../../farkle_ii_amd/csrc/fk_kernels.h" // DevBlock and the wave helpers the header's kernels use
#include "../../farkle_ii_amd/csrc/fk_round_robin.h"

int main() {
    long long n;
    int mode;
    while (scanf("%lld %d", &n, &mode) == 2) {
        if (n < 2 || n > 0x7fffffffLL) return 2;
        unsigned long long checked = 0, bad = 0, pid = 0;
        for (long long i = 0; i + 1 < n; ++i) {
            if (mode == 0) {
                for (long long j = i + 1; j < n; ++j, ++pid, ++checked) {
                    uint32_t gi, gj;
                    fkrr::rr_unrank((uint32_t)n, pid, gi, gj);
                    bad += (gi != (uint32_t)i || gj != (uint32_t)j) ? 1u : 0u;
                }
            } else {
                const unsigned long long first = pid, last = pid + (unsigned long long)(n - i - 2);
                const long long js[2] = {i + 1, n - 1};
                const unsigned long long ids[2] = {first, last};
                for (int q = 0; q < 2; ++q, ++checked) {
                    uint32_t gi, gj;
                    fkrr::rr_unrank((uint32_t)n, ids[q], gi, gj);
                    bad += (gi != (uint32_t)i || gj != (uint32_t)js[q]) ? 1u : 0u;
                }
                pid = last + 1;
            }
        }
        if (pid != (unsigned long long)n * (unsigned long long)(n - 1) / 2u) return 3; // the enumeration itself
        printf("%lld %llu %llu\n", n, checked, bad);
    }
    return feof(stdin) ? 0 : 1;
}
