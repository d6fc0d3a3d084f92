// Host program for the statistics of csrc/fk_rr_inference.h (ri_score_test, ri_stat_at, ri_interval): plain __host__ __device__ C++,
// checked without a GPU and without the oracle.
//   stdin, one case per line:   count1 nobs1 count2 nobs2 critical_value        (the critical value as a C99 hex double)
//   stdout, one line per case:  z difference null_proportion | the statistic at the five differences below | low high of the
//                               interval, low high of the interval with the two samples exchanged        (twelve hex doubles)
#include <cstdio>
#include <cstdlib>

#include "../../farkle_ii_amd/csrc/fk_kernels.h" // farkle_hip.h's types and what fk_round_robin.h's kernels use
#include "../../farkle_ii_amd/csrc/fk_round_robin.h"
#include "../../farkle_ii_amd/csrc/fk_rr_inference.h"

static const double DIFFERENCES[5] = {-0.5, -0.0625, 0.0, 0.03, 0.75};

int main() {
    long long c1, n1, c2, n2;
    char crit_text[64];
    while (scanf("%lld %lld %lld %lld %63s", &c1, &n1, &c2, &n2, crit_text) == 5) {
        if (n1 <= 0 || n2 <= 0 || c1 < 0 || c2 < 0 || c1 > n1 || c2 > n2) return 2;
        const double crit = strtod(crit_text, nullptr);
        const fkri::Score s = fkri::ri_score_test(c1, n1, c2, n2);
        printf("%a %a %a", s.z, s.difference, s.null_proportion);
        for (double d : DIFFERENCES) printf(" %a", fkri::ri_stat_at(c1, n1, c2, n2, d));
        double low, high, low_x, high_x;
        fkri::ri_interval(c1, n1, c2, n2, crit, low, high);
        fkri::ri_interval(c2, n2, c1, n1, crit, low_x, high_x);
        printf(" %a %a %a %a\n", low, high, low_x, high_x);
    }
    return feof(stdin) ? 0 : 1;
}
