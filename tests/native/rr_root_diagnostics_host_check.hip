// Host program for the per-pair rules of csrc/fk_rr_root_diagnostics.h (rd_decision, rd_agreement): plain __host__ __device__ C++,
// checked without a GPU and without the oracle.
//   stdin, one case per line:   effect_a decision_a effect_b decision_b holm_reject      (the effects as C99 hex doubles or "nan")
//   stdout, one line per case:  discrepancy absolute flags | rd_decision(holm_reject, effect_a)
#include <cstdio>
#include <cstdlib>

#include "../../farkle_ii_amd/csrc/fk_kernels.h" // farkle_hip.h's types and what fk_round_robin.h's kernels use
#include "../../farkle_ii_amd/csrc/fk_round_robin.h"
#include "../../farkle_ii_amd/csrc/fk_rr_inference.h"
#include "../../farkle_ii_amd/csrc/fk_rr_root_diagnostics.h"

int main() {
    char a_text[64], b_text[64];
    unsigned decision_a, decision_b, reject;
    while (scanf("%63s %u %63s %u %u", a_text, &decision_a, b_text, &decision_b, &reject) == 5) {
        const double a = strtod(a_text, nullptr), b = strtod(b_text, nullptr);
        const fkri::Agreement g = fkri::rd_agreement(a, decision_a, b, decision_b);
        printf("%a %a %u %u\n", g.discrepancy, g.absolute, g.flags, fkri::rd_decision(reject != 0u, a));
    }
    return feof(stdin) ? 0 : 1;
}
