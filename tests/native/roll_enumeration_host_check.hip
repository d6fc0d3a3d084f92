// Host check of the exact ordered-roll law (fk_device.h).  No GPU, no oracle.
//   score_counts — the SWAR scorer the roll census takes a roll's raw cell from, and the rule the score table is built by — over all
//   6^d ordered outcomes of d = 1 .. 6 dice.  Prints one line per non-empty cell, in ascending (dice, score, used):
//       cell <dice> <max immediate score> <scoring dice> <ordered outcomes>
//   and one line per dice count: total <dice> <ordered outcomes> <farkles>.  tests/test_roll_enumeration_host.py compares the cells
//   with the reference's enumeration (tests/golden/roll_enumeration.json).
#include <cstdint>
#include <cstdio>

#include "../../farkle_ii_amd/csrc/fk_device.h"

using namespace fk;

int main() {
    for (uint32_t d = 1; d <= 6; ++d) {
        static long cells[61][7];
        for (auto &row : cells)
            for (long &v : row) v = 0;
        long outcomes = 1, bad = 0;
        for (uint32_t i = 0; i < d; ++i) outcomes *= 6;
        for (long o = 0; o < outcomes; ++o) {
            uint32_t counts = 0; // nibble-packed face counts, face 1 in the low nibble
            long rest = o;
            for (uint32_t i = 0; i < d; ++i) {
                counts += 1u << (4u * (uint32_t)(rest % 6));
                rest /= 6;
            }
            const RawScore r = score_counts(counts);
            if (r.score < 0 || r.score > 3000 || r.score % 50 != 0 || r.used < 0 || r.used > (int32_t)d) {
                ++bad;
                continue;
            }
            cells[r.score / 50][r.used] += 1;
        }
        for (int s = 0; s < 61; ++s)
            for (int u = 0; u < 7; ++u)
                if (cells[s][u]) printf("cell %u %d %d %ld\n", d, s * 50, u, cells[s][u]);
        long farkles = 0;
        for (int u = 0; u < 7; ++u) farkles += cells[0][u];
        printf("total %u %ld %ld\n", d, outcomes, farkles);
        printf("bad %u %ld\n", d, bad);
    }
    return 0;
}
