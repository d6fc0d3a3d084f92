// Host check of the two-seat game end in its round-11 form (fk_device.h).  No GPU, no oracle.
//   finish2_50 = finish2_second (who won, from the two cE words) + finish2_50_winner (the metrics, from the winner's five words) against
//   finish2_50_decoded (every field of both seats decoded, then picked):
//     - one record over EVERY combination of its nine 16-bit fields at 0, 1, the guard-band limit where the field has one (fk_device.h:
//       RG_N_ROLLS, RG_TURN50, RG_DICE; a banked total of RG_TURN50 for the score) and 0xffff, as seat 0 and as seat 1;
//     - against an opponent record whose fields walk through the same values out of step, with a lower, an equal and a higher score
//       (both winners, and the tie that seat 0 wins);
//     - final_round 0 / 1, and the round count at 0, 1 and 65 535.
//   finish2_square (the tally's sums of squares: one 32-bit product for the eight metrics that are 16-bit fields or the round count, the
//   64-bit product for the two point-valued ones) against the 64-bit product, on every metric of every case above and at the maxima.
#include <cstdio>
#include <cstdint>

#include "../../farkle_ii_amd/csrc/fk_device.h"

using namespace fk;

// the bounds stated beside finish2_square
static_assert(65535ull * 65535ull < (1ull << 32), "a 16-bit metric's square fits 32 bits");
static_assert(65535u * 50u < (1u << 24), "a point-valued metric fits the 24-bit multiply's operand");
static_assert(FINISH2_POINT_METRICS == 0x11u, "m[0] (winning score) and m[4] (highest turn) are the point-valued metrics");

static bool same(const Finish2 &x, const Finish2 &y) {
    if (x.completed != y.completed || x.winner != y.winner || x.widx != y.widx) return false;
    for (int j = 0; j < 10; ++j)
        if (x.m[j] != y.m[j]) return false;
    return true;
}

int main() {
    const uint32_t score[] = {0, 1, RG_TURN50, 65535}, rolls[] = {0, 1, RG_N_ROLLS, 65535}, highest[] = {0, 1, RG_TURN50, 65535};
    const uint32_t dice[] = {0, 1, RG_DICE, 65535}, plain[] = {0, 1, 65535};
    const uint32_t idx[] = {0, 63, (1u << (32 - LEAN_IDX_SHIFT)) - 1u}, flags[] = {0, 3};
    const uint32_t round_counts[] = {0, 1, 65535};
    long cases = 0, bad = 0, bad_tie = 0, bad_metric = 0, bad_square = 0, wins[2] = {0, 0}, ties = 0, completed = 0;
    // the record under test from its nine field indices; cE's score comes separately
    auto record = [&](const uint32_t *f, uint32_t sc, uint32_t n) {
        LeanCounters r;
        r.cA = rolls[f[0]] | (plain[f[1]] << 16);    // rolls | farkles
        r.cB = highest[f[2]] | (plain[f[3]] << 16);  // highest turn / 50 | hot dice
        r.cC = plain[f[4]] | (dice[f[5]] << 16);     // smart-five uses | dice
        r.cD = plain[f[6]] | (dice[f[7]] << 16);     // smart-one uses | dice
        r.cE = sc | (flags[n % 2u] << 16) | (idx[n % 3u] << LEAN_IDX_SHIFT);
        return r;
    };
    const uint32_t radix[9] = {4, 3, 4, 3, 3, 4, 3, 4, 4}; // the last digit is the score
    uint32_t f[9] = {0};
    uint32_t n = 0;
    for (bool more = true; more; ++n) {
        const uint32_t sc = score[f[8]];
        const LeanCounters rec = record(f, sc, n);
        // the opponent: every field index shifted by a per-field stride, so its values differ from the record's in every field
        uint32_t g[9];
        for (int i = 0; i < 9; ++i) g[i] = (f[i] + 1u + (n >> i) % (radix[i] - 1u)) % radix[i];
        const uint32_t lower = sc == 0u ? 0u : sc - 1u, higher = sc == 65535u ? 65535u : sc + 1u;
        for (uint32_t other_score : {lower, sc, higher}) {
            const LeanCounters opp = record(g, other_score, n + 1u);
            for (int as_seat = 0; as_seat < 2; ++as_seat)
                for (uint32_t fr = 0; fr < 2; ++fr)
                    for (uint32_t rounds : round_counts) {
                        const LeanCounters &a = as_seat == 0 ? rec : opp, &b = as_seat == 0 ? opp : rec;
                        const uint32_t max_rounds = rounds == 0u ? (fr ? 1u : 0u) : rounds; // (a final round needs a round)
                        const Finish2 x = finish2_50(a, b, rounds, fr, max_rounds);
                        const Finish2 y = finish2_50_decoded(a, b, rounds, fr, max_rounds);
                        ++cases;
                        if (!same(x, y)) ++bad;
                        const uint32_t sa = a.cE & 0xffffu, sb = b.cE & 0xffffu;
                        if (sa == sb) {
                            ++ties;
                            if (x.winner != 0u) ++bad_tie;
                        }
                        wins[x.winner] += 1;
                        if (x.completed) ++completed;
                        if (finish2_second(a.cE, b.cE) != (sb > sa)) ++bad;
                        const LeanCounters &w = (sb > sa) ? b : a; // the metrics are the winner's own fields, stated without either function
                        if (x.m[0] != (w.cE & 0xffffu) * 50u || x.m[1] != rounds || x.m[2] != (w.cA >> 16) || x.m[3] != (w.cA & 0xffffu) ||
                            x.m[4] != (w.cB & 0xffffu) * 50u || x.m[5] != (w.cC & 0xffffu) || x.m[6] != (w.cC >> 16) || x.m[7] != (w.cD & 0xffffu) ||
                            x.m[8] != (w.cD >> 16) || x.m[9] != (w.cB >> 16) || x.widx != (w.cE >> LEAN_IDX_SHIFT))
                            ++bad_metric;
                        for (uint32_t j = 0; j < 10; ++j)
                            if (finish2_square(j, x.m[j]) != (uint64_t)x.m[j] * x.m[j]) ++bad_square;
                    }
        }
        more = false; // next combination (odometer)
        for (int i = 0; i < 9; ++i) {
            if (++f[i] < radix[i]) {
                more = true;
                break;
            }
            f[i] = 0;
        }
    }
    // the squares at the maxima, one metric at a time: 16-bit metrics at 65 535, point-valued ones at 65 535 * 50
    long maxima = 0;
    for (uint32_t j = 0; j < 10; ++j) {
        const bool points = (FINISH2_POINT_METRICS >> j) & 1u;
        for (uint32_t v : {0u, 1u, 65534u, 65535u, points ? 65535u * 50u : 65535u, points ? 65534u * 50u : 46341u}) { // (46 341^2 > 2^31)
            ++maxima;
            if (finish2_square(j, v) != (uint64_t)v * v) ++bad_square;
        }
        if (!points && (finish2_square(j, 65535u) >> 32) != 0u) ++bad_square; // the addend's high half is zero
    }
    printf("finish2_short records %u cases %ld bad %ld ties %ld bad_tie %ld bad_metric %ld bad_square %ld (seat0 wins %ld seat1 wins %ld completed %ld maxima %ld)\n",
           n, cases, bad, ties, bad_tie, bad_metric, bad_square, wins[0], wins[1], completed, maxima);
    const bool all_seen = n == 4u * 3u * 4u * 3u * 3u * 4u * 3u * 4u * 4u && ties > 0 && wins[0] > ties && wins[1] > 0 && completed > 0 && completed < cases;
    return (bad == 0 && bad_tie == 0 && bad_metric == 0 && bad_square == 0 && all_seen) ? 0 : 1;
}
