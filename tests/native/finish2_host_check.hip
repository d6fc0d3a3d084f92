// Host check of the two-seat game end (fk_device.h, round 10).  No GPU, no oracle.
//   finish2_50 (the form the two-seat lean game kernels run: the winner's five counter words are picked, then decoded) against
//   finish2_50_decoded (every field of both seats decoded, then picked), on lean records whose fields are each at 0, at 1, at their
//   guard-band maximum (fk_device.h: RG_*; the banked total stays below 65 536 / 50) and at the field's 16-bit maximum:
//     - equal scores: seat 0 wins the tie, at every score value;
//     - every metric at 0 and at its maximum, for the winner and for the loser (a metric of the loser must not leak);
//     - a game that ended in its final round against one that ended at the round limit; a game with max_rounds 0 (no round, no winner);
//     - strategy indices at 0, at the 14-bit maximum, and different between the seats; the flag bits of cE set and clear.
#include <cstdio>
#include <cstdint>

#include "../../farkle_ii_amd/csrc/fk_device.h"

using namespace fk;

static bool same(const Finish2 &x, const Finish2 &y) {
    if (x.completed != y.completed || x.winner != y.winner || x.widx != y.widx) return false;
    for (int j = 0; j < 10; ++j)
        if (x.m[j] != y.m[j]) return false;
    return true;
}

int main() {
    const uint32_t score[] = {0, 1, 199, 200, 1310, 65535};          // / 50; 65 535 = the field's maximum
    const uint32_t rolls[] = {0, RG_N_ROLLS, 65535}, farkles[] = {0, 65535};
    const uint32_t highest[] = {0, RG_TURN50, 65535}, hot[] = {0, 65535};
    const uint32_t uses[] = {0, 65535}, dice[] = {0, RG_DICE, 65535};
    const uint32_t idx[] = {0, 63, (1u << (32 - LEAN_IDX_SHIFT)) - 1u}, flags[] = {0, 3};
    long cases = 0, bad = 0, ties = 0, bad_tie = 0, completed = 0, limit = 0, no_rounds = 0, bad_metric = 0;
    // one seat's record from a case number: the fields cycle independently through their values
    auto record = [&](uint32_t n, uint32_t sc) {
        LeanCounters r;
        r.cA = rolls[n % 3u] | (farkles[(n / 3u) % 2u] << 16);
        r.cB = highest[(n / 6u) % 3u] | (hot[(n / 18u) % 2u] << 16);
        r.cC = uses[(n / 36u) % 2u] | (dice[(n / 72u) % 3u] << 16);
        r.cD = uses[(n / 216u) % 2u] | (dice[(n / 432u) % 3u] << 16);
        r.cE = sc | (flags[(n / 1296u) % 2u] << 16) | (idx[(n / 2592u) % 3u] << LEAN_IDX_SHIFT);
        return r;
    };
    constexpr uint32_t RECORDS = 7776; // 3 * 2 * 3 * 2 * 2 * 3 * 2 * 3 * 2 * 3
    struct End {
        uint32_t rounds, final_round, max_rounds;
    };
    const End ends[] = {{1, 1, 200}, {200, 1, 200}, {200, 0, 200}, {1, 0, 1}, {0, 0, 0}, {65535, 1, 65535}};
    for (uint32_t s0 : score)
        for (uint32_t s1 : score)
            for (uint32_t n0 = 0; n0 < RECORDS; n0 += 7u)       // (strides coprime to every cycle length: all values of every field are met,
                for (uint32_t n1 = 0; n1 < RECORDS; n1 += 211u) //  in many combinations with the other seat's)
                    for (const End &e : ends) {
                        const LeanCounters a = record(n0, s0), b = record(n1, s1);
                        const Finish2 x = finish2_50(a, b, e.rounds, e.final_round, e.max_rounds);
                        const Finish2 y = finish2_50_decoded(a, b, e.rounds, e.final_round, e.max_rounds);
                        ++cases;
                        if (!same(x, y)) ++bad;
                        if (s0 == s1) {
                            ++ties;
                            if (x.winner != 0u) ++bad_tie;
                        }
                        if (x.completed) ++completed;
                        else if (e.max_rounds == 0u) ++no_rounds;
                        else ++limit;
                        // the metrics are the winner's own fields, stated once more without either function
                        const LeanCounters &w = (s1 > s0) ? b : a;
                        if (x.m[0] != (w.cE & 0xffffu) * 50u || x.m[1] != e.rounds || x.m[2] != (w.cA >> 16) || x.m[3] != (w.cA & 0xffffu) ||
                            x.m[4] != (w.cB & 0xffffu) * 50u || x.m[5] != (w.cC & 0xffffu) || x.m[6] != (w.cC >> 16) || x.m[7] != (w.cD & 0xffffu) ||
                            x.m[8] != (w.cD >> 16) || x.m[9] != (w.cB >> 16) || x.widx != (w.cE >> LEAN_IDX_SHIFT))
                            ++bad_metric;
                    }
    printf("finish2 cases %ld bad %ld ties %ld bad_tie %ld bad_metric %ld (completed %ld round_limit %ld no_rounds %ld)\n", cases, bad, ties, bad_tie,
           bad_metric, completed, limit, no_rounds);
    const bool all_seen = ties > 0 && completed > 0 && limit > 0 && no_rounds > 0 && cases > 100000;
    return (bad == 0 && bad_tie == 0 && bad_metric == 0 && all_seen) ? 0 : 1;
}
