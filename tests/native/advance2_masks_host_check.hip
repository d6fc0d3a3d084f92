// Host-side check of the two-seat table advance on lane masks in farkle_ii_amd/csrc/fk_device.h (no GPU calls): advance2_flags50 on
// lanes_t, the form the two-seat lean game kernels run since they carry the game flags as 64-lane masks, against advance2_table50, lane
// by lane (and its one-lane form, on bool, against both).
//   every combination of the five booleans the rule reads (turn over, target reached, rounds at the limit, owner is seat 1, final round)
//   x max_rounds {0, 1, 2} x rounds {max_rounds - 1 (where there is one), max_rounds, max_rounds + 1}: for each the 32 boolean cases are
//   packed into 64-lane masks (two lanes per case) in three lane orders (identity, reversed, a stride-37 permutation), so a mask
//   operation that mixed up lanes or leaked one lane's bit into another's would be seen.  `rounds at the limit` is not free: it is the
//   compare of rounds with max_rounds, so the boolean picks among the rounds values on either side of the limit.
// Compared per lane: ended, turn passes, the final-round flag, rounds, score_to_beat (through the trigger mask), the seat after the
// advance.  Built and run by tests/test_advance2_masks_host.py with hipcc (host compilation only), once more under the address and
// undefined-behaviour sanitizers.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../farkle_ii_amd/csrc/fk_device.h"

using namespace fk;

namespace {

constexpr int32_t TARGET50 = 200;

uint32_t lane_of(int order, uint32_t i) { // a permutation of 0..63
    return order == 0 ? i : order == 1 ? 63u - i : (i * 37u + 11u) & 63u;
}

} // namespace

int main() {
    long cases = 0, bad = 0, ended_n = 0, sw_n = 0, trig_n = 0, closes_n = 0;
    for (uint32_t max_rounds = 0; max_rounds <= 2; ++max_rounds)
        for (int rounds_pick = 0; rounds_pick < 2; ++rounds_pick) // which value on each side of the limit
            for (int order = 0; order < 3; ++order) {
                // lane i carries boolean case i >> 1 (both lanes of a pair the same case, the odd one with another score below / above the target)
                uint32_t rounds[64], seat[64], fr[64];
                int32_t score[64], stb[64];
                bool over[64];
                lanes_t m_over = 0, m_reached = 0, m_limit = 0, m_seat1 = 0, m_final = 0;
                for (uint32_t i = 0; i < 64; ++i) {
                    const uint32_t l = lane_of(order, i), c = i >> 1;
                    over[l] = c & 1u, seat[l] = (c >> 1) & 1u, fr[l] = (c >> 2) & 1u;
                    const bool reached = (c >> 3) & 1u, at_limit = (c >> 4) & 1u;
                    score[l] = reached ? TARGET50 + (int32_t)(i & 1u) * 7 : TARGET50 - 1 - (int32_t)(i & 1u) * 150;
                    // below the limit: max_rounds - 1 (or the limit itself is unreachable with max_rounds 0: then every value is at or above it)
                    if (at_limit) rounds[l] = rounds_pick ? max_rounds + 1u : max_rounds;
                    else rounds[l] = max_rounds == 0u ? 0u : rounds_pick && max_rounds > 1u ? max_rounds - 2u : max_rounds - 1u;
                    stb[l] = fr[l] ? 230 : TARGET50;
                    const lanes_t bit = 1ull << l;
                    m_over |= over[l] ? bit : 0ull, m_seat1 |= seat[l] ? bit : 0ull, m_final |= fr[l] ? bit : 0ull;
                    m_reached |= score[l] >= TARGET50 ? bit : 0ull;
                    m_limit |= rounds[l] >= max_rounds ? bit : 0ull; // (max_rounds 0: set whatever the case asked for, as in the kernel)
                }
                const Advance2Flags<lanes_t> m = advance2_flags50<lanes_t>(m_over, m_reached, m_limit, m_seat1, m_final);
                const lanes_t seat1_after = m_seat1 ^ m.sw;
                for (uint32_t l = 0; l < 64; ++l) {
                    Table2 t{seat[l], rounds[l], 0u, fr[l], 0u, stb[l]};
                    const Advance2 want = advance2_table50(over[l], score[l], TARGET50, max_rounds, t);
                    const bool ended = (m.ended >> l) & 1u, sw = (m.sw >> l) & 1u, trig = (m.trig >> l) & 1u, closes = (m.closes >> l) & 1u;
                    const Advance2Flags<bool> one = advance2_flags50<bool>(over[l], score[l] >= TARGET50, rounds[l] >= max_rounds, seat[l] != 0u, fr[l] != 0u);
                    if (one.ended != ended || one.sw != sw || one.trig != trig || one.closes != closes || one.in_final != (bool)((m.in_final >> l) & 1u)) ++bad;
                    const uint32_t rounds_after = rounds[l] + (closes ? 1u : 0u);
                    const int32_t stb_after = trig ? score[l] : stb[l];
                    ++cases;
                    ended_n += ended, sw_n += sw, trig_n += trig, closes_n += closes;
                    if (ended != want.ended || sw != want.sw || (uint32_t)((m.in_final >> l) & 1u) != t.final_round || rounds_after != t.rounds ||
                        stb_after != t.score_to_beat || (uint32_t)((seat1_after >> l) & 1u) != t.seat) {
                        if (++bad <= 10)
                            std::printf("MISMATCH max_rounds %u order %d lane %u: over %d seat %u fr %u score %d rounds %u -> ended %d/%d sw %d/%d fr %d/%u "
                                        "rounds %u/%u stb %d/%d\n", max_rounds, order, l, (int)over[l], seat[l], fr[l], score[l], rounds[l], (int)ended,
                                        (int)want.ended, (int)sw, (int)want.sw, (int)((m.in_final >> l) & 1u), t.final_round, rounds_after, t.rounds,
                                        stb_after, t.score_to_beat);
                    }
                }
            }
    std::printf("cases %ld ended %ld sw %ld trig %ld closes %ld bad %ld\n", cases, ended_n, sw_n, trig_n, closes_n, bad);
    return bad == 0 && ended_n && sw_n && trig_n && closes_n ? 0 : 1;
}
