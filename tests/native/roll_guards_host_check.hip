// Host check of the roll step's guards and of the discard table's wide entries (fk_device.h, round 9).  No GPU, no oracle.
//   1. roll_guards50 (the form the game kernels run: whole-word compares on the packed counter words) against roll_guards50_decoded
//      (every field decoded, the limits as engine.py and the record layout state them): every combination of the five guarded values
//      within +-2 of its limit — rolls of the turn 998 ... 1002, turn score / 50 1309 ... 1313, n_rolls 63 999 ... 64 003, smart-five dice
//      and smart-one dice 62 999 ... 63 003 — and of 0 and the field's maximum, with the neighbouring fields of each word at 0 and at
//      their maximum (a compare on the whole word must not see them).
//   2. discard_lut_entry32 against discard_lut_entry on all 2^16 keys: both increments, the points and the dice taken back.
//   3. roll_back_end50w (wide entry) against roll_back_end50 (byte entry) on every key whose choice is not empty and on the empty one:
//      same registers, same results, LEAN and full records.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "../../farkle_ii_amd/csrc/fk_device.h"

using namespace fk;

int main() {
    long cases = 0, bad_guard = 0, seen[3] = {0, 0, 0};
    const uint32_t rolls_turn[] = {0, 998, 999, 1000, 1001, 1002};
    const int32_t turn[] = {0, 1309, 1310, 1311, 1312, 1313};
    const uint32_t n_rolls[] = {0, 63999, 64000, 64001, 64002, 64003, 65535};
    const uint32_t dice[] = {0, 62999, 63000, 63001, 63002, 63003, 65535};
    const uint32_t other[] = {0, 0xffffu}; // the other half of each counter word
    for (uint32_t rt : rolls_turn)
        for (int32_t ts : turn)
            for (uint32_t nr : n_rolls)
                for (uint32_t d5 : dice)
                    for (uint32_t d1 : dice)
                        for (uint32_t o : other) {
                            RollRegs r{nr | (o << 16), o | (o << 16), o | (d5 << 16), o | (d1 << 16), o | (o << 16), 0, 6u, ts};
                            const uint32_t a = roll_guards50(rt, r), b = roll_guards50_decoded(rt, r);
                            ++cases;
                            if (a != b) ++bad_guard;
                            if (b < 3u) ++seen[b];
                        }

    long bad_wide = 0;
    std::vector<uint32_t> nonempty;
    for (uint32_t k = 0; k < DISCARD_LUT_KEYS; ++k) {
        const uint32_t b = discard_lut_entry(k), x = discard_lut_entry32(k), d5 = b & 3u, d1 = (b >> 2) & 3u;
        const bool ok = (x & DW_INC) == ((d5 << 16) | (d5 ? 1u : 0u)) && ((x >> DW_D1_SHIFT) & DW_INC) == ((d1 << 16) | (d1 ? 1u : 0u)) &&
                        ((x >> DW_POINTS_SHIFT) & 0xffu) == d5 + 2u * d1 && (x >> DW_DICE_SHIFT) == d5 + d1 &&
                        (x & ~(DW_INC | (DW_INC << DW_D1_SHIFT) | (0xffu << DW_POINTS_SHIFT) | (0xffu << DW_DICE_SHIFT))) == 0u;
        if (!ok) ++bad_wide;
        if (b != 0u && (nonempty.empty() || discard_lut_entry(nonempty.back()) != b)) nonempty.push_back(k);
    }

    // the two front ends of the back end on the same inputs: score entries of rolls with lone ones and fives, every distinct choice
    long bad_back = 0, back_cases = 0;
    std::vector<uint32_t> entries;
    for (uint32_t key = 1; key < SCORE_LUT_KEYS; ++key) {
        const uint32_t e = score_lut_entry32(key);
        if (e != 0u && (e & SE_SINGLES) && entries.size() < 64) entries.push_back(e);
    }
    nonempty.push_back(0u); // (a key whose entry is the empty choice)
    for (uint32_t e : entries)
        for (uint32_t k : nonempty) {
            const uint32_t b = discard_lut_entry(k), x = discard_lut_entry32(k), d5 = b & 3u, d1 = (b >> 2) & 3u;
            if (d5 > ((e >> 9) & 7u) || d1 > ((e >> 12) & 7u) || d5 + 2u * d1 >= (e & 63u)) continue; // not a choice this roll can get
            for (uint32_t n = (e >> 6) & 7u; n <= 6u; ++n)
                for (uint32_t bits : {0x0f00u, 0x5f00u, 0xef00u})
                    for (int32_t ts : {0, 9, 400})
                        for (int fr = 0; fr < 2; ++fr) {
                            const Strat50 sp{7, bits | 2u};
                            RollRegs a{5u, 3u | (2u << 16), 7u | (9u << 16), 1u | (4u << 16), 40u, 40, n, ts}, w = a;
                            bool oa, ow;
                            const bool ra = roll_back_end50<true>(e, b, n, sp, 0u, fr != 0, 190, a, oa);
                            const bool rw = roll_back_end50w<true>(e, x, n, sp, 0u, fr != 0, 190, w, ow);
                            RollRegs a2{5u, 3u, 7u | (9u << 16), 1u | (4u << 16), 2u, 40, n, ts}, w2 = a2;
                            bool oa2, ow2;
                            const bool ra2 = roll_back_end50<false>(e, b, n, sp, 0u, fr != 0, 190, a2, oa2);
                            const bool rw2 = roll_back_end50w<false>(e, x, n, sp, 0u, fr != 0, 190, w2, ow2);
                            auto same = [](const RollRegs &p, const RollRegs &q) {
                                return p.cA == q.cA && p.cB == q.cB && p.cC == q.cC && p.cD == q.cD && p.cE == q.cE && p.score == q.score &&
                                       p.dice == q.dice && p.turn_score == q.turn_score;
                            };
                            ++back_cases;
                            if (ra != rw || oa != ow || !same(a, w) || ra2 != rw2 || oa2 != ow2 || !same(a2, w2)) ++bad_back;
                        }
        }
    printf("guard cases %ld bad_guard %ld (none %ld roll_limit %ld overflow %ld) wide keys %u bad_wide %ld back_cases %ld bad_back %ld\n", cases, bad_guard,
           seen[0], seen[1], seen[2], DISCARD_LUT_KEYS, bad_wide, back_cases, bad_back);
    const bool all_seen = seen[0] > 0 && seen[1] > 0 && seen[2] > 0 && back_cases > 1000;
    return (bad_guard == 0 && bad_wide == 0 && bad_back == 0 && all_seen) ? 0 : 1;
}
