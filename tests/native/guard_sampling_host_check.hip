// Host check of the sampled guard bands of the two-seat lean instances (fk_device.h, round 12).  No GPU, no oracle.
// The instances test the three u16 bands (n_rolls, sf_dice, so_dice) every K = RG_SAMPLE_TRIPS trips (sampled_overflow50) and where a game
// ends (game_end_overflow50); the roll limit and the turn-score band stay in every roll (roll_guards50_turn).
//   1. sampled_overflow50 and roll_guards50_turn together are roll_guards50: on every combination of the five guarded values within +-2
//      of its limit, of 0 and of the field's maximum, with the neighbouring halves at 0 and at their maximum.
//   2. K rolls of worst-case growth through roll_back_end50w (a roll, a farkle or not, two returned fives and two returned ones: the most
//      a discard entry holds — and, stated apart, six dice per roll, more than any entry holds), every field started within +-2 of its
//      band and of 65 535 - 6 K: a record that passed a test does not wrap before the next one (the field never decreases and never
//      exceeds 65 535), and a record beyond a band at any roll of the window is still beyond it — flagged — at the window's end.
//   3. The game's end: game_end_overflow50 flags a state iff a field of EITHER record is beyond its band (the loser's included), or
//      highest_turn is; and highest_turn never exceeds 60 units x 1 000 rolls, so it fits its 16 bits wherever the per-roll test let it.
#include <cstdio>
#include <cstdint>

#include "../../farkle_ii_amd/csrc/fk_device.h"

using namespace fk;

int main() {
    constexpr uint32_t K = RG_SAMPLE_TRIPS;
    long cases = 0, bad_split = 0;
    const uint32_t rolls_turn[] = {0, 998, 999, 1000, 1001, 1002};
    const int32_t turn[] = {0, 1309, 1310, 1311, 1312, 1313};
    const uint32_t n_rolls[] = {0, 63999, 64000, 64001, 64002, 64003, 65535};
    const uint32_t dice[] = {0, 62999, 63000, 63001, 63002, 63003, 65535};
    const uint32_t other[] = {0, 0xffffu};
    for (uint32_t rt : rolls_turn)
        for (int32_t ts : turn)
            for (uint32_t nr : n_rolls)
                for (uint32_t d5 : dice)
                    for (uint32_t d1 : dice)
                        for (uint32_t o : other) {
                            const RollRegs r{nr | (o << 16), o | (o << 16), o | (d5 << 16), o | (d1 << 16), o | (o << 16), 0, 6u, ts};
                            const uint32_t whole = roll_guards50_decoded(rt, r), part = roll_guards50_turn(rt, r);
                            const bool sampled = sampled_overflow50(r.cA, r.cC, r.cD);
                            // the roll limit first, then any band: the two halves together say what the whole says
                            const uint32_t both = part == RG_ROLL_LIMIT ? (uint32_t)RG_ROLL_LIMIT : (part == RG_OVERFLOW || sampled) ? (uint32_t)RG_OVERFLOW : (uint32_t)RG_NONE;
                            ++cases;
                            if (both != whole) ++bad_split;
                            const bool bands = nr > RG_N_ROLLS || d5 > RG_DICE || d1 > RG_DICE;
                            if (sampled != bands) ++bad_split;
                        }

    // 2. a window of K rolls from every start; the discard entry that returns the most dice (d5 = d1 = 2, both use counters counted)
    long windows = 0, wrapped = 0, missed = 0, grew_more = 0;
    uint32_t worst = 0; // the wide entry with the largest increments of cC and cD
    for (uint32_t k = 0; k < DISCARD_LUT_KEYS; ++k) {
        const uint32_t x = discard_lut_entry32(k);
        if ((x & DW_INC) + ((x >> DW_D1_SHIFT) & DW_INC) > (worst & DW_INC) + ((worst >> DW_D1_SHIFT) & DW_INC)) worst = x;
    }
    const uint32_t worst5 = (worst & DW_INC) >> 16, worst1 = ((worst >> DW_D1_SHIFT) & DW_INC) >> 16;
    uint32_t e_score = 0; // a score entry with enough lone ones and fives for that choice, six dice
    for (uint32_t key = 1; key < SCORE_LUT_KEYS && !e_score; ++key) {
        const uint32_t e = score_lut_entry32(key);
        if (e && ((e >> 9) & 7u) >= worst5 && ((e >> 12) & 7u) >= worst1 && (e & 63u) >= worst5 + 2u * worst1) e_score = e; // (growth is the point: no roll may leave itself nothing)
    }
    const uint32_t starts_rolls[] = {RG_N_ROLLS - 2, RG_N_ROLLS - 1, RG_N_ROLLS, 65535 - 6 * K - 2, 65535 - 6 * K - 1, 65535 - 6 * K, 65535 - K};
    const uint32_t starts_dice[] = {RG_DICE - 2, RG_DICE - 1, RG_DICE, 65535 - 6 * K - 2, 65535 - 6 * K - 1, 65535 - 6 * K};
    for (uint32_t nr : starts_rolls)
        for (uint32_t d5 : starts_dice)
            for (uint32_t d1 : starts_dice)
                for (int farkle = 0; farkle < 2; ++farkle) {
                    // (a record that passed the last test holds at most the bands; the starts above them are further than any record gets)
                    RollRegs r{nr, 0u, d5 << 16, d1 << 16, BE_HAS_SCORED, 0, 6u, 0};
                    const Strat50 sp{7, 0x0f00u | 2u};
                    bool beyond = false, of;
                    uint32_t p_rolls = nr, p5 = d5, p1 = d1;
                    for (uint32_t t = 0; t < K; ++t) {
                        r.turn_score = 0;
                        (void)roll_back_end50w<true>(farkle ? 0u : e_score, farkle ? 0u : worst, 6u, sp, 0u, false, 190, r, of);
                        const uint32_t a = r.cA & 0xffffu, c = r.cC >> 16, d = r.cD >> 16;
                        if (a < p_rolls || c < p5 || d < p1) ++wrapped; // a field that wrapped went down
                        if (a - p_rolls > 1u || c - p5 > 6u || d - p1 > 6u) ++grew_more; // the growth the argument assumes
                        p_rolls = a, p5 = c, p1 = d;
                        beyond = beyond || a > RG_N_ROLLS || c > RG_DICE || d > RG_DICE;
                    }
                    ++windows;
                    if (beyond != sampled_overflow50(r.cA, r.cC, r.cD)) ++missed; // whatever went beyond inside the window is seen at its end
                }
    // ... and the bound stated apart from any table entry: band + 6 K stays a u16
    const bool bound = RG_N_ROLLS + K <= 65535u && RG_DICE + 6u * K <= 65535u && worst5 + worst1 <= 6u;

    // 3. the game's end
    long ends = 0, bad_end = 0;
    const uint32_t highest[] = {0, RG_TURN50 - 1, RG_TURN50, RG_TURN50 + 1, RG_TURN50 + 2, 60000, 65535};
    for (int loser = 0; loser < 2; ++loser) // which record holds the field under test; the other one is an ordinary record
        for (uint32_t nr : n_rolls)
            for (uint32_t d5 : dice)
                for (uint32_t d1 : dice)
                    for (uint32_t hi : highest)
                        for (uint32_t o : other) {
                            const LeanCounters x{nr | (o << 16), hi | (o << 16), o | (d5 << 16), o | (d1 << 16), 40u | (o << 16)}, y{17u, 9u, 3u, 2u, 200u};
                            const bool want = nr > RG_N_ROLLS || d5 > RG_DICE || d1 > RG_DICE || hi > RG_TURN50;
                            const bool got = loser ? game_end_overflow50(y, x) : game_end_overflow50(x, y);
                            ++ends;
                            if (got != want) ++bad_end;
                        }
    const bool highest_fits = 60u * RG_TURN_ROLLS <= 65535u; // a roll scores at most 3 000 points = 60 units

    printf("split cases %ld bad_split %ld windows %ld wrapped %ld grew_more %ld missed %ld bound %d ends %ld bad_end %ld highest_fits %d (K %u, worst entry d5 %u d1 %u)\n",
           cases, bad_split, windows, wrapped, grew_more, missed, (int)bound, ends, bad_end, (int)highest_fits, K, worst5, worst1);
    return (bad_split == 0 && wrapped == 0 && grew_more == 0 && missed == 0 && bound && bad_end == 0 && highest_fits && windows > 100 && e_score != 0u) ? 0 : 1;
}
