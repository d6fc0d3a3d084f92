// Host-side check of the roll step's back end in farkle_ii_amd/csrc/fk_device.h (no GPU calls): the form the game kernels run,
// roll_back_end50, against its readable statement roll_back_end50_decoded, each followed by the two-seat table advance, over
//   all 923 multisets x dice rolled n from the multiset's dice count to 6 x the 144 flag sets ThresholdStrategy admits
//   x thr50 {1, 5, 8, 201} x dthr -1..6 x turn score / 50 {0, 9, 10, 1300} x has_scored x seat x {normal round, trigger, final round}
//   x rounds {below, at} max_rounds, for lean and full counter words, with per-lane flags and (lean) with launch-uniform flags;
// after every advance the relations the two-seat kernels rely on instead of carrying the trigger seat and the safety flag are asserted;
// seat 1's counter words sit at their guard bands, so `overflow` is seen both ways.  Also: every discard-table byte's two high bits
// agree with its d5 / d1 fields.  Built and run by tests/test_roll_back_end_host.py with hipcc (host compilation only).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../farkle_ii_amd/csrc/fk_device.h"

using namespace fk;

namespace {

constexpr int32_t TARGET50 = 200;
constexpr uint32_t MAX_ROUNDS = 7;

struct Counts {
    long cases = 0, bad_regs = 0, bad_over = 0, bad_table = 0, bad_derived = 0, overflows = 0, overs = 0, ended = 0;
};

bool same(const RollRegs &a, const RollRegs &b) {
    return a.cA == b.cA && a.cB == b.cB && a.cC == b.cC && a.cD == b.cD && a.cE == b.cE && a.score == b.score && a.dice == b.dice &&
           a.turn_score == b.turn_score;
}
bool same(const Table2 &a, const Table2 &b) {
    return a.seat == b.seat && a.rounds == b.rounds && a.trigger == b.trigger && a.final_round == b.final_round && a.safety == b.safety &&
           a.score_to_beat == b.score_to_beat;
}

template <bool LEAN>
void one_roll(uint32_t e, uint32_t choice, uint32_t n, const Strat50 &sp, int32_t turn, Counts &c) {
    for (uint32_t has_scored = 0; has_scored < 2; ++has_scored)
        for (uint32_t seat = 0; seat < 2; ++seat)
            for (int phase = 0; phase < 3; ++phase)       // normal round, a bank that reaches the target, final round
                for (uint32_t at_max = 0; at_max < 2; ++at_max) {
                    const int32_t score = phase == 0 ? 20 : phase == 1 ? TARGET50 - 10 : 150;
                    const bool final_round = phase == 2;
                    const int32_t stb = final_round ? 165 : TARGET50;
                    const uint32_t flags = has_scored ? BE_HAS_SCORED : 0u;
                    RollRegs r0;
                    if (seat == 0u) r0 = RollRegs{5u | (2u << 16), 12u, 3u | (4u << 16), 1u | (1u << 16), 0u, score, 0u, turn};
                    else r0 = RollRegs{63999u | (7u << 16), 1305u, 9u | (62999u << 16), 9u | (62999u << 16), 0u, score, 0u, turn};
                    if (LEAN) r0.cB |= 3u << 16, r0.cE = (uint32_t)score | flags | (77u << 18); // hot dice beside highest_turn; score, flags, index
                    else r0.cE = 3u | flags;
                    RollRegs a = r0, b = r0;
                    bool ofa = false, ofb = false;
                    const bool oa = roll_back_end50<LEAN>(e, choice, n, sp, 0u, final_round, stb, a, ofa);
                    const bool ob = roll_back_end50_decoded<LEAN>(e, choice, n, sp, final_round, stb, b, ofb);
                    ++c.cases;
                    c.overflows += ofb, c.overs += ob;
                    if (!same(a, b)) ++c.bad_regs;
                    if (oa != ob || ofa != ofb) ++c.bad_over;
                    if (LEAN) { // the same with every flag taken from the launch-uniform word (MIXED = 0: no flag differs between lanes)
                        RollRegs u = r0;
                        bool ofu = false;
                        const bool ou = roll_back_end50<LEAN, 0u>(e, choice, n, Strat50{sp.thr50, sp.bits & 0xffu, sp.dthr}, sp.bits & 0xff00u,
                                                                  final_round, stb, u, ofu);
                        if (!same(u, b)) ++c.bad_regs;
                        if (ou != ob || ofu != ofb) ++c.bad_over;
                    }
                    // (in a final round the trigger seat is the one that does not own the turn: the state a game can be in)
                    Table2 ta{seat, at_max ? MAX_ROUNDS : MAX_ROUNDS - 1u, final_round ? seat ^ 1u : 0u, final_round ? 1u : 0u, 0u, stb}, tb = ta;
                    const Advance2 xa = advance2_table50(oa, a.score, TARGET50, MAX_ROUNDS, ta);
                    const Advance2 xb = advance2_table50(ob, b.score, TARGET50, MAX_ROUNDS, tb);
                    c.ended += xb.ended;
                    if (!same(ta, tb) || xa.ended != xb.ended || xa.sw != xb.sw) ++c.bad_table;
                    // what the two-seat kernel instances derive instead of carrying (fk_kernels.h: seat_turns, finish_game): in a final round
                    // the trigger seat is the other seat; a game that has ended hit the round limit iff it is not in its final round
                    if (ta.final_round != 0u && ta.trigger != (ta.seat ^ 1u)) ++c.bad_derived;
                    if (xa.ended && ta.safety != (ta.final_round != 0u ? 0u : 1u)) ++c.bad_derived;
                    if (!xa.ended && ta.safety != 0u) ++c.bad_derived;
                    if (xa.ended && xa.sw) ++c.bad_derived; // the seat that ended the game still owns the turn
                }
}

} // namespace

int main() {
    std::vector<uint8_t> dlut(DISCARD_LUT_KEYS);
    long bad_bits = 0;
    for (uint32_t k = 0; k < DISCARD_LUT_KEYS; ++k) {
        const uint32_t b = dlut[k] = discard_lut_entry(k);
        const uint32_t d5 = b & 3u, d1 = (b >> 2) & 3u;
        if (((b >> DCH_ANY5_SHIFT) & 1u) != (d5 ? 1u : 0u) || ((b >> DCH_ANY1_SHIFT) & 1u) != (d1 ? 1u : 0u) || (b >> 6) != 0u) ++bad_bits;
    }
    std::vector<uint32_t> lut32(SCORE_LUT_KEYS);
    for (uint32_t k = 0; k < SCORE_LUT_KEYS; ++k) lut32[k] = score_lut_entry32(k);
    std::vector<uint32_t> keys; // the 923 multisets of 1..6 dice
    std::vector<uint32_t> dice_of;
    for (uint32_t key = 1; key < SCORE_LUT_KEYS; ++key) {
        uint32_t m = 0;
        bool ok = true;
        for (int f = 0; f < 6; ++f) {
            const uint32_t c = (key >> (3 * f)) & 7u;
            ok &= c <= 6u;
            m += c;
        }
        if (ok && m >= 1 && m <= 6) keys.push_back(key), dice_of.push_back(m);
    }
    unsigned n_threads = std::thread::hardware_concurrency();
    n_threads = n_threads < 1 ? 1 : n_threads > 16 ? 16 : n_threads;
    std::vector<Counts> per(n_threads);
    std::atomic<size_t> next{0};
    auto work = [&](Counts &c) {
        for (size_t i = next++; i < keys.size(); i = next++) {
            const uint32_t key = keys[i];
            for (uint32_t n = dice_of[i]; n <= 6; ++n)
                for (uint32_t flags = 0; flags < 256; ++flags) {
                    const uint32_t bits = flags << 8;
                    if ((bits & SF_SMART_ONE) && !(bits & SF_SMART_FIVE)) continue; // strategies.py:196-207 (validate_strategies)
                    if ((bits & SF_REQUIRE_BOTH) && !((bits & SF_CONSIDER_SCORE) && (bits & SF_CONSIDER_DICE))) continue;
                    for (int32_t thr50 : {1, 5, 8, 201})
                        for (int32_t dthr = -1; dthr <= 6; ++dthr) {
                            const Strat50 sp{thr50, ((uint32_t)(uint8_t)(int8_t)dthr) | bits};
                            for (int32_t turn : {0, 9, 10, 1300}) {
                                uint32_t e;
                                const uint32_t choice = discard_lookup50(lut32.data(), dlut.data(), key, (int32_t)n, turn, sp, e);
                                one_roll<true>(e, choice, n, sp, turn, c);
                                one_roll<false>(e, choice, n, sp, turn, c);
                            }
                        }
                }
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < n_threads; ++t) pool.emplace_back(work, std::ref(per[t]));
    work(per[0]);
    for (auto &t : pool) t.join();
    Counts c;
    for (const Counts &p : per)
        c.cases += p.cases, c.bad_regs += p.bad_regs, c.bad_over += p.bad_over, c.bad_table += p.bad_table, c.bad_derived += p.bad_derived, c.overflows += p.overflows,
            c.overs += p.overs, c.ended += p.ended;
    printf("multisets %zu cases %ld bad_regs %ld bad_over %ld bad_table %ld bad_derived %ld bad_bits %ld (overs %ld overflows %ld ended %ld)\n", keys.size(), c.cases,
           c.bad_regs, c.bad_over, c.bad_table, c.bad_derived, bad_bits, c.overs, c.overflows, c.ended);
    const bool seen = c.overs > 0 && c.overs < c.cases && c.overflows > 0 && c.overflows < c.cases && c.ended > 0;
    return (keys.size() == 923 && c.bad_regs == 0 && c.bad_over == 0 && c.bad_table == 0 && c.bad_derived == 0 && bad_bits == 0 && seen) ? 0 : 1;
}
