// fk_trace.h — roll-level game trace on the device (included by farkle_hip.hip after fk_kernels.h).
//
// fk_trace_kernel<WRITE> plays an explicit list of games, one lane per game, and emits every roll as a 16-byte fk_roll_event
// (include/farkle_hip.h).  It restates FarkleGame.play / _run_final_round (src/farkle/game/engine.py:436-550) around
// FarklePlayer.take_turn (:208-273) from the plain, table-free functions of fk_device.h:
//     ss_* / pcg_seed              the seat streams (src/farkle/utils/random.py:80-188)
//     roll_counts_sequential       the dice in DRAW order (engine.py:85-101) — the game kernels' order-free key cannot give them
//     default_score                the SWAR scorer + discard search in points (src/farkle/game/scoring.py:618-693)
//     should_continue              FarklePlayer._should_continue in points (engine.py:156-205)
// It reads neither the score / discard tables nor the LDS image and does not use the fast dice path: its rows equal the game
// kernels' byte for byte through an independent path.
//
// Tracing is a diagnostic over thousands of games, not 10^8: lanes of a wave diverge (games differ in length 40-fold, seats in
// strategy) and nothing is done about it.  One wave per workgroup, so that a list of a few hundred games still spreads over CUs.
//
// Two passes over the same code.  WRITE = false counts the events of every game and produces the rows; an exclusive scan of the
// counts gives event_begin; WRITE = true replays the games from their seeds and stores the events at their offsets.
//
// Per-seat state — generator state and increment, the buffered half-word, score, has_scored, the nine row counters: TR_FIELDS
// dwords — lives in a call-scoped HBM workspace, not in scratch (k may be 128).  Layout [seat][field][game], game-minor: the 64
// lanes of a wave touch 64 adjacent dwords whatever seat each of them is at.
#pragma once

namespace fktr {

constexpr uint32_t TR_BLOCK = 64;
enum : uint32_t {
    TF_STATE = 0, // 4 dwords: lo, hi of the 128-bit LCG state, low dword first
    TF_INC = 4,   // 4 dwords: the increment (written once)
    TF_BUF = 8,   // buffered high half of the last 64-bit output
    TF_FLAGS = 9, // bit 0 has_buf, bit 1 has_scored
    TF_SCORE = 10,
    TF_FARKLES = 11, TF_ROLLS, TF_TURNS, TF_HIGHEST, TF_S5_USES, TF_S5_DICE, TF_S1_USES, TF_S1_DICE, TF_HOT,
    TR_FIELDS = 20
};
constexpr uint32_t TR_ROLL_LIMIT = 1000u; // engine.py:36
// error word: the smallest (game << 8 | kind) of the launch, ~0 = none
constexpr unsigned long long TR_NO_ERROR = ~0ull;
enum : uint32_t { TR_ERR_ROLL_LIMIT = 1, TR_ERR_OVERFLOW = 2 };

struct TraceArgs {
    const fk_coord *coords;       // [n_games], seat_index 0
    const int2 *strat;            // [S]: score_threshold in points, flag bits | dice threshold (fk_device.h: Strat)
    const int32_t *seat_strategy; // [n_games][k]
    uint32_t n_games, n_pad, k;   // n_pad: n_games rounded up to the wave, the workspace's game stride
    int32_t target_score;
    uint32_t max_rounds;
    uint32_t *ws;                  // [k][TR_FIELDS][n_pad]
    uint8_t *rows;                 // WRITE = false: [n_games] rows of 4 + 28 k bytes
    long long *counts;             // WRITE = false: [n_games] events per game
    const long long *begin;        // WRITE = true: [n_games + 1]
    uint4 *events;                 // WRITE = true
    unsigned long long *err;
};

struct SeatRegs {
    Rng r;
    int32_t score;
    uint32_t has_scored;
    uint32_t farkles, rolls, turns, highest, s5_uses, s5_dice, s1_uses, s1_dice, hot;
};

__device__ inline uint32_t *seat_ptr(const TraceArgs &a, uint32_t seat, uint32_t g) {
    return a.ws + (size_t)seat * TR_FIELDS * a.n_pad + g;
}

__device__ inline void seat_load(const TraceArgs &a, uint32_t seat, uint32_t g, SeatRegs &s) {
    const uint32_t *p = seat_ptr(a, seat, g);
    const size_t n = a.n_pad;
    s.r.lo = (uint64_t)p[(TF_STATE + 0) * n] | ((uint64_t)p[(TF_STATE + 1) * n] << 32);
    s.r.hi = (uint64_t)p[(TF_STATE + 2) * n] | ((uint64_t)p[(TF_STATE + 3) * n] << 32);
    s.r.inc_lo = (uint64_t)p[(TF_INC + 0) * n] | ((uint64_t)p[(TF_INC + 1) * n] << 32);
    s.r.inc_hi = (uint64_t)p[(TF_INC + 2) * n] | ((uint64_t)p[(TF_INC + 3) * n] << 32);
    s.r.buf = p[TF_BUF * n];
    const uint32_t f = p[TF_FLAGS * n];
    s.r.has_buf = f & 1u;
    s.has_scored = (f >> 1) & 1u;
    s.score = (int32_t)p[TF_SCORE * n];
    s.farkles = p[TF_FARKLES * n];
    s.rolls = p[TF_ROLLS * n];
    s.turns = p[TF_TURNS * n];
    s.highest = p[TF_HIGHEST * n];
    s.s5_uses = p[TF_S5_USES * n];
    s.s5_dice = p[TF_S5_DICE * n];
    s.s1_uses = p[TF_S1_USES * n];
    s.s1_dice = p[TF_S1_DICE * n];
    s.hot = p[TF_HOT * n];
}

// everything a turn may change (the increment is not one of them)
__device__ inline void seat_store(const TraceArgs &a, uint32_t seat, uint32_t g, const SeatRegs &s) {
    uint32_t *p = seat_ptr(a, seat, g);
    const size_t n = a.n_pad;
    p[(TF_STATE + 0) * n] = (uint32_t)s.r.lo;
    p[(TF_STATE + 1) * n] = (uint32_t)(s.r.lo >> 32);
    p[(TF_STATE + 2) * n] = (uint32_t)s.r.hi;
    p[(TF_STATE + 3) * n] = (uint32_t)(s.r.hi >> 32);
    p[TF_BUF * n] = s.r.buf;
    p[TF_FLAGS * n] = (s.r.has_buf & 1u) | (s.has_scored << 1);
    p[TF_SCORE * n] = (uint32_t)s.score;
    p[TF_FARKLES * n] = s.farkles;
    p[TF_ROLLS * n] = s.rolls;
    p[TF_TURNS * n] = s.turns;
    p[TF_HIGHEST * n] = s.highest;
    p[TF_S5_USES * n] = s.s5_uses;
    p[TF_S5_DICE * n] = s.s5_dice;
    p[TF_S1_USES * n] = s.s1_uses;
    p[TF_S1_DICE * n] = s.s1_dice;
    p[TF_HOT * n] = s.hot;
}

// _make_players (src/farkle/simulation/simulation.py:412-447): seat i's stream is the game's coordinate with seat_index = i
__device__ inline void seed_seats(const TraceArgs &a, uint32_t g) {
    const fk_coord c = a.coords[g];
    SeedPool gp;
    ss_begin(gp, 2u, c.purpose, (uint32_t)c.root_seed, (uint32_t)(c.root_seed >> 32));
    ss_absorb64(gp, c.k);
    ss_absorb64(gp, c.shuffle_index);
    ss_absorb64(gp, c.pair_id);
    ss_absorb64(gp, c.order);
    ss_absorb64(gp, c.game_index);
    for (uint32_t seat = 0; seat < a.k; ++seat) {
        SeedPool sp = gp;
        ss_absorb64(sp, c.seat_index + seat);
        ss_absorb64(sp, c.replicate_index);
        uint32_t g8[8];
        ss_generate<8>(sp, g8);
        SeatRegs s{};
        pcg_seed(s.r, g8);
        uint32_t *p = seat_ptr(a, seat, g);
        const size_t n = a.n_pad;
        p[(TF_INC + 0) * n] = (uint32_t)s.r.inc_lo;
        p[(TF_INC + 1) * n] = (uint32_t)(s.r.inc_lo >> 32);
        p[(TF_INC + 2) * n] = (uint32_t)s.r.inc_hi;
        p[(TF_INC + 3) * n] = (uint32_t)(s.r.inc_hi >> 32);
        seat_store(a, seat, g, s);
    }
}

// nibble-packed faces of roll_counts_sequential -> the event's 3-bit fields + the dice count
__device__ inline uint32_t event_dice(uint32_t faces4, uint32_t n) {
    uint32_t d = n << 18;
    for (uint32_t i = 0; i < 6u; ++i) d |= ((faces4 >> (4u * i)) & 7u) << (3u * i);
    return d;
}

// The row of a finished game (simulation.py:628-655; ranks engine.py:477-483: stable sort by score descending).
__device__ inline void write_row(const TraceArgs &a, uint32_t g, uint32_t rounds, bool safety) {
    const size_t n = a.n_pad;
    uint32_t *row = reinterpret_cast<uint32_t *>(a.rows + (size_t)g * (4u + 28u * a.k));
    uint32_t winner = 0xffu, over = 0u;
    for (uint32_t i = 0; i < a.k; ++i) {
        const uint32_t *p = seat_ptr(a, i, g);
        const int32_t score = (int32_t)p[TF_SCORE * n];
        uint32_t rank = 0u;
        if (!safety) {
            rank = 1u;
            for (uint32_t j = 0; j < a.k; ++j) {
                const int32_t sj = (int32_t)seat_ptr(a, j, g)[TF_SCORE * n];
                rank += (sj > score || (sj == score && j < i)) ? 1u : 0u;
            }
            if (rank == 1u) winner = i;
        }
        const uint32_t farkles = p[TF_FARKLES * n], rolls = p[TF_ROLLS * n], turns = p[TF_TURNS * n], highest = p[TF_HIGHEST * n];
        const uint32_t s5u = p[TF_S5_USES * n], s5d = p[TF_S5_DICE * n], s1u = p[TF_S1_USES * n], s1d = p[TF_S1_DICE * n], hot = p[TF_HOT * n];
        over |= farkles | rolls | turns | highest | s5u | s5d | s1u | s1d | hot; // any of them beyond 16 bits
        uint32_t *s = row + 1u + 7u * i;
        s[0] = (uint32_t)score;
        s[1] = (uint32_t)a.seat_strategy[(size_t)g * a.k + i];
        s[2] = (farkles & 0xffffu) | (rolls << 16);
        s[3] = (turns & 0xffffu) | (highest << 16);
        s[4] = (s5u & 0xffffu) | (s5d << 16);
        s[5] = (s1u & 0xffffu) | (s1d << 16);
        s[6] = (hot & 0xffffu) | (rank << 16) | ((safety ? 1u : 0u) << 24);
    }
    row[0] = (rounds & 0xffffu) | ((safety ? (uint32_t)FK_SAFETY_LIMIT : (uint32_t)FK_COMPLETED) << 16) | (winner << 24);
    if (over > 0xffffu) atomicMin(a.err, ((unsigned long long)g << 8) | TR_ERR_OVERFLOW);
}

template <bool WRITE>
__global__ __launch_bounds__(TR_BLOCK) void fk_trace_kernel(TraceArgs a) {
    const uint32_t g = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (g >= a.n_games) return;
    seed_seats(a, g);
    long long n_events = 0;
    const long long base = WRITE ? a.begin[g] : 0;
    // FarkleGame.play (engine.py:436-521): rounds of k turns until a banked total reaches the target; then every other seat
    // plays one final turn in seat order (_run_final_round :523-550).  `trigger` < 0: no final round yet.
    uint32_t rounds = 0, seat = 0;
    int32_t trigger = -1, score_to_beat = a.target_score;
    bool done = a.max_rounds == 0u;
    if (!done) rounds = 1;
    while (!done) {
        const bool final_round = trigger >= 0;
        SeatRegs s;
        seat_load(a, seat, g, s);
        const int2 packed = a.strat[a.seat_strategy[(size_t)g * a.k + seat]];
        const Strat strat{packed.x, (uint32_t)packed.y};
        // take_turn (engine.py:208-273)
        s.turns += 1u;
        uint32_t dice = 6u, rolls_this_turn = 0u;
        int32_t turn_score = 0;
        while (dice > 0u) {
            if (rolls_this_turn >= TR_ROLL_LIMIT) { // :242
                atomicMin(a.err, ((unsigned long long)g << 8) | TR_ERR_ROLL_LIMIT);
                if (!WRITE) a.counts[g] = n_events;
                return;
            }
            const uint32_t n = dice;
            uint32_t faces = 0u;
            const uint32_t counts = roll_counts_sequential<4>(s.r, n, &faces); // _roll :85-101
            s.rolls += 1u;
            rolls_this_turn += 1u;
            const RollResult rr = default_score(counts, (int32_t)n, turn_score, strat); // _score_roll :103-147
            uint32_t flags = final_round ? (uint32_t)FK_EV_FINAL_ROUND : 0u;
            if (rr.score == 0) { // :135-137, 247-249
                s.farkles += 1u;
                turn_score = 0;
                dice = 0u;
            } else {
                if (rr.d5 > 0) { // :139-144
                    s.s5_uses += 1u;
                    s.s5_dice += (uint32_t)rr.d5;
                }
                if (rr.d1 > 0) {
                    s.s1_uses += 1u;
                    s.s1_dice += (uint32_t)rr.d1;
                }
                dice = (rr.used == (int32_t)n) ? 6u : n - (uint32_t)rr.used; // :146
                turn_score += rr.score;
                if (strat.has(SF_AUTO_HOT) && dice == 6u) { // _apply_hot_dice :149-154
                    s.hot += 1u;
                    flags |= FK_EV_AUTO_HOT | FK_EV_ROLL_AGAIN;
                } else {
                    // _should_continue :156-205: decide() is not asked when the final-round lead is banked (:189)
                    const bool stop = final_round && (s.score + turn_score > score_to_beat) && !strat.has(SF_RUN_UP);
                    const bool keep = should_continue(strat, turn_score, (int32_t)dice, s.has_scored != 0u, final_round, score_to_beat, s.score);
                    flags |= (stop ? 0u : (uint32_t)FK_EV_DECIDE) | (keep ? (uint32_t)FK_EV_ROLL_AGAIN : 0u);
                }
            }
            if (WRITE) {
                const uint32_t z = (uint32_t)rr.score | (rounds << 16);
                const uint32_t w = seat | (((uint32_t)rr.used | (dice << 4)) << 8) | (((uint32_t)rr.d5 | ((uint32_t)rr.d1 << 4)) << 16) | (flags << 24);
                a.events[base + n_events] = make_uint4(event_dice(faces, n), (uint32_t)turn_score, z, w);
            }
            n_events += 1;
            if (!(flags & FK_EV_ROLL_AGAIN)) break;
        }
        if (!s.has_scored && turn_score >= 500) s.has_scored = 1u; // :267
        if (s.has_scored) {                                       // :271-273
            s.score += turn_score;
            s.highest = (uint32_t)turn_score > s.highest ? (uint32_t)turn_score : s.highest;
        }
        seat_store(a, seat, g, s);
        // whose turn is next
        if (trigger < 0) {
            if (s.score >= a.target_score) { // engine.py:462-468
                trigger = (int32_t)seat;
                score_to_beat = s.score;
                seat = seat == 0u ? 1u : 0u;
                done = a.k == 1u;
            } else if (++seat == a.k) {
                seat = 0u;
                if (rounds >= a.max_rounds) done = true; // `while rounds < max_rounds` ends: the safety limit (:453, 472)
                else rounds += 1u;
            }
        } else {
            score_to_beat = s.score > score_to_beat ? s.score : score_to_beat; // :546-548
            seat += 1u;
            if (seat == (uint32_t)trigger) seat += 1u;
            done = seat >= a.k;
        }
    }
    if (!WRITE) {
        a.counts[g] = n_events;
        write_row(a, g, rounds, trigger < 0);
    }
}

} // namespace fktr
