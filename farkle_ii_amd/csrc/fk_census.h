// fk_census.h — roll census on the device (included by farkle_hip.hip after fk_trace.h).
//
// fk_census_kernel is the sibling of fk_trace_kernel (fk_trace.h): one lane plays one game with the same plain, table-free
// functions of fk_device.h (ss_* / pcg_seed, roll_counts_sequential, score_counts, default_score_raw, should_continue) and the
// same restatement of FarkleGame.play / _run_final_round around FarklePlayer.take_turn — but where the trace stores a 16-byte
// event per roll, the census COUNTS the roll and stores nothing per roll and nothing per game.  The census is a pure function of the
// trace's event stream (farkle_ii_amd/roll_census.py: RollCensus.from_events is the host statement), so it is pinned bit for
// bit against fk_trace_games.  The game loop is restated, not shared: a template over both would have to be proven to leave
// fk_trace_kernel's code unchanged, and the two differ in every line that touches memory.
//
// Tables (all exact integer counts; "raw" = score_counts(counts), the roll's maximum immediate score and scoring dice BEFORE
// Smart-5 / Smart-1 discards — the reference's score_roll_cached(outcome)[:2]):
//   roll_cells     [6][61][7]       dice rolled - 1, raw score / 50, raw used       32-bit LDS histogram per workgroup -> u64
//   strategy_dice  [S][6][3]        rolls, farkles (raw score 0), all dice scored (raw used == n), for the strategy at turn
//   strategy_turns [S][3]           turns, turns that ended on a farkle, sum of the turns' final turn_score in points
//   turn_hist      [S][turn_bins]   the turn's final turn_score / 50, clamped to turn_bins - 1
// The per-strategy tables take ordinary 64-bit global atomics whose result is not used: S * (21 + turn_bins) counters do not fit
// LDS at 5 160 strategies, and a census of a 64-strategy table is a diagnostic, not a throughput path.
//
// The LDS counters cannot overflow: a game that reaches the flush holds fewer than 65 536 rolls per seat (TR_ERR_OVERFLOW fails the
// call otherwise, and no table is returned), so a workgroup of CN_BLOCK = 256 games of at most 128 seats adds fewer than 2^31.
//
// Two sources of games, one instance each (the arguments of the other mode are dead in an instance, which keeps the kernel's SGPRs
// below the spill line): fk_census_kernel<true> plays an explicit list (coords + seat_strategy, fk_census_games), <false> a
// tournament chunk (fk_tournament_run_census: game id -> (shuffle, game) of the chunk, the seats from the blocked permutations the
// tournament's own kernels wrote, the coordinate of namespace 103 rebuilt on the fly, max_rounds overrides looked up in the chunk's
// sorted list).  The four tables and the error word are one device block with computed offsets, for the same reason.
//
// Resources (hipcc, gfx950): 102 / 106 VGPRs, 105 / 106 SGPRs, 0 B scratch, 10 248 B LDS, 4 waves per SIMD.
//
// Per-seat state lives in a call-scoped HBM workspace laid out [seat][field][game], as the trace's does, with the fields the census
// needs: generator, flags, score and the four row counters that can pass 16 bits when `rolls` does not.
#pragma once

namespace fkcn {

using fktr::TR_ERR_OVERFLOW;
using fktr::TR_ERR_ROLL_LIMIT;
using fktr::TR_ROLL_LIMIT;

constexpr uint32_t CN_BLOCK = 256;
constexpr uint32_t CN_N = 6, CN_SCORES = 61, CN_USED = 7, CN_CELLS = CN_N * CN_SCORES * CN_USED; // 2 562
constexpr uint32_t CN_DICE_COLS = 3, CN_TURN_COLS = 3;
enum : uint32_t {
    CF_STATE = 0, // 4 dwords: lo, hi of the 128-bit LCG state, low dword first
    CF_INC = 4,   // 4 dwords: the increment (written once)
    CF_BUF = 8,   // buffered high half of the last 64-bit output
    CF_FLAGS = 9, // bit 0 has_buf, bit 1 has_scored
    CF_SCORE = 10,
    // the row counters the trace checks against 16 bits; farkles, turns, the discard uses and hot dice never exceed `rolls`
    CF_ROLLS = 11, CF_HIGHEST, CF_S5_DICE, CF_S1_DICE,
    CN_FIELDS = 15
};

struct CensusArgs {
    const fk_coord *coords;       // list mode (fk_census_kernel<true>): [n_games], seat_index 0
    const int32_t *seat_strategy; // list mode: [n_games][k]
    const uint16_t *perm_T;       // tournament mode (fk_census_kernel<false>): blocked permutations of the chunk, see perm_at()
    uint32_t perm_slots, gps;
    uint64_t root_seed, shuffle0;
    const DevOverride *ov;        // tournament mode: chunk-local max_rounds overrides, sorted by game
    uint32_t n_ov;
    const int2 *strat;            // [S]: score_threshold in points, flag bits | dice threshold (fk_device.h: Strat)
    uint32_t n_games, n_pad, k, S; // n_pad: n_games rounded up to the workgroup, the workspace's game stride
    int32_t target_score;
    uint32_t max_rounds;
    uint32_t turn_bins;
    unsigned long long game_base; // the chunk's first game in the call (error word)
    uint32_t *ws;                 // [k][CN_FIELDS][n_pad]
    // the call's tables, one block: roll_cells [CN_CELLS] | strategy_dice [S][6][3] | strategy_turns [S][3] | turn_hist [S][turn_bins] |
    // the error word: the smallest (game << 8 | kind) of the call, ~0 = none (fk_trace.h)
    unsigned long long *tables;
};

__host__ __device__ inline size_t dice_offset(uint32_t S) { (void)S; return CN_CELLS; }
__host__ __device__ inline size_t turns_offset(uint32_t S) { return dice_offset(S) + (size_t)S * CN_N * CN_DICE_COLS; }
__host__ __device__ inline size_t hist_offset(uint32_t S) { return turns_offset(S) + (size_t)S * CN_TURN_COLS; }
__host__ __device__ inline size_t err_offset(uint32_t S, uint32_t turn_bins) { return hist_offset(S) + (size_t)S * turn_bins; }

struct SeatRegs {
    Rng r;
    int32_t score;
    uint32_t has_scored, rolls, highest, s5_dice, s1_dice;
};

__device__ inline uint32_t *seat_ptr(const CensusArgs &a, uint32_t seat, uint32_t g) {
    return a.ws + (size_t)seat * CN_FIELDS * a.n_pad + g;
}

__device__ inline void seat_load(const CensusArgs &a, uint32_t seat, uint32_t g, SeatRegs &s) {
    const uint32_t *p = seat_ptr(a, seat, g);
    const size_t n = a.n_pad;
    s.r.lo = (uint64_t)p[(CF_STATE + 0) * n] | ((uint64_t)p[(CF_STATE + 1) * n] << 32);
    s.r.hi = (uint64_t)p[(CF_STATE + 2) * n] | ((uint64_t)p[(CF_STATE + 3) * n] << 32);
    s.r.inc_lo = (uint64_t)p[(CF_INC + 0) * n] | ((uint64_t)p[(CF_INC + 1) * n] << 32);
    s.r.inc_hi = (uint64_t)p[(CF_INC + 2) * n] | ((uint64_t)p[(CF_INC + 3) * n] << 32);
    s.r.buf = p[CF_BUF * n];
    const uint32_t f = p[CF_FLAGS * n];
    s.r.has_buf = f & 1u;
    s.has_scored = (f >> 1) & 1u;
    s.score = (int32_t)p[CF_SCORE * n];
    s.rolls = p[CF_ROLLS * n];
    s.highest = p[CF_HIGHEST * n];
    s.s5_dice = p[CF_S5_DICE * n];
    s.s1_dice = p[CF_S1_DICE * n];
}

// everything a turn may change (the increment is not one of them)
__device__ inline void seat_store(const CensusArgs &a, uint32_t seat, uint32_t g, const SeatRegs &s) {
    uint32_t *p = seat_ptr(a, seat, g);
    const size_t n = a.n_pad;
    p[(CF_STATE + 0) * n] = (uint32_t)s.r.lo;
    p[(CF_STATE + 1) * n] = (uint32_t)(s.r.lo >> 32);
    p[(CF_STATE + 2) * n] = (uint32_t)s.r.hi;
    p[(CF_STATE + 3) * n] = (uint32_t)(s.r.hi >> 32);
    p[CF_BUF * n] = s.r.buf;
    p[CF_FLAGS * n] = (s.r.has_buf & 1u) | (s.has_scored << 1);
    p[CF_SCORE * n] = (uint32_t)s.score;
    p[CF_ROLLS * n] = s.rolls;
    p[CF_HIGHEST * n] = s.highest;
    p[CF_S5_DICE * n] = s.s5_dice;
    p[CF_S1_DICE * n] = s.s1_dice;
}

// the game's coordinate: the list's, or the tournament's (namespace 103, run_tournament.py:301-351: shuffle, game of the shuffle)
template <bool LIST>
__device__ inline fk_coord game_coord(const CensusArgs &a, uint32_t g) {
    if (LIST) return a.coords[g];
    fk_coord c{};
    c.purpose = 103u; // TOURNAMENT_PLAYER
    c.root_seed = a.root_seed;
    c.k = a.k;
    c.shuffle_index = a.shuffle0 + g / a.gps;
    c.game_index = g % a.gps;
    return c;
}

template <bool LIST>
__device__ inline uint32_t seat_strategy_of(const CensusArgs &a, uint32_t g, uint32_t seat) {
    if (LIST) return (uint32_t)a.seat_strategy[(size_t)g * a.k + seat];
    const uint32_t sh = g / a.gps, gl = g - sh * a.gps;
    return perm_at(a.perm_T, a.S, a.perm_slots, sh, gl * a.k + seat);
}

__device__ inline uint32_t game_max_rounds(const CensusArgs &a, uint32_t g) {
    uint32_t lo = 0, hi = a.n_ov; // first override with game >= g
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.ov[mid].game < g) lo = mid + 1u;
        else hi = mid;
    }
    return (lo < a.n_ov && a.ov[lo].game == g) ? a.ov[lo].max_rounds : a.max_rounds;
}

// _make_players (src/farkle/simulation/simulation.py:412-447): seat i's stream is the game's coordinate with seat_index = i
template <bool LIST>
__device__ inline void seed_seats(const CensusArgs &a, uint32_t g) {
    const fk_coord c = game_coord<LIST>(a, g);
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
        p[(CF_INC + 0) * n] = (uint32_t)s.r.inc_lo;
        p[(CF_INC + 1) * n] = (uint32_t)(s.r.inc_lo >> 32);
        p[(CF_INC + 2) * n] = (uint32_t)s.r.inc_hi;
        p[(CF_INC + 3) * n] = (uint32_t)(s.r.inc_hi >> 32);
        seat_store(a, seat, g, s);
    }
}

// One game, counted.  Returns false when a turn ran into the 1 000-roll fuse (the error word is set; the game is abandoned).
template <bool LIST>
__device__ inline bool census_game(const CensusArgs &a, uint32_t g, uint32_t *cells) {
    seed_seats<LIST>(a, g);
    unsigned long long *const err = a.tables + err_offset(a.S, a.turn_bins);
    const uint32_t max_rounds = (!LIST && a.n_ov) ? game_max_rounds(a, g) : a.max_rounds;
    // FarkleGame.play (engine.py:436-521): rounds of k turns until a banked total reaches the target; then every other seat
    // plays one final turn in seat order (_run_final_round :523-550).  `trigger` < 0: no final round yet.
    uint32_t rounds = 0, seat = 0;
    int32_t trigger = -1, score_to_beat = a.target_score;
    bool done = max_rounds == 0u;
    if (!done) rounds = 1;
    while (!done) {
        const bool final_round = trigger >= 0;
        SeatRegs s;
        seat_load(a, seat, g, s);
        const uint32_t si = seat_strategy_of<LIST>(a, g, seat);
        const int2 packed = a.strat[si];
        const Strat strat{packed.x, (uint32_t)packed.y};
        unsigned long long *sd = a.tables + dice_offset(a.S) + (size_t)si * CN_N * CN_DICE_COLS;
        // take_turn (engine.py:208-273)
        uint32_t dice = 6u, rolls_this_turn = 0u;
        int32_t turn_score = 0;
        bool farkled = false;
        while (dice > 0u) {
            if (rolls_this_turn >= TR_ROLL_LIMIT) { // :242
                atomicMin(err, ((a.game_base + g) << 8) | TR_ERR_ROLL_LIMIT);
                return false;
            }
            const uint32_t n = dice;
            uint32_t faces = 0u;
            const uint32_t counts = roll_counts_sequential<4>(s.r, n, &faces); // _roll :85-101
            s.rolls += 1u;
            rolls_this_turn += 1u;
            const RawScore raw = score_counts(counts);
            const RollResult rr = default_score_raw(raw, (int32_t)n, turn_score, strat); // _score_roll :103-147
            // the census of this roll
            atomicAdd(&cells[((n - 1u) * CN_SCORES + (uint32_t)raw.score / 50u) * CN_USED + (uint32_t)raw.used], 1u);
            unsigned long long *row = sd + (n - 1u) * CN_DICE_COLS;
            atomicAdd(&row[0], 1ull);
            if (raw.score == 0) atomicAdd(&row[1], 1ull);
            if ((uint32_t)raw.used == n) atomicAdd(&row[2], 1ull);
            bool again = false;
            if (rr.score == 0) { // :135-137, 247-249
                farkled = true;
                turn_score = 0;
                dice = 0u;
            } else {
                s.s5_dice += (uint32_t)rr.d5; // :139-144
                s.s1_dice += (uint32_t)rr.d1;
                dice = (rr.used == (int32_t)n) ? 6u : n - (uint32_t)rr.used; // :146
                turn_score += rr.score;
                if (strat.has(SF_AUTO_HOT) && dice == 6u) // _apply_hot_dice :149-154
                    again = true;
                else // _should_continue :156-205
                    again = should_continue(strat, turn_score, (int32_t)dice, s.has_scored != 0u, final_round, score_to_beat, s.score);
            }
            if (!again) break;
        }
        // the census of this turn
        unsigned long long *st = a.tables + turns_offset(a.S) + (size_t)si * CN_TURN_COLS;
        atomicAdd(&st[0], 1ull);
        if (farkled) atomicAdd(&st[1], 1ull);
        if (turn_score > 0) atomicAdd(&st[2], (unsigned long long)turn_score);
        const uint32_t bin = min((uint32_t)turn_score / 50u, a.turn_bins - 1u);
        atomicAdd(&a.tables[hist_offset(a.S) + (size_t)si * a.turn_bins + bin], 1ull);
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
                if (rounds >= max_rounds) done = true; // `while rounds < max_rounds` ends: the safety limit (:453, 472)
                else rounds += 1u;
            }
        } else {
            score_to_beat = s.score > score_to_beat ? s.score : score_to_beat; // :546-548
            seat += 1u;
            if (seat == (uint32_t)trigger) seat += 1u;
            done = seat >= a.k;
        }
    }
    // the row counters of the finished game against 16 bits, as the trace's write_row checks them
    uint32_t over = 0u;
    const size_t n = a.n_pad;
    for (uint32_t i = 0; i < a.k; ++i) {
        const uint32_t *p = seat_ptr(a, i, g);
        over |= p[CF_ROLLS * n] | p[CF_HIGHEST * n] | p[CF_S5_DICE * n] | p[CF_S1_DICE * n];
    }
    if (over > 0xffffu) atomicMin(err, ((a.game_base + g) << 8) | TR_ERR_OVERFLOW);
    return true;
}

template <bool LIST>
__global__ __launch_bounds__(CN_BLOCK) void fk_census_kernel(CensusArgs a) {
    __shared__ uint32_t cells[CN_CELLS];
    for (uint32_t i = threadIdx.x; i < CN_CELLS; i += CN_BLOCK) cells[i] = 0u;
    __syncthreads();
    const uint32_t g = blockIdx.x * CN_BLOCK + threadIdx.x;
    if (g < a.n_games) (void)census_game<LIST>(a, g, cells);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < CN_CELLS; i += CN_BLOCK) {
        const uint32_t v = cells[i];
        if (v) atomicAdd(&a.tables[i], (unsigned long long)v);
    }
}

} // namespace fkcn
