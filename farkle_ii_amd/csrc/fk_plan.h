// fk_plan.h — which game-kernel instance a call runs, and how many of its blocks: the instance table and the launch planner.
// Plain host C++ (no context, no device properties, no runtime call), included behind fk_kernels.h, whose constants it uses:
// tests/native/launch_plan_host_check.hip runs it without a GPU against tests/golden/launch_plan.json.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

constexpr size_t PLAN_LDS_LIMIT = 160 * 1024; // the LDS of a CU as the plan counts it (farkle_hip.hip asserts that a launch may ask for as much)
// The hot / cold rows are seated for at most five waves per SIMD; k = 4 keeps its cold records in LDS, in 320-thread blocks: five
// 256-thread blocks of 32 768 bytes do NOT fit the 160 KB once each is rounded up to the LDS allocation granule (measured: the fifth
// block never became resident, tools/exp_occupancy.py), four 320-thread blocks do.
constexpr int HC_WAVES = 5, HC_COLD_LDS_K = 4, HC_COLD_LDS_BLOCK = 320;

// One compiled shape of the game kernel (each exists in the three MIXED forms): the kernel template, its arguments other than MIXED,
// and what the planner needs to seat it.
struct PlayRow {
    bool hc;   // false: fk_play_kernel<BLOCK, LEAN, WPE, MIXED, GS, BLK, KC>; true: fk_play_hc_kernel<BLOCK, MIXED, LT, KI, WPE, PKR, CL, NS>
    int block, wpe;
    bool lean, gs, blk; // 10-dword seat records (16-bit total / 50) | state store: one LDS record per lane, the others in HBM | batched H2H
    int kc;
    bool lt, pkr, cl;   // hot / cold: score / discard tables in LDS | ... | cold records in LDS (no cold plane)
    int ki, ns;
    int k_min, k_max;   // the seat counts it serves
    int seat_bytes, lane_bytes, block_bytes; // LDS per lane and seat (GS: one seat), per lane, per block
    int per_cu_cap;     // blocks per CU at most; 0: what max_waves allows
    int min_waves;      // hot / cold register rows: the max_waves below which the call stays with the LDS-record kernel
};

constexpr PlayRow rec_row(int block, bool lean, int wpe = 4, bool gs = false, bool blk = false, int kc = 0, int k_min = 1, int k_max = FK_MAX_PLAYERS,
                          int per_cu_cap = 0) {
    return {false, block, wpe, lean, gs, blk, kc, false, false, false, 0, 0, k_min, k_max, (int)(lean ? LEAN_DW : NF) * 4, blk ? 4 : 0, 0, per_cu_cap, 0};
}
// hot part: the generator state, 16 bytes per seat and lane (the buffered half word rides in the cold-plane slot); cold records in LDS: 32
constexpr PlayRow hc_row(int block, bool lt, int ki, int wpe, bool pkr, bool cl, int ns, int k_min, int k_max, int per_cu_cap, int min_waves) {
    return {true, block, wpe, true, false, false, 0, lt, pkr, cl, ki, ns, k_min, k_max, cl ? 32 : 16, 0, lt ? (int)LT_BYTES : 0, per_cu_cap, min_waves};
}

// The 21 shapes, in the planner's order of preference among rows that seat equally many lanes (full records, then larger blocks).
// Instances are compiled for 4 waves/SIMD (<= 128 VGPRs); the 768-thread LEAN instances for 6 (80 VGPRs): their 12 waves split evenly
// over the 4 SIMDs, so two blocks (24 waves) co-reside.  Every other variant that was built and measured lost or tied; their code left
// the tree in round 6 (profiles/HISTORY.md).
constexpr PlayRow PLAY_ROWS[] = {
    rec_row(1024, false), rec_row(512, false), rec_row(256, false), rec_row(128, false), rec_row(64, false),
    rec_row(1024, true),
    rec_row(768, true, 6, false, false, 2, 2, 2), // two seats: the flat hand-over
    rec_row(768, true, 6, false, false, 0),       // (any other seat count; at two seats the row in front wins the tie)
    rec_row(512, true), rec_row(256, true), rec_row(128, true), rec_row(64, true),
    // state store: the path of tables too wide for LDS records (k > 64), 2 x 768 threads per CU whatever k is.  Only on request
    // otherwise: measured 2x slower than LDS records at k = 4 / 8 (the per-turn record exchange is bound by L2 / Infinity-Cache
    // request throughput)
    rec_row(768, true, 6, true),
    rec_row(768, true, 6, false, true, 2, 2, 2, 2), // batched H2H: lean LDS records of both seats + block index, two blocks per CU
    // hot / cold (fk_play_hc.h).  k = 4, cold records in LDS: +5 % over ten-dword records (k = 3 and k = 5 measured +-0).  (77 VGPRs: a
    // SIMD must be able to take six waves, or the 2 + 1 + 1 + 1 waves of four 320-thread blocks do not all find a slot — a 96-register
    // build seated three blocks.)
    hc_row(HC_COLD_LDS_BLOCK, false, 0, 6, false, true, 4, HC_COLD_LDS_K, HC_COLD_LDS_K, HC_WAVES * 256 / HC_COLD_LDS_BLOCK, 0),
    // register rows (increments of every seat in registers, tables in LDS, strategies loaded per turn).  k = 5 .. 7 run FOUR waves per
    // SIMD in whatever block size lets the hot planes and the table image fit: 4 x 256 threads at k = 5, 2 x 512 at k = 6, 1 x 1 024 at
    // k = 7, register arrays and select trees sized for the launch's own seat count; k = 8 (hot planes alone 160 KB at four waves)
    // stays at 3 x 256.
    hc_row(256, true, 5, 4, false, false, 6, 5, 5, 4, 4), hc_row(512, true, 6, 4, false, false, 6, 6, 6, 2, 4),
    hc_row(1024, true, 7, 4, false, false, 8, 7, 7, 1, 4), hc_row(256, true, 8, 0, true, false, 8, 8, 8, 3, 3),
    // nine to twelve seats (round 5): ONE 768-thread block per CU = three waves per SIMD, 168 registers per lane; the hot planes
    // (147 456 bytes at twelve seats) fit beside the table image
    hc_row(768, true, 10, 3, false, false, 10, 9, 10, 1, 3), hc_row(768, true, 12, 3, false, false, 12, 11, 12, 1, 3),
};
constexpr int N_PLAY_ROWS = (int)(sizeof(PLAY_ROWS) / sizeof(PLAY_ROWS[0]));
static_assert(PLAY_ROWS[N_PLAY_ROWS - 1].k_max == (int)HC_MAX_K, "the hot / cold rows end at the seat count fk_play_hc.h is built for");

struct PlanKnobs { // the options a caller can set (fk_set_option) that the plan depends on, and the device's CU count
    int cus = 1;
    int32_t max_waves = 6, blocks_per_cu = 0, block = 0, lean = -1, gs = -1, hc = -1, use_lds_tally = -1;
};

enum PlanMode { PLAN_TOURNAMENT, PLAN_LIST, PLAN_H2H }; // fk_tournament_run*, the game-list entries, fk_h2h_run_blocks

struct LaunchPlan {
    int row = -1; // index into PLAY_ROWS
    int block = 0, grid = 0, cus = 1; // block == 0: no instance fits
    mutable int launched_grid = 0; // the grid after the occupancy clamp of the launch
    mutable const char *instance = nullptr; // the kernel instance the launch ran, as the compiler spells its template (fk_last_play_instance)
    size_t lds = 0;
    bool lds_tally = false;
    uint32_t mixed_flags = 0xff00u; // flag bits that differ between strategies of the table (selects the kernel instance)
    const PlayRow &shape() const { return PLAY_ROWS[row]; }
};

inline size_t row_lds_bytes(const PlayRow &r, int32_t k) {
    return (size_t)r.block * ((size_t)r.seat_bytes * (size_t)(r.gs ? 1 : k) + (size_t)r.lane_bytes) + (size_t)r.block_bytes;
}

// `row` with as many blocks per CU as LDS, the row's cap or the wave budget, and option blocks_per_cu allow (at least one).
// Waves per SIMD: the occupancy an instance is compiled for (WPE) is a floor, not a ceiling — every LDS-record instance allocates at
// most 80 VGPRs, so six waves fit (the launch trims the grid to the occupancy HIP reports).  Measured at k = 2 / 5160 strategies:
// 4 waves 25.8 ms, 6 waves (80 VGPRs) 22.4 ms, 7 waves (72 VGPRs) 23.5 ms.
inline LaunchPlan seat_row(const PlanKnobs &kn, int row, size_t lds, bool lds_tally) {
    const PlayRow &r = PLAY_ROWS[row];
    int per_cu = std::min((int)(PLAN_LDS_LIMIT / lds), r.per_cu_cap ? r.per_cu_cap : std::max(1, kn.max_waves * 4 * 64 / r.block));
    if (kn.blocks_per_cu > 0) per_cu = std::min(per_cu, kn.blocks_per_cu);
    LaunchPlan p;
    p.row = row;
    p.block = r.block;
    p.grid = kn.cus * std::max(per_cu, 1);
    p.cus = kn.cus;
    p.lds = lds;
    p.lds_tally = lds_tally;
    return p;
}

// The row and grid of a call: among the LDS-record rows the one with the most resident lanes per CU (ties: an LDS tally, full records,
// the earlier row); for a tournament then the hot / cold row of this k, if the options and the target allow it and it seats more
// lanes.  State-store rows are taken on request, or when no other row fits.  Lean records carry the banked total / 50 in 16 bits:
// tables whose target is above 50 * LEAN_MAX_TARGET50 points play with full records; block == 0 in the result = no instance fits
// (such a target with batched H2H, or with more seats than LDS holds full records for).
inline LaunchPlan plan_play(const PlanKnobs &kn, PlanMode mode, int32_t k, int64_t S, bool single_batch, int32_t target_score) {
    LaunchPlan best;
    const int32_t target50 = ceil_div50(target_score);
    const bool gs_wanted = kn.gs == 1;
    const size_t tally_bytes = (mode == PLAN_TOURNAMENT && single_batch && kn.use_lds_tally != 0 && S <= 4096) ? (size_t)S * LT_COLS * 8 : 0;
    int best_lanes = -1;
    for (int i = 0; i < N_PLAY_ROWS; ++i) {
        const PlayRow &r = PLAY_ROWS[i];
        if (r.hc || r.blk != (mode == PLAN_H2H) || k < r.k_min || k > r.k_max) continue;
        if (r.lean && target50 > LEAN_MAX_TARGET50) continue;
        if (r.gs && !gs_wanted && best_lanes >= 0) continue; // the other layout only if the wanted one does not fit
        if (!r.gs && !r.blk) { // options lean / block choose among the LDS-record rows
            if ((kn.lean >= 0 && (int)r.lean != kn.lean) || (kn.block != 0 && r.block != kn.block)) continue;
            if (r.lean && S > (1 << (32 - CE_IDX_SHIFT))) continue; // strategy index must fit cE[31:18]
        }
        const bool tally = tally_bytes && row_lds_bytes(r, k) + tally_bytes <= PLAN_LDS_LIMIT / (r.gs ? 2 : 1);
        const size_t lds = row_lds_bytes(r, k) + (tally ? tally_bytes : 0);
        if (lds > PLAN_LDS_LIMIT) continue;
        const LaunchPlan p = seat_row(kn, i, lds, tally);
        int lanes = p.grid / p.cus * p.block * 4 + (tally ? 2 : 0) + (r.lean ? 0 : 1); // tie-breaks: tally, then full records
        if (r.gs == gs_wanted) lanes += 1 << 24;                                         // the wanted layout wins when it fits
        if (lanes > best_lanes) {
            best_lanes = lanes;
            best = p;
        }
    }
    // feasible whenever lean records are: a state-store row needs 40 bytes of LDS per lane whatever k is
    if (mode != PLAN_TOURNAMENT || best.block == 0 || kn.hc == 0 || gs_wanted || best.lds_tally || target50 > HC_MAX_TARGET50) return best;
    // The hot / cold row, from five seats on when it seats more lanes than the LDS-record plan.  Measured on the 5 160-strategy grid
    // against the LDS-record kernel in the same process (round 3, tools/exp_hc2.py, tools/exp_hc3.py): k = 8 +27 %, k = 7 +25 %,
    // k = 6 +23 %, k = 5 +10 % games/s.  The library holds the rows' own instances only: option max_waves below a row's wave count
    // sends the call to the LDS-record kernel instead of to an instance that was not compiled.
    for (int i = 0; i < N_PLAY_ROWS; ++i) {
        const PlayRow &r = PLAY_ROWS[i];
        if (!r.hc || k < r.k_min || k > r.k_max || kn.max_waves < r.min_waves || row_lds_bytes(r, k) > PLAN_LDS_LIMIT) continue;
        const LaunchPlan p = seat_row(kn, i, row_lds_bytes(r, k), false);
        if (r.cl || p.grid / p.cus * p.block > best.grid / best.cus * best.block) return p; // (the cold-in-LDS row whatever it seats)
    }
    return best;
}
