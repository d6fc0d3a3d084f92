// fk_rare_events.h — the game-stats stage's rare-event game list and second-highest-score histograms on the device (included by
// farkle_hip.hip after fk_game_stats.h; fk_tournament_run_rare_events).
//
// Reference semantics (analysis/game_stats.py): a game is a rare event when at least two seats reach the rare target
// (`multi`, _build_rare_event_summary_shard :2827) or when it completed with k >= 2 and its runner-up margin is <= one of the
// configured thresholds (:2834-2837).  The quantile thresholds (_resolve_rare_event_thresholds :3293-3328) are order statistics
// of two integer histograms: the runner-up margin of completed games (fk_game_stats.h already keeps it) and the second-highest
// seat score over ALL attempted games with k >= 2, safety-limit games included (_second_highest :3395-3406).
//
// Everything here runs behind fk_game_record_kernel / fk_game_stats_gather_kernel, which stay as they are; nothing runs inside
// the game kernel.
//
//   The second score lives in a SECOND RECORD ARRAY (uint32 per game, units of 50) instead of the free bits of the game
//   record's w: the record kernel and its 16-byte layout then compile unchanged, at the price of 4 more bytes per game.
//
//   fk_second_score_kernel    one lane per game (grid-stride): second-highest R_SCORE of the game's k >= 2 state records ->
//                             sec[id] and the call's game-level histogram (LDS, non-zero bins flushed per workgroup).
//   fk_second_gather_kernel   workgroup = (strategy, segment of shuffles), as fk_game_stats_gather_kernel: the strategy's seat
//                             exposures read sec[] through the inverse permutation into one LDS histogram.
//   Values at or beyond the window go to the game-stats spill list as kind 3 (SPILL_SECOND); nothing is clamped.
//
//   The flagged games are written by an ORDER-PRESERVING stream compaction, so that events come out in ascending (shuffle, game)
//   order for any grid, workspace chunking and split of the shuffle range.  A game's flags are a pure function of its 16-byte
//   game record, so the count is a pass of its own over those records (simpler than a second instance of the record kernel,
//   whose grid-stride loop does not keep games of one workgroup contiguous):
//     fk_event_count_kernel     workgroup b owns games [256 b, 256 b + 256): each wave ballots its flagged lanes (64-bit
//                               __ballot), the four wave counts are summed through LDS -> blk[b].
//     fk_event_scan_kernel      ONE workgroup of 1024 lanes scans blk[] in tiles (wave scan by __shfl_up, wave totals through
//                               LDS) into 64-bit bases, starting from the call's running total, which it then advances: the
//                               base carries across the chunks of one call.
//     fk_event_scatter_kernel   recomputes the flags, ranks each flagged lane by mbcnt of its wave's ballot plus the counts of
//                               the waves before it, and writes head + seats at base[b] + rank (when inside the capacity).
//
//   event_head uint32 [cap][4]:  x = shuffle index - shuffle_begin
//                                y = game index | completed << 16 | multi << 17 | threshold mask << 18 (bit i: margin <= thresholds[i])
//                                z = runner-up margin / 50,  w = score spread / 50  (0 unless completed with k >= 2)
//   event_seats uint16 [cap][k]: the seats' strategy TABLE indices in seat order (perm_at of the device permutation).
#pragma once

namespace fkre {

constexpr uint32_t MAX_SECOND_BINS = 4096, MAX_THRESHOLDS = 8, COUNT_BLOCK = 256, SCAN_BLOCK = 1024;
enum : int32_t { SPILL_SECOND = 3 };

struct Thresholds { // by value: the unrolled reads below stay in scalar registers
    int32_t n;
    int32_t v[MAX_THRESHOLDS]; // points, any sign
};

// bit 0: multi; bit 1 + i: completed, k >= 2 and margin <= v[i]
__device__ inline uint32_t event_flags(const uint4 r, const Thresholds &t) {
    uint32_t f = r.w >= 2u ? 1u : 0u;
    if ((r.x >> 17) & 1u) {
        const int64_t margin = (int64_t)r.y * 50;
#pragma unroll
        for (int i = 0; i < (int)MAX_THRESHOLDS; ++i)
            if (i < t.n && margin <= (int64_t)t.v[i]) f |= 2u << i;
    }
    return f;
}

// LDS: second [ws]
__global__ __launch_bounds__(256) void fk_second_score_kernel(const uint32_t *state, const uint32_t *inv_sched, uint32_t n_games, uint32_t gps,
                                                              uint32_t n_sh, uint32_t k, uint32_t ws, uint32_t *sec,
                                                              unsigned long long *g_second, fkg::Spill sp) {
    extern __shared__ uint32_t lds[];
    for (uint32_t i = threadIdx.x; i < ws; i += blockDim.x) lds[i] = 0;
    __syncthreads();
    for (uint32_t id = blockIdx.x * blockDim.x + threadIdx.x; id < n_games; id += gridDim.x * blockDim.x) {
        const uint32_t slot = inv_sched ? inv_sched[id] : walk_slot(id, gps, n_sh, true);
        const uint32_t *gs = state + (size_t)slot * k * STATE_DW;
        int32_t hi = INT32_MIN, second = INT32_MIN;
        for (uint32_t j = 0; j < k; ++j) {
            const int32_t sc = (int32_t)gs[(size_t)j * STATE_DW + R_SCORE]; // units of 50
            if (sc > hi) {
                second = hi;
                hi = sc;
            } else if (sc > second) {
                second = sc;
            }
        }
        sec[id] = (uint32_t)second; // (k >= 2: the host launches nothing for one seat)
        fkg::hist_add(lds, ws, (uint32_t)second, sp, -1, SPILL_SECOND);
    }
    __syncthreads();
    fkg::hist_flush(lds, ws, g_second);
}

// grid = (S, n_seg); LDS: second [ws].  Output rows have sb bins (>= ws).
__global__ __launch_bounds__(256) void fk_second_gather_kernel(const uint32_t *sec, const uint16_t *inv_T, uint32_t perm_slots, uint32_t S, uint32_t k,
                                                               uint32_t gps, uint32_t n_sh, uint32_t rows_per_seg, uint32_t ws, uint32_t sb,
                                                               unsigned long long *s_second, fkg::Spill sp) {
    extern __shared__ uint32_t lds[];
    const uint32_t s = blockIdx.x;
    const uint32_t first = blockIdx.y * rows_per_seg, last = min(first + rows_per_seg, n_sh);
    if (first >= last) return; // (uniform over the workgroup)
    for (uint32_t i = threadIdx.x; i < ws; i += blockDim.x) lds[i] = 0;
    __syncthreads();
    for (uint32_t sh = first + threadIdx.x; sh < last; sh += blockDim.x) {
        const uint32_t p = perm_at(inv_T, S, perm_slots, sh, s); // position = game * k + seat of the strategy in this shuffle
        fkg::hist_add(lds, ws, sec[(size_t)sh * gps + p / k], sp, (int32_t)s, SPILL_SECOND);
    }
    __syncthreads();
    fkg::hist_flush(lds, ws, s_second + (size_t)s * sb);
}

// workgroup b: games [256 b, 256 b + 256) -> blk[b]
__global__ __launch_bounds__(256) void fk_event_count_kernel(const uint4 *grec, uint32_t n_games, Thresholds t, uint32_t *blk) {
    __shared__ uint32_t wave_n[COUNT_BLOCK / 64];
    const uint32_t id = blockIdx.x * COUNT_BLOCK + threadIdx.x;
    const bool flagged = id < n_games && event_flags(grec[id], t) != 0u;
    const uint64_t m = __ballot(flagged);
    if ((threadIdx.x & 63u) == 0u) wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

// one workgroup: base[b] = *total + (blk[0] + ... + blk[b - 1]); *total += every blk
__global__ __launch_bounds__(1024) void fk_event_scan_kernel(const uint32_t *blk, uint32_t n_blocks, unsigned long long *total,
                                                             unsigned long long *base) {
    __shared__ uint32_t wave_sum[SCAN_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long run = *total;
    __syncthreads();
    for (uint32_t tile = 0; tile < n_blocks; tile += SCAN_BLOCK) {
        const uint32_t i = tile + threadIdx.x;
        const uint32_t v = i < n_blocks ? blk[i] : 0u;
        uint32_t x = v; // inclusive scan over the wave
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63u) wave_sum[wave] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < SCAN_BLOCK / 64; ++w) {
            const uint32_t s = wave_sum[w];
            before += w < wave ? s : 0u;
            all += s;
        }
        if (i < n_blocks) base[i] = run + before + (x - v);
        run += all; // (a tile holds at most 1024 * 256 events)
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = run;
}

__global__ __launch_bounds__(256) void fk_event_scatter_kernel(const uint4 *grec, const uint16_t *perm_T, uint32_t perm_slots, uint32_t S, uint32_t k,
                                                               uint32_t gps, uint32_t n_games, uint32_t sh_base, Thresholds t,
                                                               const unsigned long long *base, unsigned long long cap, uint4 *head,
                                                               uint16_t *seats) {
    __shared__ uint32_t wave_n[COUNT_BLOCK / 64];
    const uint32_t id = blockIdx.x * COUNT_BLOCK + threadIdx.x, wave = threadIdx.x >> 6;
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    uint32_t f = 0;
    if (id < n_games) {
        r = grec[id];
        f = event_flags(r, t);
    }
    const uint64_t m = __ballot(f != 0u);
    if ((threadIdx.x & 63u) == 0u) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!f) return;
    uint32_t rank = mbcnt(m);
    for (uint32_t w = 0; w < wave; ++w) rank += wave_n[w];
    const unsigned long long e = base[blockIdx.x] + rank;
    if (e >= cap) return; // (the host reports the size the list needs)
    const uint32_t sh = id / gps, g = id - sh * gps;
    head[e] = make_uint4(sh_base + sh, g | (((r.x >> 16) & 1u) << 16) | ((f & 1u) << 17) | ((f >> 1) << 18), r.y, r.z);
    uint16_t *dst = seats + (size_t)e * k;
    for (uint32_t j = 0; j < k; ++j) dst[j] = perm_at(perm_T, S, perm_slots, sh, g * k + j);
}

} // namespace fkre
