// fk_game_stats.h — the game-stats stage's per-k sufficient statistics on the device (included by farkle_hip.hip after
// fk_kernels.h).
//
// Reference semantics (analysis/game_stats.py, _compute_k_game_stats :840-1220): per strategy over its seat exposures and per
// player count over its games, the n_rounds histogram and the outcome counts; over COMPLETED games with at least two scores the
// runner-up margin (max - second max) and the score spread (max - min) of the game's seat scores (:3378-3406); and for the
// rare-event summary (_build_rare_event_summary_shard :2715-2880) the games where at least two seats reach the rare target.
// Seat scores are multiples of 50, so every quantity is an exact integer histogram.
//
//   fk_game_record_kernel   one lane per game (grid-stride): reads the game's result record and its k state records (R_SCORE,
//                           units of 50) and writes a 16-byte game-major record
//                             x = n_rounds | completed << 16 | margins valid (completed, k >= 2) << 17
//                             y = (max - second max) / 50,   z = (max - min) / 50,   w = seats with score >= rare target
//                           It also accumulates the call's GAME-level counts and n_rounds / runner-up histograms in LDS and
//                           flushes their non-zero bins (one global atomic per bin per workgroup).
//   fk_game_stats_gather_kernel   workgroup = (strategy, segment of shuffles).  A strategy sits once per shuffle: each lane finds
//                           its seat through the inverse permutation (as fk_seat_stats_kernel does), reads that game's record
//                           and adds to the workgroup's LDS histograms; non-zero bins are flushed at the end.  No per-exposure
//                           global atomics.
//
// Exactness: a value at or beyond its histogram window (n_rounds >= rounds window, a margin / 50 >= margin window) is never
// clamped: it is appended to the spill list as (strategy index or -1 for the game level, kind, value).  The list counts every
// entry even past its capacity, so the host can report the size it needs.
#pragma once

namespace fkg {

constexpr uint32_t MAX_ROUNDS_BINS = 4096, MAX_MARGIN_BINS = 2048;
enum : int32_t { SPILL_ROUNDS = 0, SPILL_RUNNER = 1, SPILL_SPREAD = 2 };
enum : uint32_t { GC_ATTEMPTED = 0, GC_COMPLETED, GC_SAFETY, GC_MULTI, N_COUNTS };

struct Spill {
    unsigned long long *count; // entries wanted (may exceed cap)
    int32_t *entries;          // [cap][3]: strategy index (-1: game level), kind, value
    uint64_t cap;
};

__device__ inline void spill_push(const Spill &sp, int32_t who, int32_t kind, uint32_t value) {
    const unsigned long long i = atomicAdd(sp.count, 1ull);
    if (i < sp.cap) {
        int32_t *e = sp.entries + (size_t)i * 3;
        e[0] = who;
        e[1] = kind;
        e[2] = (int32_t)value;
    }
}

// add `v` to LDS bin `v` of a window of `w` bins, or spill it
__device__ inline void hist_add(uint32_t *h, uint32_t w, uint32_t v, const Spill &sp, int32_t who, int32_t kind) {
    if (v < w) atomicAdd(&h[v], 1u);
    else spill_push(sp, who, kind, v);
}

__device__ inline void hist_flush(const uint32_t *h, uint32_t w, unsigned long long *out) {
    for (uint32_t i = threadIdx.x; i < w; i += blockDim.x)
        if (h[i]) atomicAdd(&out[i], (unsigned long long)h[i]);
}

// LDS: rounds [wr] | runner [wm] | counts [4]
__global__ __launch_bounds__(256) void fk_game_record_kernel(const uint32_t *state, const uint32_t *recs, const uint32_t *inv_sched,
                                                             uint32_t n_games, uint32_t gps, uint32_t n_sh, uint32_t k, int64_t rare_target,
                                                             uint32_t wr, uint32_t wm, uint4 *grec, unsigned long long *g_counts,
                                                             unsigned long long *g_rounds, unsigned long long *g_runner, Spill sp) {
    extern __shared__ uint32_t lds[];
    uint32_t *h_rounds = lds, *h_runner = lds + wr, *cnt = lds + wr + wm;
    for (uint32_t i = threadIdx.x; i < wr + wm + N_COUNTS; i += blockDim.x) lds[i] = 0;
    __syncthreads();
    for (uint32_t id = blockIdx.x * blockDim.x + threadIdx.x; id < n_games; id += gridDim.x * blockDim.x) {
        const uint32_t slot = inv_sched ? inv_sched[id] : walk_slot(id, gps, n_sh, true);
        const uint4 q0 = *reinterpret_cast<const uint4 *>(recs + (size_t)id * REC_DW);
        const bool completed = !(q0.x & REC_SAFETY);
        const uint32_t rounds = q0.z & 0xffffu;
        const uint32_t *gs = state + (size_t)slot * k * STATE_DW;
        int32_t hi = INT32_MIN, second = INT32_MIN, lo = INT32_MAX;
        uint32_t n_target = 0;
        for (uint32_t j = 0; j < k; ++j) {
            const int32_t sc = (int32_t)gs[(size_t)j * STATE_DW + R_SCORE]; // units of 50
            if (sc > hi) {
                second = hi;
                hi = sc;
            } else if (sc > second) {
                second = sc;
            }
            lo = min(lo, sc);
            n_target += (int64_t)sc * 50 >= rare_target ? 1u : 0u;
        }
        const bool margins = completed && k >= 2;
        const uint32_t runner = margins ? (uint32_t)(hi - second) : 0u, spread = margins ? (uint32_t)(hi - lo) : 0u;
        grec[id] = make_uint4(rounds | (completed ? 1u << 16 : 0u) | (margins ? 1u << 17 : 0u), runner, spread, n_target);
        atomicAdd(&cnt[GC_ATTEMPTED], 1u);
        atomicAdd(&cnt[completed ? GC_COMPLETED : GC_SAFETY], 1u);
        if (n_target >= 2) atomicAdd(&cnt[GC_MULTI], 1u);
        hist_add(h_rounds, wr, rounds, sp, -1, SPILL_ROUNDS);
        if (margins) hist_add(h_runner, wm, runner, sp, -1, SPILL_RUNNER);
    }
    __syncthreads();
    hist_flush(h_rounds, wr, g_rounds);
    hist_flush(h_runner, wm, g_runner);
    hist_flush(cnt, N_COUNTS, g_counts);
}

// grid = (S, n_seg); LDS: rounds [wr] | runner [wm] | spread [wm] | counts [4].  Output rows have rb / mb bins (>= wr / wm).
__global__ __launch_bounds__(256) void fk_game_stats_gather_kernel(const uint4 *grec, const uint16_t *inv_T, uint32_t perm_slots, uint32_t S,
                                                                   uint32_t k, uint32_t gps, uint32_t n_sh, uint32_t rows_per_seg,
                                                                   uint32_t wr, uint32_t wm, uint32_t rb, uint32_t mb,
                                                                   unsigned long long *s_counts, unsigned long long *s_rounds,
                                                                   unsigned long long *s_runner, unsigned long long *s_spread, Spill sp) {
    extern __shared__ uint32_t lds[];
    uint32_t *h_rounds = lds, *h_runner = lds + wr, *h_spread = lds + wr + wm, *cnt = lds + wr + 2 * wm;
    const uint32_t s = blockIdx.x;
    const uint32_t first = blockIdx.y * rows_per_seg, last = min(first + rows_per_seg, n_sh);
    if (first >= last) return; // (uniform over the workgroup)
    for (uint32_t i = threadIdx.x; i < wr + 2 * wm + N_COUNTS; i += blockDim.x) lds[i] = 0;
    __syncthreads();
    uint32_t n_att = 0, n_comp = 0, n_multi = 0;
    for (uint32_t sh = first + threadIdx.x; sh < last; sh += blockDim.x) {
        const uint32_t p = perm_at(inv_T, S, perm_slots, sh, s); // position = game * k + seat of the strategy in this shuffle
        const uint4 r = grec[(size_t)sh * gps + p / k];
        ++n_att;
        n_comp += (r.x >> 16) & 1u;
        n_multi += r.w >= 2 ? 1u : 0u;
        hist_add(h_rounds, wr, r.x & 0xffffu, sp, (int32_t)s, SPILL_ROUNDS);
        if ((r.x >> 17) & 1u) {
            hist_add(h_runner, wm, r.y, sp, (int32_t)s, SPILL_RUNNER);
            hist_add(h_spread, wm, r.z, sp, (int32_t)s, SPILL_SPREAD);
        }
    }
    if (n_att) {
        atomicAdd(&cnt[GC_ATTEMPTED], n_att);
        atomicAdd(&cnt[GC_COMPLETED], n_comp);
        atomicAdd(&cnt[GC_SAFETY], n_att - n_comp);
        atomicAdd(&cnt[GC_MULTI], n_multi);
    }
    __syncthreads();
    hist_flush(h_rounds, wr, s_rounds + (size_t)s * rb);
    hist_flush(h_runner, wm, s_runner + (size_t)s * mb);
    hist_flush(h_spread, wm, s_spread + (size_t)s * mb);
    hist_flush(cnt, N_COUNTS, s_counts + (size_t)s * N_COUNTS);
}

} // namespace fkg
