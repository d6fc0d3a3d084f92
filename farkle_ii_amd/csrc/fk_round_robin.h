// fk_round_robin.h — head-to-head round robin: every pair of a strategy table in one call (fk_h2h_round_robin), included by
// farkle_hip.hip behind fk_kernels.h.  Everything the host loop of fk_h2h_run_blocks does per block happens here on the device:
//
//   rr_unrank                pair id -> (i, j), the position in itertools.combinations(range(n), 2) (h2h_schedule.py:564); plain
//                            __host__ __device__ C++, which tests/native/round_robin_host_check.hip checks without a GPU
//   fk_rr_window_kernel      the window's strategy rows strat[2 row + seat] and patience rows, by unranking the n-row table
//   fk_rr_need_kernel        per block: the attempts the next generation plays, min(max_attempts - attempted, target - completed),
//                            0 for a terminal block; and the flag "plays in this generation"
//   (hipcub ExclusiveSum     over the needs: the generation's game offsets; over the flags: the index among the playing blocks)
//   fk_rr_compact_kernel     the playing blocks' rows, in order
//   fk_rr_pass_bounds_kernel one lane per pass: the playing blocks its game range [pass * max_launch, ...) cuts (binary search)
//   fk_rr_pass_blocks_kernel the DevBlocks of one pass: pair, attempt0, order, pass-local start, window row
//   fk_rr_apply_kernel       after fk_h2h_reduce_kernel: state += planned attempts and the generation's counts, with the
//                            conservation check (completed + safety == planned, wins1 + wins2 == completed) on the device
//   fk_rr_summary_kernel     one lane per pair of a finished window -> the per-strategy summary (FK_RR_SUMMARY_COLS columns)
//
// A block is window row `row`: pair = window's first pair + row / 2, order = row & 1; order 0 seats table[i] in seat 1 and
// table[j] in seat 2, order 1 swaps them (h2h_schedule.py:567-568).  The game kernel, fk_block_map_kernel, fk_pool_kernel, the
// seed stage and fk_h2h_reduce_kernel see such a window exactly as they see the block list of an fk_h2h_run_blocks call.
#pragma once

#include <cmath>
#include <cstdint>

namespace fkrr {
namespace { // internal linkage, as fk_kernels.h: a host-only build that launches none of the kernels links without their code object

constexpr uint32_t RR_STATE = 5; // attempted, completed, safety, wins_seat1, wins_seat2 (FK_RR_STATE_COLS)
constexpr uint32_t RR_COLS = 8;  // FK_RR_SUMMARY_COLS
enum : uint32_t { RC_PAIRS = 0, RC_RESOLVED, RC_COMPLETED, RC_SAFETY, RC_WINS, RC_SEAT1_COMPLETED, RC_SEAT1_WINS, RC_AHEAD };

// pairs of an n-row table in front of row i: (i, i + 1) is pair i (2n - i - 1) / 2
__host__ __device__ inline uint64_t rr_row_begin(uint64_t n, uint64_t i) { return i * (2u * n - i - 1u) / 2u; }

// pair id -> (i, j), i < j.  Closed form in double, then an integer fix-up: (2n - 1)^2 is exact in a double up to n = 4.7 x 10^7
// and the fix-up absorbs the rounding of larger tables (the discriminant is off by 2^11 at most, the root by far less than 1).
__host__ __device__ inline void rr_unrank(uint32_t n, uint64_t pair_id, uint32_t &i_out, uint32_t &j_out) {
    const double b = 2.0 * (double)n - 1.0;
    double disc = b * b - 8.0 * (double)pair_id;
    if (disc < 0.0) disc = 0.0;
    int64_t i = (int64_t)((b - sqrt(disc)) * 0.5);
    if (i < 0) i = 0;
    if (i > (int64_t)n - 2) i = (int64_t)n - 2;
    while (i > 0 && rr_row_begin(n, (uint64_t)i) > pair_id) --i;
    while (i < (int64_t)n - 2 && rr_row_begin(n, (uint64_t)i + 1u) <= pair_id) ++i;
    i_out = (uint32_t)i;
    j_out = (uint32_t)((uint64_t)i + 1u + (pair_id - rr_row_begin(n, (uint64_t)i)));
}

// the error record of a call: [0] 0 = none, else 1; [1] the window row of the first block that broke conservation
struct RrError {
    uint32_t raised, row;
};

__global__ void fk_rr_window_kernel(const uint2 *__restrict__ table, const uint8_t *__restrict__ table_patience, uint32_t n, uint64_t pair0,
                                    uint32_t n_rows, uint2 *__restrict__ strat, uint8_t *__restrict__ patience) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    uint32_t i, j;
    rr_unrank(n, pair0 + (row >> 1), i, j);
    const uint32_t s1 = (row & 1u) ? j : i, s2 = (row & 1u) ? i : j;
    strat[2u * row] = table[s1];
    strat[2u * row + 1u] = table[s2];
    patience[2u * row] = table_patience[s1];
    patience[2u * row + 1u] = table_patience[s2];
}

// need[n_rows] = flag[n_rows] = 0: the scans run over n_rows + 1 items, so that their last outputs are the totals
__global__ void fk_rr_need_kernel(const uint32_t *__restrict__ state, uint32_t n_rows, uint32_t target, uint32_t max_attempts,
                                  unsigned long long *__restrict__ need, uint32_t *__restrict__ flag) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row > n_rows) return;
    uint32_t nd = 0;
    if (row < n_rows) {
        const uint32_t attempted = state[row * RR_STATE], completed = state[row * RR_STATE + 1u];
        if (attempted < max_attempts && completed < target) nd = min(max_attempts - attempted, target - completed);
    }
    need[row] = nd;
    flag[row] = nd ? 1u : 0u;
}

__global__ void fk_rr_compact_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ aidx, uint32_t n_rows,
                                     uint32_t *__restrict__ act) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row < n_rows && flag[row]) act[aidx[row]] = row;
}

// Pass p plays games [p * max_launch, min(total, (p + 1) * max_launch)) of the generation.  Its blocks are the playing blocks
// [lo, hi): lo = the first whose range ends behind the pass's first game, hi = the first that begins at or behind its end.
__global__ void fk_rr_pass_bounds_kernel(const unsigned long long *__restrict__ off, const unsigned long long *__restrict__ need,
                                         const uint32_t *__restrict__ act, uint32_t n_act, unsigned long long total,
                                         unsigned long long max_launch, uint32_t n_passes, uint32_t *__restrict__ bounds /* [n_passes][2] */) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_passes) return;
    const unsigned long long g0 = (unsigned long long)p * max_launch, g1 = min(total, g0 + max_launch);
    uint32_t lo = 0, hi = n_act;
    while (lo < hi) { // first a with off + need > g0
        const uint32_t mid = (lo + hi) >> 1, r = act[mid];
        if (off[r] + need[r] > g0) hi = mid;
        else lo = mid + 1u;
    }
    const uint32_t first = lo;
    hi = n_act;
    while (lo < hi) { // first a with off >= g1
        const uint32_t mid = (lo + hi) >> 1;
        if (off[act[mid]] >= g1) hi = mid;
        else lo = mid + 1u;
    }
    bounds[2u * p] = first;
    bounds[2u * p + 1u] = lo;
}

__global__ void fk_rr_pass_blocks_kernel(const unsigned long long *__restrict__ off, const uint32_t *__restrict__ act,
                                         const uint32_t *__restrict__ state, uint32_t first, uint32_t n_blocks, unsigned long long g0,
                                         uint64_t pair0, DevBlock *__restrict__ blocks) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_blocks) return;
    const uint32_t row = act[first + q];
    const unsigned long long o = off[row];
    DevBlock b;
    b.pair = pair0 + (row >> 1);
    b.attempt0 = (uint64_t)state[row * RR_STATE] + (o < g0 ? g0 - o : 0ull); // a block may straddle passes
    b.order = row & 1u;
    b.start = o > g0 ? (uint32_t)(o - g0) : 0u;
    b.row = row;
    b.pad = 0u;
    blocks[q] = b;
}

// out[row] = {completed, safety, wins_seat1, wins_seat2} of the generation (fk_h2h_reduce_kernel), need[row] the attempts planned
__global__ void fk_rr_apply_kernel(uint32_t *__restrict__ state, const unsigned long long *__restrict__ need,
                                   const unsigned long long *__restrict__ out, uint32_t n_rows, RrError *__restrict__ err) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const unsigned long long planned = need[row];
    const unsigned long long comp = out[(size_t)row * 4u], saf = out[(size_t)row * 4u + 1u], w1 = out[(size_t)row * 4u + 2u],
                             w2 = out[(size_t)row * 4u + 3u];
    if (comp + saf != planned || w1 + w2 != comp) {
        if (atomicCAS(&err->raised, 0u, 1u) == 0u) err->row = row;
        return;
    }
    if (!planned) return;
    uint32_t *s = state + (size_t)row * RR_STATE;
    s[0] += (uint32_t)planned;
    s[1] += (uint32_t)comp;
    s[2] += (uint32_t)saf;
    s[3] += (uint32_t)w1;
    s[4] += (uint32_t)w2;
}

// One lane per pair of a finished window.  Pair ids ascend with the lane, so the lanes of a wave that share row i are adjacent:
// their row-i contributions are summed by a segmented scan over the wave (a lane takes its neighbour at distance d only when
// that neighbour has the same i) and leave with one 64-bit atomic per column from the last lane of each segment.  The j side is
// one atomic per lane and column: consecutive lanes hit consecutive rows.
__global__ void fk_rr_summary_kernel(const uint32_t *__restrict__ state, uint32_t n, uint64_t pair0, uint32_t n_pairs, uint32_t target,
                                     unsigned long long *__restrict__ summary /* [n][RR_COLS] */) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // blockDim is a multiple of 64: whole waves
    const bool live = p < n_pairs;
    uint32_t i = 0xffffffffu, j = 0xffffffffu;
    uint32_t vi[RR_COLS], vj[RR_COLS];
#pragma unroll
    for (uint32_t c = 0; c < RR_COLS; ++c) vi[c] = vj[c] = 0u;
    if (live) {
        rr_unrank(n, pair0 + p, i, j);
        const uint32_t *a = state + (size_t)p * 2u * RR_STATE, *b = a + RR_STATE; // order 0: i in seat 1; order 1: j in seat 1
        const uint32_t resolved = (a[1] >= target && b[1] >= target) ? 1u : 0u;
        const uint32_t wins_i = a[3] + b[4], wins_j = a[4] + b[3];
        vi[RC_PAIRS] = vj[RC_PAIRS] = 1u;
        vi[RC_RESOLVED] = vj[RC_RESOLVED] = resolved;
        vi[RC_COMPLETED] = vj[RC_COMPLETED] = a[1] + b[1];
        vi[RC_SAFETY] = vj[RC_SAFETY] = a[2] + b[2];
        vi[RC_WINS] = wins_i;
        vj[RC_WINS] = wins_j;
        vi[RC_SEAT1_COMPLETED] = a[1];
        vj[RC_SEAT1_COMPLETED] = b[1];
        vi[RC_SEAT1_WINS] = a[3];
        vj[RC_SEAT1_WINS] = b[3];
        vi[RC_AHEAD] = (resolved && wins_i > wins_j) ? 1u : 0u;
        vj[RC_AHEAD] = (resolved && wins_j > wins_i) ? 1u : 0u;
    }
    const uint32_t lane = lane_id();
    unsigned long long acc[RR_COLS];
#pragma unroll
    for (uint32_t c = 0; c < RR_COLS; ++c) acc[c] = vi[c];
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t i_up = __shfl_up(i, d, 64);
        const bool take = lane >= d && i_up == i;
#pragma unroll
        for (uint32_t c = 0; c < RR_COLS; ++c) {
            const unsigned long long up = __shfl_up(acc[c], d, 64);
            if (take) acc[c] += up;
        }
    }
    const uint32_t i_next = __shfl_down(i, 1u, 64);
    if (live && (lane == 63u || i_next != i)) {
#pragma unroll
        for (uint32_t c = 0; c < RR_COLS; ++c)
            if (acc[c]) atomicAdd(&summary[(size_t)i * RR_COLS + c], acc[c]);
    }
    if (live) {
#pragma unroll
        for (uint32_t c = 0; c < RR_COLS; ++c)
            if (vj[c]) atomicAdd(&summary[(size_t)j * RR_COLS + c], (unsigned long long)vj[c]);
    }
}

} // namespace
} // namespace fkrr
