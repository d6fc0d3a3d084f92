// fk_agreement.h — the method agreement of a round robin on the device (fk_agreement_pairs, fk_rr_agreement, fk_rank_concordance),
// included by farkle_hip.hip behind fk_rr_inference.h.  What the reference's analysis/structure_agreement.py computes per pair
// (_pair_agreement :73-125) and over the scored population (kendalltau's pair counts), from the decision classes of the inference
// and the two screening ranks of every table row.
//
//   ag_pair_code             class + the ranks of rows i and j -> one byte: bits 0-1 h2h_direction, 2-3 win_rate_preference, 4-5
//                            trueskill_preference, each 0 none / 1 a / 2 b (_h2h_direction :65-70, _preference :55-62); plain
//                            __host__ __device__ C++, which tests/native/agreement_host_check.hip walks without a GPU
//   fk_ag_pairs_kernel       grid-stride over pair ids: the class byte coalesced, the rank pairs of both rows, the code byte stored
//                            when codes are wanted; the eleven counters as popcounts of wave ballots, kept per wave across trips,
//                            then summed over the workgroup's waves in LDS: one 64-bit atomicAdd per counter per workgroup
//   cc_relation, cc_row_counts   one item against one other / against a run of columns: concordant, discordant, tied in x only, tied
//                            in y only, tied in both — by comparison, never by subtraction
//   fk_ag_concordance_kernel one workgroup per tile of the upper triangle of the m x m comparison, tile edge CC_TILE: the column
//                            tile's keys in LDS, one row per thread in registers, the diagonal tile masked to j > i, the ragged
//                            last tile to < m; u32 counts per thread, a wave sum, the waves in LDS, five 64-bit atomics
//
// Vector stores and ordinary atomics only.  Every result is an integer.
#pragma once

#include <cstdint>

namespace fkag {
namespace { // internal linkage, as fk_round_robin.h

using ull = unsigned long long;

constexpr uint32_t AG_COUNTS = FK_AGREE_COUNTS;
constexpr uint32_t AG_BLOCK = 256;
constexpr uint32_t AG_WAVES = AG_BLOCK / 64u;
constexpr uint32_t AG_MAX_GRID = 2048; // a grid-stride kernel gains nothing beyond a few workgroups per compute unit
constexpr int32_t AG_NO_RANK = FK_AGREE_NO_RANK;
constexpr uint32_t CC_COUNTS = FK_CONCORDANCE_COUNTS;
constexpr uint32_t CC_TILE = FK_CONCORDANCE_TILE; // rows of a tile = threads of its workgroup = columns in LDS

// the counters (include/farkle_hip.h)
enum : uint32_t {
    AG_PAIRS = 0, AG_DIRECTIONAL, AG_UNRESOLVED, AG_NONVIABLE, AG_EQUIVALENT, AG_WT_AVAILABLE, AG_WT_AGREE, AG_HW_AVAILABLE, AG_HW_AGREE,
    AG_HT_AVAILABLE, AG_HT_AGREE
};
enum : uint32_t { CC_CONCORDANT = 0, CC_DISCORDANT, CC_TIED_X, CC_TIED_Y, CC_TIED_BOTH };

// 0 none, 1 a, 2 b: classes 0 and 2 are won by A, 1 and 3 by B, 4 .. 6 by neither
__host__ __device__ inline uint32_t ag_direction(uint32_t cls) { return cls < 4u ? 1u + (cls & 1u) : 0u; }

// none when a rank is null or the two are equal; otherwise the smaller rank is preferred
__host__ __device__ inline uint32_t ag_preference(int32_t rank_a, int32_t rank_b) {
    if (rank_a == AG_NO_RANK || rank_b == AG_NO_RANK || rank_a == rank_b) return 0u;
    return rank_a < rank_b ? 1u : 2u;
}

__host__ __device__ inline uint32_t ag_pair_code(uint32_t cls, int32_t win_a, int32_t win_b, int32_t ts_a, int32_t ts_b) {
    return ag_direction(cls) | ag_preference(win_a, win_b) << 2 | ag_preference(ts_a, ts_b) << 4;
}

// `ranks[row]` = (win_rate_rank, trueskill_rank).  `counts` [AG_COUNTS], zeroed.  Every lane of a workgroup makes the same trips.
__global__ __launch_bounds__(AG_BLOCK) void fk_ag_pairs_kernel(const uint8_t *__restrict__ cls, const int2 *__restrict__ ranks, uint32_t n, uint32_t n_pairs,
                                                               uint8_t *__restrict__ codes, ull *__restrict__ counts) {
    __shared__ uint32_t part[AG_WAVES][AG_COUNTS];
    uint32_t acc[AG_COUNTS]; // of this wave: at most n_pairs < 2^31 each
#pragma unroll
    for (uint32_t k = 0; k < AG_COUNTS; ++k) acc[k] = 0u;
    const uint32_t stride = gridDim.x * AG_BLOCK; // at most 2^19: base + stride stays below 2^32
    for (uint32_t base = blockIdx.x * AG_BLOCK; base < n_pairs; base += stride) {
        const uint32_t p = base + threadIdx.x;
        const bool live = p < n_pairs;
        uint32_t c = 7u, code = 0u;
        if (live) {
            uint32_t i, j;
            fkrr::rr_unrank(n, p, i, j);
            c = cls[p];
            const int2 a = ranks[i], b = ranks[j];
            code = ag_pair_code(c, a.x, b.x, a.y, b.y);
            if (codes) codes[p] = (uint8_t)code;
        }
        const uint32_t h = code & 3u, w = (code >> 2) & 3u, t = (code >> 4) & 3u;
        acc[AG_PAIRS] += (uint32_t)__popcll(__ballot(live));
        acc[AG_DIRECTIONAL] += (uint32_t)__popcll(__ballot(h != 0u));
        acc[AG_UNRESOLVED] += (uint32_t)__popcll(__ballot(c == 5u || c == 6u));
        acc[AG_NONVIABLE] += (uint32_t)__popcll(__ballot(c == 6u));
        acc[AG_EQUIVALENT] += (uint32_t)__popcll(__ballot(c == 4u));
        acc[AG_WT_AVAILABLE] += (uint32_t)__popcll(__ballot(w != 0u && t != 0u));
        acc[AG_WT_AGREE] += (uint32_t)__popcll(__ballot(w != 0u && w == t));
        acc[AG_HW_AVAILABLE] += (uint32_t)__popcll(__ballot(h != 0u && w != 0u));
        acc[AG_HW_AGREE] += (uint32_t)__popcll(__ballot(h != 0u && h == w));
        acc[AG_HT_AVAILABLE] += (uint32_t)__popcll(__ballot(h != 0u && t != 0u));
        acc[AG_HT_AGREE] += (uint32_t)__popcll(__ballot(h != 0u && h == t));
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < AG_COUNTS; ++k) part[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < AG_COUNTS) {
        ull sum = 0ull;
        for (uint32_t wv = 0; wv < AG_WAVES; ++wv) sum += part[wv][threadIdx.x];
        if (sum) atomicAdd(&counts[threadIdx.x], sum);
    }
}

// how item (x, y) stands to item (cx, cy): one of CC_*
__host__ __device__ inline uint32_t cc_relation(int32_t x, int32_t y, int32_t cx, int32_t cy) {
    const bool tie_x = x == cx, tie_y = y == cy;
    if (tie_x) return tie_y ? CC_TIED_BOTH : CC_TIED_X;
    if (tie_y) return CC_TIED_Y;
    return (x < cx) == (y < cy) ? CC_CONCORDANT : CC_DISCORDANT;
}

// Row `row` of a tile against the tile's columns col0 .. col0 + cols - 1 (keys cx[k], cy[k]): the columns above `row` only, which
// masks the diagonal tile to j > i and changes nothing in a tile right of it.  Adds to out[CC_COUNTS].
__host__ __device__ inline void cc_row_counts(int32_t x, int32_t y, uint32_t row, uint32_t col0, uint32_t cols, const int32_t *cx, const int32_t *cy,
                                              uint32_t *out) {
    for (uint32_t k = 0; k < cols; ++k) {
        const uint32_t r = col0 + k > row ? cc_relation(x, y, cx[k], cy[k]) : CC_COUNTS;
#pragma unroll
        for (uint32_t q = 0; q < CC_COUNTS; ++q) out[q] += r == q ? 1u : 0u; // (no indexed register array)
    }
}

__device__ inline uint32_t ag_wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Grid: the T (T + 1) / 2 tiles (bi <= bj) of T = ceil(m / CC_TILE) tile rows, CC_TILE threads.  Tile t is pair t of T + 1 items
// shifted by one column: (bi, bj + 1) = rr_unrank(T + 1, t).  `counts` [CC_COUNTS], zeroed.
__global__ __launch_bounds__(CC_TILE) void fk_ag_concordance_kernel(const int32_t *__restrict__ x, const int32_t *__restrict__ y, uint32_t m, uint32_t tiles,
                                                                    ull *__restrict__ counts) {
    __shared__ int32_t col_x[CC_TILE], col_y[CC_TILE];
    __shared__ uint32_t part[CC_TILE / 64u][CC_COUNTS];
    uint32_t bi, bj;
    fkrr::rr_unrank(tiles + 1u, blockIdx.x, bi, bj);
    bj -= 1u;
    const uint32_t col0 = bj * CC_TILE, cols = m - col0 < CC_TILE ? m - col0 : CC_TILE; // col0 < m: the tile exists
    const uint32_t col = col0 + threadIdx.x, row = bi * CC_TILE + threadIdx.x;
    col_x[threadIdx.x] = col < m ? x[col] : 0;
    col_y[threadIdx.x] = col < m ? y[col] : 0;
    __syncthreads();
    uint32_t mine[CC_COUNTS] = {0u, 0u, 0u, 0u, 0u};
    if (row < m) cc_row_counts(x[row], y[row], row, col0, cols, col_x, col_y, mine);
#pragma unroll
    for (uint32_t k = 0; k < CC_COUNTS; ++k) {
        const uint32_t s = ag_wave_sum(mine[k]);
        if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < CC_COUNTS) {
        ull sum = 0ull;
        for (uint32_t wv = 0; wv < CC_TILE / 64u; ++wv) sum += part[wv][threadIdx.x];
        if (sum) atomicAdd(&counts[threadIdx.x], sum);
    }
}

} // namespace
} // namespace fkag
