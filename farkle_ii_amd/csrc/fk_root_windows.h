// fk_root_windows.h — the two-root stability stage's window estimates on the device (fk_root_window_estimates), included by
// farkle_hip.hip behind fk_performance.h.  What the reference's analysis/root_stability.py sums over a row window of one cell's batch
// matrix (_estimate_matrix_cells :411-433): five integer column totals, the positive-batch count and the three float64 sums
// sum(w * w), sum(w * e), sum(e * e) its batch mcse is made of.  _matched_count_convergence (:1429-1513) and _half_drift
// (:1516-1628) repeat that for prefixes and halves of every cell; here all of a stage's windows go through one call.
//
//   THE ORDER.  np.sum(x, axis=0) over a C-contiguous [R][w] array adds row by row when w >= 2, and collapses to a vector summed by
//   np_add_reduce (fk_performance.h) when w == 1.  The reference slices the columns in chunks, so a column is of the second kind when
//   its chunk has width 1; the caller names the first such column of a window (pairwise_begin, farkle_ii_amd/root_stability.py:
//   window_pairwise_begin).  Both orders are stated here once, as plain __host__ __device__ C++ that
//   tests/native/root_windows_host_check.hip walks without a GPU against NumPy itself:
//   walk_column             one column from `row_begin` down, in ascending row order, the running sums snapshot at every row_end of
//                           the group's windows (ascending).  Sequential, so the prefixes of one first row cost one pass and every
//                           snapshot has the bits of a walk of its own.  The loads of ROWS_IN_FLIGHT rows are issued before their
//                           dependent adds.
//   pairwise_column         the three float sums of one window's column through np_add_reduce over the window's rows (every row is
//                           an element: a row without an exposure contributes 0.0, as the reference's np.where does).
//   fk_rw_walk_kernel       one lane task = (group of windows of one cell that share row_begin, column); the column sits on the lane, so
//                           a matrix row is read coalesced.  Tasks = groups x column blocks, strided over the grid.
//   fk_rw_pairwise_kernel   one lane task = (window with pairwise columns, column >= pairwise_begin); overwrites the float sums the
//                           walk left for these columns.  Launched behind the walk on the same stream.
//
// A count is exact as a double below 2^53 and the entry refuses totals beyond 2^62, so (double)w is one rounding; every product and
// every addition is its own IEEE operation (`#pragma clang fp contract(off)`).  A (window, column) is owned by one lane: no result
// depends on the grid.  All results leave through plain vector stores.
#pragma once

#include <cstdint>

#include "fk_performance.h"

namespace fkw {
namespace { // internal linkage, as fk_performance.h

constexpr uint32_t COLUMN_BLOCK = 64;  // columns per workgroup: one wave
constexpr uint32_t ROWS_IN_FLIGHT = 4; // rows whose 4 loads are issued together: 16 independent loads ahead of the add chain
constexpr uint32_t MAX_GRID = 8192;    // workgroups of a launch at most (option "root_windows_grid" caps lower)
constexpr uint32_t N_TOTALS = 6;       // wins | exposures | completed | safety | losses | positive batches
constexpr uint32_t N_SUMS = 3;         // sum_w2 | sum_we | sum_e2

struct Cell { // one cell's four row-major int64 [B][S] matrices
    const int64_t *w, *e, *c, *f;
    int64_t B;
};
struct Group { // the windows of one cell that share their first row; their snapshots lie at snaps[first .. first + count), ascending row_end
    uint32_t cell, first, count, pad;
    int64_t row_begin;
};
struct Snap {
    int64_t row_end;
    uint32_t window;         // the window's position in the caller's list
    uint32_t pairwise_begin; // float sums are stored for the columns below it only
};
struct PairTask { // a window with pairwise columns
    uint32_t cell, window, pairwise_begin, pad;
    int64_t row_begin, row_end;
};

struct Running {
    long long w = 0, e = 0, c = 0, f = 0, positive = 0;
    double w2 = 0.0, we = 0.0, e2 = 0.0;
};

__host__ __device__ inline void add_row(Running &a, long long w, long long e, long long c, long long f) {
#pragma clang fp contract(off)
    a.w += w, a.e += e, a.c += c, a.f += f;
    a.positive += e > 0 ? 1 : 0;
    // (a row without an exposure has no win either — the entry checks wins <= completed <= exposures — so its products are the 0.0
    // the reference's mask puts there)
    const double dw = (double)w, de = (double)e;
    const double p_ww = dw * dw, p_we = dw * de, p_ee = de * de;
    a.w2 = a.w2 + p_ww;
    a.we = a.we + p_we;
    a.e2 = a.e2 + p_ee;
}

// totals: int64 [n_windows][N_TOTALS][S]; sums: double [n_windows][N_SUMS][S].  W .. F point at the column's cell of row 0.
__host__ __device__ inline void store_snapshot(const Running &a, const Snap &snap, uint32_t s, size_t S, long long *totals, double *sums) {
    long long *t = totals + (size_t)snap.window * N_TOTALS * S + s;
    t[0] = a.w, t[S] = a.e, t[2 * S] = a.c, t[3 * S] = a.f, t[4 * S] = a.e - a.w, t[5 * S] = a.positive;
    if (s < snap.pairwise_begin) {
        double *d = sums + (size_t)snap.window * N_SUMS * S + s;
        d[0] = a.w2, d[S] = a.we, d[2 * S] = a.e2;
    }
}

__host__ __device__ inline void walk_column(const int64_t *W, const int64_t *E, const int64_t *C, const int64_t *F, size_t S, uint32_t s,
                                            int64_t row_begin, const Snap *snaps, uint32_t n_snaps, long long *totals, double *sums) {
    Running a;
    int64_t r = row_begin;
    for (uint32_t i = 0; i < n_snaps; ++i) {
        const int64_t end = snaps[i].row_end; // ascending: a snapshot at the row the one before ended at walks nothing
        for (; r + (int64_t)ROWS_IN_FLIGHT <= end; r += ROWS_IN_FLIGHT) {
            long long w[ROWS_IN_FLIGHT], e[ROWS_IN_FLIGHT], c[ROWS_IN_FLIGHT], f[ROWS_IN_FLIGHT];
#pragma unroll
            for (uint32_t j = 0; j < ROWS_IN_FLIGHT; ++j) {
                const size_t at = (size_t)(r + j) * S;
                w[j] = W[at], e[j] = E[at], c[j] = C[at], f[j] = F[at];
            }
#pragma unroll
            for (uint32_t j = 0; j < ROWS_IN_FLIGHT; ++j) add_row(a, w[j], e[j], c[j], f[j]);
        }
        for (; r < end; ++r) {
            const size_t at = (size_t)r * S;
            add_row(a, W[at], E[at], C[at], F[at]);
        }
        store_snapshot(a, snaps[i], s, S, totals, sums);
    }
}

// x * y of two int64 columns as a stream of doubles, one element per row
struct ProductStream {
    const int64_t *x, *y;
    size_t stride;
    __host__ __device__ inline double operator()() {
#pragma clang fp contract(off)
        const double a = (double)(long long)*x, b = (double)(long long)*y;
        x += stride, y += stride;
        return a * b;
    }
};

// W, E point at the column's cell of row 0; sums as above
__host__ __device__ inline void pairwise_column(const int64_t *W, const int64_t *E, size_t S, uint32_t s, int64_t row_begin, int64_t row_end,
                                                uint32_t window, double *sums) {
    const uint64_t n = (uint64_t)(row_end - row_begin);
    const int64_t *w0 = W + (size_t)row_begin * S, *e0 = E + (size_t)row_begin * S;
    double *d = sums + (size_t)window * N_SUMS * S + s;
    ProductStream ww{w0, w0, S}, we{w0, e0, S}, ee{e0, e0, S};
    d[0] = fkp::np_add_reduce(ww, n);
    d[S] = fkp::np_add_reduce(we, n);
    d[2 * S] = fkp::np_add_reduce(ee, n);
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(COLUMN_BLOCK) void fk_rw_walk_kernel(const Cell *cells, const Group *groups, const Snap *snaps, uint32_t n_groups,
                                                                   uint32_t S, long long *totals, double *sums) {
    const uint32_t column_blocks = (S + COLUMN_BLOCK - 1u) / COLUMN_BLOCK;
    const uint64_t n_tasks = (uint64_t)n_groups * column_blocks;
    for (uint64_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
        const Group g = groups[task / column_blocks];
        const uint32_t s = (uint32_t)(task % column_blocks) * COLUMN_BLOCK + threadIdx.x;
        if (s >= S) continue;
        const Cell cell = cells[g.cell];
        walk_column(cell.w + s, cell.e + s, cell.c + s, cell.f + s, (size_t)S, s, g.row_begin, snaps + g.first, g.count, totals, sums);
    }
}

__global__ __launch_bounds__(COLUMN_BLOCK) void fk_rw_pairwise_kernel(const Cell *cells, const PairTask *tasks, uint32_t n_pair_tasks, uint32_t S,
                                                                       double *sums) {
    const uint32_t column_blocks = (S + COLUMN_BLOCK - 1u) / COLUMN_BLOCK;
    const uint64_t n_tasks = (uint64_t)n_pair_tasks * column_blocks;
    for (uint64_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
        const PairTask t = tasks[task / column_blocks];
        // the column blocks count from pairwise_begin: a window whose last column alone is pairwise occupies one lane of one block
        const uint64_t s = (uint64_t)t.pairwise_begin + (task % column_blocks) * COLUMN_BLOCK + threadIdx.x;
        if (s >= S) continue;
        const Cell cell = cells[t.cell];
        pairwise_column(cell.w + s, cell.e + s, (size_t)S, (uint32_t)s, t.row_begin, t.row_end, t.window, sums);
    }
}
#endif // __HIPCC__

} // namespace
} // namespace fkw
