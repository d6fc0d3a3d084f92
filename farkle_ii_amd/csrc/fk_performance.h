// fk_performance.h — the performance stage's point estimates on the device (fk_performance_by_k, fk_performance_across_k), included by
// farkle_hip.hip behind fk_power_plan.h.  What the reference's analysis/performance.py computes from a player count's batch matrix
// (_estimate_one_k_matrix :425-542) and from the per-k chance deltas of the complete-support strategies (_across_k_estimates :575-687,
// _pareto_membership :547-572): the tables the joint batch bootstrap (fk_bootstrap.h) is the uncertainty for.
//
//   np_add_reduce           NumPy's float64 add.reduce over a contiguous vector, the order np.sum, np.mean and np.std share: the vector in
//                           buffers of 8 192 elements, each buffer by the pairwise tree (halves rounded down to a multiple of 8 until a
//                           block has 128 elements or fewer), a block by eight strided accumulators combined as
//                           ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) and a sequential tail, a block below 8 elements
//                           sequentially from 0.0.  The elements come from a stream functor in their order, so the vector — a column's
//                           positive-exposure rates, compacted — never exists.  Plain __host__ __device__ C++: the one statement of the
//                           order, which tests/native/performance_host_check.hip walks without a GPU against NumPy itself.
//   fk_perf_by_k_kernel     one lane per strategy column (a matrix row is read coalesced along S), the columns strided over the grid.
//                           Three walks down the column in ascending batch order: the integer totals and the positive-exposure count;
//                           rate_sum = add.reduce(wins / exposures over the positive rows); ssd = add.reduce((r - mean) * (r - mean)).
//   fk_perf_rows_kernel     one lane per complete-support strategy: add.reduce of its d chance deltas and of its d variances, the first
//                           position of its minimum (np.argmin), and the maximum of the minima by a wave reduction and one atomic on
//                           order-preserving keys.
//   fk_perf_pareto_kernel   one wave per workgroup owns 64 candidate rows in registers; all n rows stream through LDS in tiles of PT rows
//                           (every lane reads the same tile row: a broadcast, no bank conflict).  A candidate is dominated when a row
//                           is >= in every coordinate and > in one; equal rows, the candidate itself among them, dominate nothing.  The
//                           wave leaves once every lane is dominated.  Blocks of candidates are strided over the grid.
//   fk_perf_leader_kernel   the smallest row whose minimum lies within 1e-15 of the largest (np.isclose(rtol = 0, atol = 1e-15)).
//
// Every float operation is its own IEEE operation (`#pragma clang fp contract(off)`: hipcc would fuse (r - mean) * (r - mean) + acc).  A
// column and a row are owned by one lane, so no result depends on the grid.  Integer and flag results leave through plain vector stores.
#pragma once

#include <cstdint>

namespace fkp {
namespace { // internal linkage, as fk_power_plan.h

constexpr uint32_t NP_BLOCK = 128;    // PW_BLOCKSIZE of NumPy's pairwise sum
constexpr uint32_t NP_BUFFER = 8192;  // elements of one reduction buffer (np.getbufsize())
constexpr uint32_t NP_DEPTH = 9;      // a right half is at most half its node + 7: 8192 reaches a block in seven steps
constexpr uint32_t MAX_D = 16;        // player counts of an across-k call
constexpr uint32_t PT = 128;          // rows per LDS tile of the Pareto kernel: PT x MAX_D x 8 bytes = 16 KiB
constexpr uint32_t PARETO_BLOCK = 64; // candidates per workgroup: one wave
constexpr uint32_t COLUMN_BLOCK = 64; // columns per workgroup of the by-k kernel
constexpr uint32_t MAX_GRID = 4096;   // workgroups of a launch at most (option "performance_grid" caps lower)
constexpr double MAXIMIN_ATOL = 1e-15;

// one block of n <= NP_BLOCK elements from the stream
template <class Next>
__host__ __device__ inline double np_block_sum(Next &next, uint32_t n) {
#pragma clang fp contract(off)
    if (n < 8u) {
        double res = 0.0;
        for (uint32_t i = 0; i < n; ++i) res = res + next();
        return res;
    }
    double r[8];
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) r[j] = next();
    uint32_t i = 8u;
    for (; i < n - (n % 8u); i += 8u) {
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) r[j] = r[j] + next();
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + next();
    return res;
}

// the pairwise tree over n <= NP_BUFFER elements: sum(n) = sum(n2) + sum(n - n2), n2 = n / 2 rounded down to a multiple of 8, walked
// depth first with the left sums on a small stack (the stream hands out the elements in their order)
template <class Next>
__host__ __device__ inline double np_pairwise_sum(Next &next, uint32_t n) {
#pragma clang fp contract(off)
    uint32_t size[NP_DEPTH];
    double left[NP_DEPTH];
    bool right[NP_DEPTH]; // the node's left half is summed, its right half is under way
    uint32_t top = 0;
    size[0] = n;
    right[0] = false;
    for (;;) {
        uint32_t m = size[top];
        if (m > NP_BLOCK) { // descend into the left half
            uint32_t n2 = m / 2u;
            n2 -= n2 % 8u;
            size[top + 1u] = n2;
            right[top + 1u] = false;
            ++top;
            continue;
        }
        double value = np_block_sum(next, m);
        for (;;) { // hand the finished node's sum to its parent
            if (top == 0u) return value;
            --top;
            if (!right[top]) {
                left[top] = value;
                right[top] = true;
                m = size[top];
                uint32_t n2 = m / 2u;
                n2 -= n2 % 8u;
                size[top + 1u] = m - n2;
                right[top + 1u] = false;
                ++top;
                break;
            }
            value = left[top] + value;
        }
    }
}

// np.add.reduce of the n elements of the stream: 0.0, then one pairwise sum per buffer added in order
template <class Next>
__host__ __device__ inline double np_add_reduce(Next &next, uint64_t n) {
#pragma clang fp contract(off)
    double res = 0.0;
    while (n > 0u) {
        const uint32_t m = n < (uint64_t)NP_BUFFER ? (uint32_t)n : NP_BUFFER;
        res = res + np_pairwise_sum(next, m);
        n -= m;
    }
    return res;
}

// a vector in memory as a stream
struct ArrayStream {
    const double *p;
    __host__ __device__ inline double operator()() { return *p++; }
};

// ((x - mean) * (x - mean)) of a vector in memory: what np.std sums
struct SquaredDeviationStream {
    const double *p;
    double mean;
    __host__ __device__ inline double operator()() {
#pragma clang fp contract(off)
        const double d = *p++ - mean;
        return d * d;
    }
};

#if defined(__HIPCC__)
// the positive-exposure rates of one matrix column in ascending batch order; SQUARED: their squared deviations from `mean`
template <bool SQUARED>
struct ColumnStream {
    const int64_t *w, *e; // the column's cell of the next row
    size_t stride;        // S
    double mean;
    __device__ inline double operator()() {
#pragma clang fp contract(off)
        long long ev = *e;
        while (ev <= 0) { // (the caller asks for exactly as many elements as the column has positive rows)
            w += stride, e += stride;
            ev = *e;
        }
        const double r = (double)(long long)*w / (double)ev;
        w += stride, e += stride;
        if (!SQUARED) return r;
        const double d = r - mean;
        return d * d;
    }
};

// out: int64 [6][S] = wins | exposures | completed | safety | losses | positive batches; sums: double [2][S] = rate_sum | ssd
__global__ __launch_bounds__(COLUMN_BLOCK) void fk_perf_by_k_kernel(const int64_t *W, const int64_t *E, const int64_t *C, const int64_t *F,
                                                                     uint32_t B, uint32_t S, long long *out, double *sums) {
#pragma clang fp contract(off)
    for (uint32_t s = blockIdx.x * COLUMN_BLOCK + threadIdx.x; s < S; s += gridDim.x * COLUMN_BLOCK) {
        long long tw = 0, te = 0, tc = 0, tf = 0, count = 0;
        for (uint32_t b = 0; b < B; ++b) {
            const size_t at = (size_t)b * S + s;
            const long long ev = E[at];
            tw += W[at], te += ev, tc += C[at], tf += F[at];
            count += ev > 0 ? 1 : 0;
        }
        out[s] = tw, out[(size_t)S + s] = te, out[2 * (size_t)S + s] = tc, out[3 * (size_t)S + s] = tf;
        out[4 * (size_t)S + s] = te - tw, out[5 * (size_t)S + s] = count;
        ColumnStream<false> rates{W + s, E + s, (size_t)S, 0.0};
        const double rate_sum = np_add_reduce(rates, (uint64_t)count);
        const double mean = rate_sum / (double)count; // (a column without a positive row is refused before the launch)
        ColumnStream<true> deviations{W + s, E + s, (size_t)S, mean};
        sums[s] = rate_sum;
        sums[(size_t)S + s] = np_add_reduce(deviations, (uint64_t)count);
    }
}

// Order-preserving key of a finite double: a > b <=> key(a) > key(b); -0.0 and 0.0 share a key
__device__ inline unsigned long long order_key(double x) {
    const unsigned long long b = x == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ inline double key_value(unsigned long long key) {
    const unsigned long long b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
    return __longlong_as_double((long long)b);
}

// deltas / variances: [n][d] row-major.  stats: double [3][n] = delta_sum | variance_sum | minimum; worst: [n]; best_key: zero on entry
__global__ __launch_bounds__(64) void fk_perf_rows_kernel(const double *deltas, const double *variances, uint32_t n, uint32_t d, double *stats,
                                                          int32_t *worst, unsigned long long *best_key) {
#pragma clang fp contract(off)
    unsigned long long key = 0;
    for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < n; i += gridDim.x * 64u) {
        const double *row = deltas + (size_t)i * d;
        ArrayStream a{row}, v{variances + (size_t)i * d};
        stats[i] = np_add_reduce(a, d);
        stats[(size_t)n + i] = np_add_reduce(v, d);
        double minimum = row[0];
        int32_t at = 0;
        for (uint32_t j = 1; j < d; ++j)
            if (row[j] < minimum) minimum = row[j], at = (int32_t)j;
        stats[2 * (size_t)n + i] = minimum;
        worst[i] = at;
        const unsigned long long k = order_key(minimum);
        key = k > key ? k : key;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off);
        key = other > key ? other : key;
    }
    if (threadIdx.x == 0 && key) atomicMax(best_key, key);
}

// member: [n], 1 unless some row is >= in every coordinate and > in at least one
__global__ __launch_bounds__(PARETO_BLOCK) void fk_perf_pareto_kernel(const double *deltas, uint32_t n, uint32_t d, uint8_t *member) {
    __shared__ double tile[PT * MAX_D];
    const uint32_t n_blocks = (n + PARETO_BLOCK - 1u) / PARETO_BLOCK;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t i = blk * PARETO_BLOCK + threadIdx.x;
        double p[MAX_D];
#pragma unroll
        for (uint32_t j = 0; j < MAX_D; ++j) p[j] = (i < n && j < d) ? deltas[(size_t)i * d + j] : 0.0;
        bool dominated = i >= n; // lanes past the last row only help with the tiles
        for (uint32_t j0 = 0; j0 < n; j0 += PT) {
            const uint32_t nj = min(PT, n - j0);
            __syncthreads(); // (the tile of the trip before is read no more)
            for (uint32_t t = threadIdx.x; t < nj * d; t += PARETO_BLOCK) tile[t] = deltas[(size_t)j0 * d + t];
            __syncthreads();
            if (!dominated) {
                for (uint32_t r = 0; r < nj && !dominated; ++r) {
                    const double *q = tile + r * d;
                    bool all_ge = true, any_gt = false;
#pragma unroll
                    for (uint32_t j = 0; j < MAX_D; ++j)
                        if (j < d) {
                            const double qv = q[j];
                            all_ge = all_ge && qv >= p[j];
                            any_gt = any_gt || qv > p[j];
                        }
                    dominated = all_ge && any_gt;
                }
            }
            if (__all(dominated)) break; // the workgroup is this one wave: it leaves together
        }
        if (i < n) member[i] = dominated ? 0 : 1;
    }
}

// leader: n on entry; the smallest row with |minimum - best| <= 1e-15
__global__ __launch_bounds__(64) void fk_perf_leader_kernel(const double *minimum, uint32_t n, const unsigned long long *best_key, uint32_t *leader) {
#pragma clang fp contract(off)
    const double best = key_value(*best_key);
    uint32_t mine = 0xffffffffu;
    for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < n; i += gridDim.x * 64u)
        if (fabs(minimum[i] - best) <= MAXIMIN_ATOL) mine = min(mine, i);
    for (int off = 32; off > 0; off >>= 1) mine = min(mine, (uint32_t)__shfl_xor((int)mine, off));
    if (threadIdx.x == 0 && mine != 0xffffffffu) atomicMin(leader, mine);
}
#endif // __HIPCC__

} // namespace
} // namespace fkp
