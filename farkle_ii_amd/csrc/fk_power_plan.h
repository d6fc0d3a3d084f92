// fk_power_plan.h — exact power of the round robin's two-sided score test on the device (fk_score_power_scan), included by
// farkle_hip.hip behind fk_agreement.h.  What the reference's analysis/h2h_schedule.py computes per (sample size, scenario) cell
// (implemented_score_test_power :324-358 over _fixed_first_count_boundary_arrays :273-295): with X1 ~ Bin(n, q_ab) and X2 ~ Bin(n, q_ba)
// independent,  power = sum over c1 of pmf_a(c1) * [ P(X2 <= lower(c1)) + P(X2 >= upper(c1)) ].
//
//   pp_boundaries           the two rejecting count boundaries of one first-sample count: the roots of the quadratic in count2, every
//                           multiply, add, divide and sqrt in the reference's order with FMA contraction OFF (one fused b * b - 4 a c
//                           moves a boundary by one where a root is an integer); plain __host__ __device__ C++, which
//                           tests/native/power_plan_host_check.hip walks without a GPU
//   pp_pmf                  exp(lf[n] - lf[k] - lf[n - k] + k log q + (n - k) log1p(-q)), lf = the context's log-factorial table
//   fk_pp_scan_kernel<LDS>  one workgroup per cell, PW_BLOCK threads.  The two tails of X2 — lo[k] = P(X2 <= k), hi[k] = P(X2 >= k),
//                           k = 0 .. n — by a chunked workgroup scan with a carried prefix: ascending chunks store pmf_b into hi and
//                           its running sum into lo, descending chunks turn hi into the suffix sum in place (a suffix sum, never
//                           1 - cdf: the rejection mass sits in tails of order 1e-9 and below).  Then c1 in strides of the
//                           workgroup: pmf_a(c1) times the two gathered tails; one workgroup sum, one store.
//                           LDS = true: the tails in static LDS, n + 1 <= PW_LDS_ENTRIES.  LDS = false: in the workgroup's slot of a
//                           global workspace, the workgroups striding over the cells.
//
// fp64 throughout, no atomics, plain vector stores.  A cell's result depends on the cell alone: not on its place in the batch.
#pragma once

#include <cstdint>

namespace fkpp {
namespace { // internal linkage, as fk_round_robin.h

constexpr uint32_t PW_BLOCK = 256;
constexpr uint32_t PW_WAVES = PW_BLOCK / 64u;
constexpr int32_t PW_MAX_N = FK_POWER_MAX_N;
constexpr uint32_t PW_LDS_ENTRIES = FK_POWER_LDS_MAX_N + 1; // 3072 entries x 2 tails x 8 bytes = 48 KiB of static LDS
static_assert(PW_LDS_ENTRIES * 16u <= 48u * 1024u, "three workgroups of the LDS kernel share a compute unit's 160 KiB");

// a cell as the kernel reads it: the caller's cell with the two logarithms of each probability taken once, on the host
struct Cell {
    int32_t n;
    uint32_t out; // the cell's place in the caller's batch
    double log_q_ab, log1m_q_ab, log_q_ba, log1m_q_ba;
};

// lower: the largest count2 <= the smaller root that rejects (-1: none); upper: the smallest count2 >= the larger root that rejects
// (n + 1: none).  `critical_squared` = pow(critical, 2) as the host's libm evaluates it.  The statements of _fixed_first_count_boundary_arrays, one element.
__host__ __device__ inline void pp_boundaries(int32_t n, double critical_squared, int32_t c1, int32_t &lower, int32_t &upper) {
#pragma clang fp contract(off)
    const double nobs = (double)n, count1 = (double)c1;
    const double quadratic = 2.0 * nobs + critical_squared;
    const double linear = (-4.0 * nobs) * count1 - (2.0 * critical_squared) * (nobs - count1);
    const double constant = (quadratic * count1) * count1 - ((2.0 * critical_squared) * nobs) * count1;
    double discriminant = linear * linear - (4.0 * quadratic) * constant;
    if (!(discriminant > 0.0)) discriminant = 0.0;
    const double root_distance = sqrt(discriminant);
    const double lower_root = (-linear - root_distance) / (2.0 * quadratic);
    const double upper_root = (-linear + root_distance) / (2.0 * quadratic);
    long long lo = (long long)ceil(lower_root) - 1, hi = (long long)floor(upper_root) + 1; // |roots| < 2^22: the casts are exact
    lo = lo < -1 ? -1 : (lo > n ? n : lo);
    hi = hi < 0 ? 0 : (hi > (long long)n + 1 ? (long long)n + 1 : hi);
    lower = c1 == 0 ? -1 : (int32_t)lo;
    upper = c1 == n ? n + 1 : (int32_t)hi;
}

// Unfused as well: the exponent reaches 1e5 and beyond, where one rounding more or less moves the mass by 1e-11 of itself; written
// this way it is the host statement's exponent bit for bit, and the device differs from it by its exp and the order of its sums alone.
__device__ inline double pp_pmf(const double *__restrict__ lf, int32_t n, int32_t k, double log_q, double log1m_q) {
#pragma clang fp contract(off)
    return exp(lf[n] - lf[k] - lf[n - k] + (double)k * log_q + (double)(n - k) * log1m_q);
}

__device__ inline double pp_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Inclusive sum over the workgroup in thread order (`reverse`: in descending thread order), every thread calls it.  `part` [PW_WAVES].
__device__ inline double pp_block_scan(double v, bool reverse, double *part) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t pos = reverse ? 63u - lane : lane; // the lane's place in the scan's direction
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const double other = __shfl(v, (int)(reverse ? lane + off : lane - off), 64); // (a lane outside the wave is not added)
        if (pos >= off) v += other;
    }
    __syncthreads(); // `part` of the chunk before has been read
    if (pos == 63u) part[wave] = v;
    __syncthreads();
    double before = 0.0;
#pragma unroll
    for (uint32_t w = 0; w < PW_WAVES; ++w)
        if (reverse ? w > wave : w < wave) before += part[w];
    return v + before;
}

// `cells` [count] in the order they are served, `power` indexed by Cell::out.  LDS: grid = count; otherwise grid <= count workgroups
// stride over the cells and `workspace` holds grid slots of 2 * slot_entries doubles, slot_entries > the largest n of `cells`.
template <bool LDS>
__global__ __launch_bounds__(PW_BLOCK) void fk_pp_scan_kernel(const Cell *__restrict__ cells, uint32_t count, const double *__restrict__ lf,
                                                             double critical_squared, double *__restrict__ workspace, uint64_t slot_entries,
                                                             double *__restrict__ power) {
    __shared__ double tails[LDS ? 2u * PW_LDS_ENTRIES : 2u];
    __shared__ double part[PW_WAVES];
    for (uint32_t at = blockIdx.x; at < count; at += gridDim.x) {
        const Cell cell = cells[at];
        const int32_t n = cell.n;
        const uint32_t entries = (uint32_t)n + 1u;
        double *const lo = LDS ? tails : workspace + (uint64_t)blockIdx.x * 2u * slot_entries;
        double *const hi = lo + (LDS ? (uint64_t)PW_LDS_ENTRIES : slot_entries);
        // 1. ascending chunks: hi[k] = pmf_b(k), lo[k] = P(X2 <= k)
        double carry = 0.0;
        for (uint32_t base = 0; base < entries; base += PW_BLOCK) {
            const uint32_t k = base + threadIdx.x;
            const double p = k < entries ? pp_pmf(lf, n, (int32_t)k, cell.log_q_ba, cell.log1m_q_ba) : 0.0;
            const double run = carry + pp_block_scan(p, false, part);
            if (k < entries) {
                hi[k] = p;
                lo[k] = run;
            }
            __syncthreads(); // the last thread's running sum, to every thread
            if (threadIdx.x == PW_BLOCK - 1u) part[0] = run;
            __syncthreads();
            carry = part[0];
        }
        // 2. descending chunks: hi[k] = P(X2 >= k), in place (a thread reads and writes its own element only)
        carry = 0.0;
        for (uint32_t base = (entries - 1u) / PW_BLOCK * PW_BLOCK;; base -= PW_BLOCK) {
            const uint32_t k = base + threadIdx.x;
            const double p = k < entries ? hi[k] : 0.0;
            const double run = carry + pp_block_scan(p, true, part);
            if (k < entries) hi[k] = run;
            __syncthreads();
            if (threadIdx.x == 0u) part[0] = run;
            __syncthreads();
            carry = part[0];
            if (base == 0u) break;
        }
        __syncthreads(); // the tails are complete (global memory: a workgroup's own stores are visible to it behind the barrier)
        // 3. the sum over the first sample's counts
        double acc = 0.0;
        for (uint32_t c1 = threadIdx.x; c1 < entries; c1 += PW_BLOCK) {
            int32_t lower, upper;
            pp_boundaries(n, critical_squared, (int32_t)c1, lower, upper); // lower in [-1, n], upper in [0, n + 1]
            const double reject = (lower >= 0 ? lo[lower] : 0.0) + (upper <= n ? hi[upper] : 0.0);
            acc += pp_pmf(lf, n, (int32_t)c1, cell.log_q_ab, cell.log1m_q_ab) * reject;
        }
        acc = pp_wave_sum(acc);
        __syncthreads(); // `part` of the last scan has been read
        if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0u) {
            double total = 0.0;
            for (uint32_t w = 0; w < PW_WAVES; ++w) total += part[w];
            power[cell.out] = total < 0.0 ? 0.0 : (total > 1.0 ? 1.0 : total);
        }
        __syncthreads(); // the next cell overwrites the tails and `part`
    }
}

} // namespace
} // namespace fkpp
