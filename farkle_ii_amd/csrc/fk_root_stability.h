// fk_root_stability.h — the two-root stability stage's bootstrap families on the device (included by farkle_hip.hip after
// fk_bootstrap.h, whose draws, integer product and counting rank it uses).
//
// Reference semantics (analysis/root_stability.py: _RootTopNRangeWriter.__call__ :816-906, _JointDiscrepancyRangeWriter.__call__
// :1201-1311).  Two roots (a, b), n_k player counts, 2 * n_k cells in (root, k) order.  Per replicate r and cell, stream = coordinate
// (ROOT_STABILITY_BOOTSTRAP = 401, root, k, replicate_index = r); B draws in [0, B) resample the cell's eligible batches (both
// families draw the same streams); rate = wins / exposures - 1 / k from the resampled integer totals.
//   top-N family   per root: score = 0.0; score += w_k * rate in the order of the player counts; the top_n first columns of
//                  lexsort((strategies, -score)) are members.
//   joint family   per k: |(rate_a - rate_b - observed[k]) / expected[k]| over the columns with expected[k] > 0; across:
//                  |(sum_k w_k * (rate_a - rate_b) - observed_across) / expected_across| where expected_across > 0; the replicate's
//                  value is the maximum of them all, 0.0 when there is none.
//
//   fk_boot_counts_kernel   (fk_bootstrap.h) the 2 * n_k streams of every replicate.
//   fk_root_rates_kernel    the hot path: one pass over the stacked matrices.  Strategy on the lane, RRB replicates per workgroup in
//                           registers, the cells walked as (a, k), (b, k) per player count so that rate_a is live while rate_b is
//                           accumulated; both roots' scores are written root-major [2][R][S] for the counting rank, the lane's running
//                           maximum is reduced over the workgroup and merged per replicate with ONE atomicMax on the value's bit
//                           pattern (non-negative doubles order as their patterns; a maximum does not depend on the order of its
//                           operands, so any grid gives the same bits; a replicate with no valid estimand keeps +0.0).
//   fk_boot_rank_kernel     (fk_bootstrap.h, unchanged) per root: top_n inclusion counts.
//   fk_root_member_kernel   the per-replicate uint8 membership [R][2][S] of the range file: the rank kernel's comparator on one
//                           (root, replicate) row per workgroup row.
//
// Float code must not be contracted into FMAs: `#pragma clang fp contract(off)` opens every kernel with float arithmetic.
#pragma once

namespace fkr {

using fkb::KDesc;
using fkb::TS;
using fkb::BT;
constexpr uint32_t RRB = 8; // replicates per workgroup of the rates kernel: 2 x RRB 64-bit accumulators + 5 x RRB doubles per lane

// grid = (ceil(S / TS), n_rep_padded / RRB), block = TS.  kd: 2 * n_k cells, (root, k) order; W / E: the stacked [sum_B][S] matrices;
// weights: [n_k]; scores: [2][n_rep][S].  JOINT: observed / expected are [n_k][S], observed_across / expected_across [S], maxima
// uint64 [n_rep_padded] zero on entry.  *bad is set when a resampled exposure total is <= 0 (the reference's ValueError).
template <bool JOINT>
__global__ __launch_bounds__(TS) void fk_root_rates_kernel(const int64_t *W, const int64_t *E, const uint32_t *counts, const KDesc *kd,
                                                           uint32_t n_k, uint32_t sum_B, uint32_t S, uint32_t n_rep, const double *weights,
                                                           const double *observed, const double *expected, const double *observed_across,
                                                           const double *expected_across, double *scores, unsigned long long *maxima,
                                                           int32_t *bad) {
#pragma clang fp contract(off)
    __shared__ uint4 cnt[BT][RRB / 4];
    __shared__ unsigned long long wg_max[RRB];
    const uint32_t s = blockIdx.x * TS + threadIdx.x;
    const uint32_t sr = min(s, S - 1u); // lanes past the last strategy repeat its column (a maximum does not mind) and write nothing
    const uint32_t rr0 = blockIdx.y * RRB;
    double score_a[RRB], score_b[RRB], across[RRB], peak[RRB], rate_a[RRB];
#pragma unroll
    for (uint32_t r = 0; r < RRB; ++r) score_a[r] = 0.0, score_b[r] = 0.0, across[r] = 0.0, peak[r] = 0.0;
    bool any_bad = false;
    for (uint32_t ki = 0; ki < n_k; ++ki) {
        const double wk = weights[ki];
#pragma unroll 1
        for (uint32_t root = 0; root < 2u; ++root) {
            const KDesc d = kd[root * n_k + ki];
            uint64_t w[RRB], e[RRB];
#pragma unroll
            for (uint32_t r = 0; r < RRB; ++r) w[r] = 0, e[r] = 0;
            fkb::cell_totals<RRB>(W, E, counts, d, sum_B, S, sr, rr0, cnt, w, e);
            double obs = 0.0, expd = 0.0;
            if (JOINT && root) obs = observed[(size_t)ki * S + sr], expd = expected[(size_t)ki * S + sr];
#pragma unroll
            for (uint32_t r = 0; r < RRB; ++r) {
                const long long tw = (long long)w[r], te = (long long)e[r];
                if (te <= 0 && rr0 + r < n_rep) any_bad = true;
                // wins / exposures - 1.0 / k: two roundings (:899, :1286)
                const double rate = (double)tw / (double)(te > 0 ? te : 1) - d.chance;
                const double term = wk * rate; // scores += weight * rate: the product is rounded, then the sum (:898)
                if (!root) {
                    rate_a[r] = rate;
                    score_a[r] = score_a[r] + term;
                } else {
                    score_b[r] = score_b[r] + term;
                    if (JOINT) {
                        const double difference = rate_a[r] - rate;
                        if (expd > 0.0) { // (NaN fails the test, as in numpy)
                            const double v = fabs((difference - obs) / expd); // :1291-1292
                            peak[r] = v > peak[r] ? v : peak[r];
                        }
                        const double part = wk * difference; // sum(...): 0 + t_1, + t_2, ... left to right (:1293-1296)
                        across[r] = across[r] + part;
                    }
                }
            }
        }
    }
    if (JOINT) {
        const double obs = observed_across[sr], expd = expected_across[sr];
        if (expd > 0.0) {
#pragma unroll
            for (uint32_t r = 0; r < RRB; ++r) {
                const double v = fabs((across[r] - obs) / expd); // :1300-1303
                peak[r] = v > peak[r] ? v : peak[r];
            }
        }
        if (threadIdx.x < RRB) wg_max[threadIdx.x] = 0ull;
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < RRB; ++r) {
            unsigned long long bits = (unsigned long long)__double_as_longlong(peak[r]);
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long other = __shfl_xor(bits, off);
                bits = other > bits ? other : bits;
            }
            if ((threadIdx.x & 63u) == 0u) atomicMax(&wg_max[r], bits);
        }
        __syncthreads();
        if (threadIdx.x < RRB && rr0 + threadIdx.x < n_rep) atomicMax(&maxima[rr0 + threadIdx.x], wg_max[threadIdx.x]);
    }
    if (s >= S) return;
    if (any_bad) *bad = 1;
#pragma unroll
    for (uint32_t r = 0; r < RRB; ++r)
        if (rr0 + r < n_rep) {
            scores[(size_t)(rr0 + r) * S + s] = score_a[r];
            scores[((size_t)n_rep + rr0 + r) * S + s] = score_b[r];
        }
}

// grid = (ceil(S / TS), 2 * n_rep), block = TS.  scores: [2][n_rep][S]; member: uint8 [n_rep][2][S] = rank <= top_n.
// The comparator is fk_boot_rank_kernel's (score_key, the tie rule folded into the comparand); the loop is stated here and not shared
// with that kernel through a device function: routed through one, the rank kernel's inner loop compiled with its counter on the VALU
// and ran 8.76 ms per 2 000 x 5 160 against 8.2 - 8.4 ms (profiles/performance_bootstrap_kernel_stats.txt).
__global__ __launch_bounds__(TS) void fk_root_member_kernel(const double *scores, uint32_t S, uint32_t n_rep, uint32_t top_n, uint8_t *member) {
    __shared__ unsigned long long keys[fkb::JT];
    const uint32_t s = blockIdx.x * TS + threadIdx.x;
    const uint32_t sr = min(s, S - 1u);
    const uint32_t root = blockIdx.y / n_rep, r = blockIdx.y - root * n_rep;
    const double *row = scores + (size_t)blockIdx.y * S;
    const uint64_t ki = fkb::score_key(row[sr]);
    uint32_t above = 0;
    for (uint32_t j0 = 0; j0 < S; j0 += fkb::JT) {
        const uint32_t nj = min(fkb::JT, S - j0);
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < nj; j += TS) keys[j] = fkb::score_key(row[j0 + j]);
        __syncthreads();
        const uint32_t split = s > j0 ? min(s - j0, nj) : 0u; // columns [0, split) of the tile come before s and win ties
        const uint64_t ki_before = ki - 1u;
        uint32_t j = 0;
        for (; j < split; ++j) above += keys[j] > ki_before ? 1u : 0u;
        for (; j < nj; ++j) above += keys[j] > ki ? 1u : 0u;
    }
    if (s < S) member[((size_t)r * 2u + root) * S + s] = above < top_n ? 1u : 0u;
}

} // namespace fkr
