// fk_rr_inference.h — round-robin inference on the device (fk_h2h_round_robin_resident, fk_rr_counts_add, fk_rr_inference), included
// by farkle_hip.hip behind fk_round_robin.h.  What the reference's analysis/h2h_inference.py does with H2H counts, per pair of a
// resident pair range:
//
//   ri_score_test            two_proportion_score_test (h2h_inference.py:68-99) in its statement order; p = erfc(|z| / sqrt 2)
//   ri_stat_at               _score_statistic_at_difference (:142-188): the closed-form cubic of the constrained null
//   ri_bound / ri_interval   _score_interval_bound (:191-231) and _score_difference_interval_fallback (:234-277): the same dyadic
//                            bracket outward from the estimate, then bisection until the bracket is at most 2^-44 wide
//                            (the reference finishes with brentq at xtol 1e-12; the library route, confint_proportions_2indep,
//                            is not reproduced)
//   fk_ri_add_kernel         one root's block states -> the 64-bit accumulator per (pair, order) (_combine_within_order, :563-635)
//   fk_ri_pair_kernel        per pair: viability (_viability_status, :638-700), the per-strategy incident sums (a segmented wave
//                            scan, as fk_rr_summary_kernel), the score test's p as Holm's sort key, the simultaneous interval
//                            (<false>: viability and sums alone, for fk_rr_root_diagnostics.h)
//   fk_ri_strategy_kernel    per strategy: completion rate, the two viability flags
//   fk_ri_holm_scale_kernel  (count - index) * p over the sorted p (_holm_adjust, :280-295); hipcub sorts before and scans (max) after
//   fk_ri_holm_scatter_kernel min(1, .) and the positions back to pair order
//   fk_ri_decide_kernel      the decision chain (:886-909), class and per-strategy class counts, and the rows of the asked slice
//
// The three ri_* statistics are plain __host__ __device__ C++: tests/native/rr_inference_host_check.hip checks them without a GPU.
// Floating-point contraction is off in every function with float arithmetic, the way fk_seat_ratio_kernel keeps it off: each
// operation of the reference is rounded once here too.
#pragma once

#include <cmath>
#include <cstdint>

namespace fkri {
namespace { // internal linkage, as fk_round_robin.h

constexpr uint32_t RI_COLS = 9; // the accumulator's columns per (pair, order)
enum : uint32_t { RI_ATTEMPTED = 0, RI_COMPLETED, RI_SAFETY, RI_WINS1, RI_WINS2, RI_REQUIRED, RI_MAX_ATTEMPTS, RI_CELLS, RI_CELLS_COMPLETE };
constexpr uint32_t RI_CLASSES = 7;     // FK_RR_CLASSES
constexpr uint32_t RI_STRAT_COLS = 12; // FK_RR_STRATEGY_COLS: seven class counts, attempted, completed, safety, two flags
constexpr uint32_t RI_SUMS = 4;        // per-strategy incident sums: attempted, completed, safety, nonviable pairs
enum : uint32_t { RI_F_INFERENTIAL = 1, RI_F_OPERATIONAL = 2, RI_F_ELIGIBLE = 4, RI_F_REJECT_BEFORE = 8, RI_F_REJECT = 16 };
enum : uint32_t { RI_C_PRACTICAL_A = 0, RI_C_PRACTICAL_B, RI_C_STATISTICAL_A, RI_C_STATISTICAL_B, RI_C_EQUIVALENT, RI_C_UNRESOLVED, RI_C_NONVIABLE };

struct Score {
    double difference, null_proportion, z, p;
};

// h2h_inference.py:80-93
__host__ __device__ inline Score ri_score_test(int64_t count1, int64_t nobs1, int64_t count2, int64_t nobs2) {
#pragma clang fp contract(off)
    Score r;
    const double rate1 = (double)count1 / (double)nobs1;
    const double rate2 = (double)count2 / (double)nobs2;
    r.difference = rate1 - rate2;
    r.null_proportion = (double)(count1 + count2) / (double)(nobs1 + nobs2);
    const double variance = r.null_proportion * (1.0 - r.null_proportion) * (1.0 / (double)nobs1 + 1.0 / (double)nobs2);
    if (variance > 0.0) {
        r.z = r.difference / sqrt(variance);
        r.p = erfc(fabs(r.z) * 0.70710678118654752440); // the argument cephes forms for 2 norm.sf(|z|)
    } else if (r.difference == 0.0) {
        r.z = 0.0;
        r.p = 1.0;
    } else {
        r.z = copysign(INFINITY, r.difference);
        r.p = 0.0;
    }
    return r;
}

// h2h_inference.py:151-188
__host__ __device__ inline double ri_stat_at(int64_t count1, int64_t nobs1, int64_t count2, int64_t nobs2, double difference) {
#pragma clang fp contract(off)
    const double observed = (double)count1 / (double)nobs1 - (double)count2 / (double)nobs2;
    double null_prop1, null_prop2;
    if (difference <= -1.0) {
        null_prop1 = 0.0, null_prop2 = 1.0;
    } else if (difference >= 1.0) {
        null_prop1 = 1.0, null_prop2 = 0.0;
    } else if (difference == 0.0) {
        null_prop1 = null_prop2 = (double)(count1 + count2) / (double)(nobs1 + nobs2);
    } else {
        const int64_t total_n = nobs1 + nobs2, total_count = count1 + count2;
        const double three_n = (double)(3 * total_n);
        const double cubic_2 = (double)(nobs1 + 2 * nobs2) * difference - (double)total_n - (double)total_count;
        const double cubic_1 = ((double)count2 * difference - (double)total_n - (double)(2 * count2)) * difference + (double)total_count;
        const double cubic_0 = (double)count2 * difference * (1.0 - difference);
        const double shift = cubic_2 / three_n;
        const double q_value = shift * shift * shift - cubic_1 * cubic_2 / (double)(6 * total_n * total_n) + cubic_0 / (double)(2 * total_n);
        const double radicand = shift * shift - cubic_1 / three_n;
        const double cubic_p = q_value != 0.0 ? copysign(sqrt(radicand > 0.0 ? radicand : 0.0), q_value) : 0.0;
        if (cubic_p == 0.0) {
            null_prop2 = -cubic_2 / three_n;
        } else {
            double cosine_argument = q_value / (cubic_p * cubic_p * cubic_p);
            cosine_argument = cosine_argument < 1.0 ? cosine_argument : 1.0;
            cosine_argument = cosine_argument > -1.0 ? cosine_argument : -1.0;
            const double angle = (3.141592653589793 + acos(cosine_argument)) / 3.0;
            null_prop2 = 2.0 * cubic_p * cos(angle) - shift;
        }
        null_prop1 = null_prop2 + difference;
        null_prop1 = null_prop1 < 1.0 ? null_prop1 : 1.0;
        null_prop1 = null_prop1 > 0.0 ? null_prop1 : 0.0;
        null_prop2 = null_prop2 < 1.0 ? null_prop2 : 1.0;
        null_prop2 = null_prop2 > 0.0 ? null_prop2 : 0.0;
    }
    const double variance = null_prop1 * (1.0 - null_prop1) / (double)nobs1 + null_prop2 * (1.0 - null_prop2) / (double)nobs2;
    const double numerator = observed - difference;
    if (variance > 0.0) return numerator / sqrt(variance);
    if (numerator == 0.0) return 0.0;
    return copysign(INFINITY, numerator);
}

// the objective of :206-212: an infinite statistic counts as a rejection
__host__ __device__ inline double ri_objective(int64_t count1, int64_t nobs1, int64_t count2, int64_t nobs2, double difference, double critical_value) {
#pragma clang fp contract(off)
    const double statistic = ri_stat_at(count1, nobs1, count2, nobs2, difference);
    if (fabs(statistic) == INFINITY) return 1.0;
    return fabs(statistic) - critical_value;
}

// :203-231.  The bracket is the reference's: the first observed + span 2^-e, e = 52 .. 0, whose objective is >= 0, against the
// candidate before it.  Inside, bisection keeps one end accepted and one rejected until they are at most 2^-44 apart.
__host__ __device__ inline double ri_bound(int64_t count1, int64_t nobs1, int64_t count2, int64_t nobs2, double observed, double endpoint,
                                           double critical_value) {
#pragma clang fp contract(off)
    if (observed == endpoint) return endpoint;
    double previous = observed, scale = 0x1p-52;
    const double span = endpoint - observed;
    for (int exponent = 52; exponent >= 0; --exponent, scale = scale * 2.0) {
        const double candidate = observed + span * scale;
        if (candidate == previous) continue;
        if (ri_objective(count1, nobs1, count2, nobs2, candidate, critical_value) >= 0.0) {
            double accepted = previous, rejected = candidate;
            while (fabs(rejected - accepted) > 0x1p-44) {
                const double mid = 0.5 * (accepted + rejected);
                if (mid == accepted || mid == rejected) break;
                if (ri_objective(count1, nobs1, count2, nobs2, mid, critical_value) >= 0.0) rejected = mid;
                else accepted = mid;
            }
            return 0.5 * (accepted + rejected);
        }
        previous = candidate;
    }
    return NAN; // (the endpoint itself rejects with an infinite statistic: not reached)
}

// :244-277, the swap for a positive estimate unrolled
__host__ __device__ inline void ri_interval(int64_t count1, int64_t nobs1, int64_t count2, int64_t nobs2, double critical_value, double &low_out,
                                            double &high_out) {
#pragma clang fp contract(off)
    double observed = (double)count1 / (double)nobs1 - (double)count2 / (double)nobs2;
    const bool swapped = observed > 0.0;
    if (swapped) {
        int64_t t = count1;
        count1 = count2, count2 = t;
        t = nobs1;
        nobs1 = nobs2, nobs2 = t;
        observed = (double)count1 / (double)nobs1 - (double)count2 / (double)nobs2;
    }
    double low = ri_bound(count1, nobs1, count2, nobs2, observed, -1.0, critical_value);
    double high = ri_bound(count1, nobs1, count2, nobs2, observed, 1.0, critical_value);
    if (count1 == count2 && nobs1 == nobs2) {
        const double symmetric = fabs(low) > fabs(high) ? fabs(low) : fabs(high);
        low = -symmetric, high = symmetric;
    }
    low_out = swapped ? -high : low;
    high_out = swapped ? -low : high;
}

// what a pair's two accumulator rows say: order 0 seats A = table[i] in seat 1, order 1 seats B = table[j] there
struct PairCounts {
    int64_t attempted, completed, safety, required, n_ab, n_ba, x_ab, x_ba, a_wins_ba;
    bool viable;
};
__host__ __device__ inline PairCounts ri_pair_counts(const unsigned long long *ab /* [2][RI_COLS] */) {
    const unsigned long long *ba = ab + RI_COLS;
    PairCounts c;
    c.attempted = (int64_t)(ab[RI_ATTEMPTED] + ba[RI_ATTEMPTED]);
    c.completed = (int64_t)(ab[RI_COMPLETED] + ba[RI_COMPLETED]);
    c.safety = (int64_t)(ab[RI_SAFETY] + ba[RI_SAFETY]);
    c.required = (int64_t)(ab[RI_REQUIRED] + ba[RI_REQUIRED]);
    c.n_ab = (int64_t)ab[RI_COMPLETED];
    c.n_ba = (int64_t)ba[RI_COMPLETED];
    c.x_ab = (int64_t)ab[RI_WINS1];
    c.x_ba = (int64_t)ba[RI_WINS1];
    c.a_wins_ba = (int64_t)ba[RI_WINS2];
    c.viable = ab[RI_CELLS] != 0u && ab[RI_CELLS_COMPLETE] == ab[RI_CELLS] && ab[RI_COMPLETED] == ab[RI_REQUIRED] &&
               ba[RI_CELLS] != 0u && ba[RI_CELLS_COMPLETE] == ba[RI_CELLS] && ba[RI_COMPLETED] == ba[RI_REQUIRED] && c.n_ab == c.n_ba;
    return c;
}

// one lane per (pair, order) row of a root's states [rows][RR_STATE]
__global__ void fk_ri_add_kernel(const uint32_t *__restrict__ state, uint64_t n_rows, uint32_t target, uint32_t max_attempts,
                                 unsigned long long *__restrict__ acc) {
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const uint32_t *s = state + row * fkrr::RR_STATE;
    unsigned long long *a = acc + row * RI_COLS;
#pragma unroll
    for (uint32_t c = 0; c < fkrr::RR_STATE; ++c) a[c] += s[c];
    a[RI_REQUIRED] += target;
    a[RI_MAX_ATTEMPTS] += max_attempts;
    a[RI_CELLS] += 1u;
    a[RI_CELLS_COMPLETE] += s[1] == target ? 1u : 0u;
}

// One lane per pair.  The i side of the incident sums leaves through the segmented wave scan of fk_rr_summary_kernel (pair ids ascend
// with the lane, so the lanes of a wave that share row i are adjacent), the j side with one atomic per lane and column.
// TESTED = false is the viability pass of fk_rr_root_diagnostics: the sums and the pair's `viable` byte, no test and no interval.
template <bool TESTED>
__global__ __launch_bounds__(256) void fk_ri_pair_kernel(const unsigned long long *__restrict__ acc, uint32_t n, uint64_t pair0, uint32_t n_pairs,
                                                         double critical_simultaneous, unsigned long long *__restrict__ sums /* [n][RI_SUMS] */,
                                                         unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals,
                                                         double2 *__restrict__ sim, uint8_t *__restrict__ viable /* [n_pairs], TESTED = false only */) {
#pragma clang fp contract(off)
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // blockDim is a multiple of 64: whole waves
    const bool live = p < n_pairs;
    uint32_t i = 0xffffffffu, j = 0xffffffffu;
    unsigned long long v[RI_SUMS] = {0ull, 0ull, 0ull, 0ull};
    if (live) {
        fkrr::rr_unrank(n, pair0 + p, i, j);
        const PairCounts c = ri_pair_counts(acc + (size_t)p * 2u * RI_COLS);
        v[0] = (unsigned long long)c.attempted, v[1] = (unsigned long long)c.completed, v[2] = (unsigned long long)c.safety;
        v[3] = c.viable ? 0ull : 1ull;
        if constexpr (TESTED) {
            double p_value = 1.0, low = NAN, high = NAN; // a pair without a test enters Holm's family as 1.0 (:864-868)
            if (c.viable) {
                p_value = ri_score_test(c.x_ab, c.n_ab, c.x_ba, c.n_ba).p;
                ri_interval(c.x_ab, c.n_ab, c.x_ba, c.n_ba, critical_simultaneous, low, high);
                low = 0.5 * low, high = 0.5 * high; // :853-854
            }
            keys[p] = (unsigned long long)__double_as_longlong(p_value); // non-negative doubles order as their bit patterns
            vals[p] = p;
            sim[p] = make_double2(low, high);
        } else {
            viable[p] = c.viable ? 1u : 0u;
        }
    }
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long up_acc[RI_SUMS];
#pragma unroll
    for (uint32_t c = 0; c < RI_SUMS; ++c) up_acc[c] = v[c];
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t i_up = __shfl_up(i, d, 64);
        const bool take = lane >= d && i_up == i;
#pragma unroll
        for (uint32_t c = 0; c < RI_SUMS; ++c) {
            const unsigned long long up = __shfl_up(up_acc[c], d, 64);
            if (take) up_acc[c] += up;
        }
    }
    const uint32_t i_next = __shfl_down(i, 1u, 64);
    if (live && (lane == 63u || i_next != i)) {
#pragma unroll
        for (uint32_t c = 0; c < RI_SUMS; ++c)
            if (up_acc[c]) atomicAdd(&sums[(size_t)i * RI_SUMS + c], up_acc[c]);
    }
    if (live) {
#pragma unroll
        for (uint32_t c = 0; c < RI_SUMS; ++c)
            if (v[c]) atomicAdd(&sums[(size_t)j * RI_SUMS + c], v[c]);
    }
}

// :669-699: operational viability is completed / attempted >= threshold (one IEEE division), inferential "all incident pairs viable"
__global__ void fk_ri_strategy_kernel(const unsigned long long *__restrict__ sums, uint32_t n, double threshold, uint8_t *__restrict__ flags,
                                      long long *__restrict__ out /* [n][RI_STRAT_COLS], zeroed */) {
#pragma clang fp contract(off)
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const unsigned long long attempted = sums[(size_t)s * RI_SUMS], completed = sums[(size_t)s * RI_SUMS + 1u];
    const bool operational = attempted != 0ull && (double)completed / (double)attempted >= threshold;
    const bool inferential = sums[(size_t)s * RI_SUMS + 3u] == 0ull;
    flags[s] = (uint8_t)((inferential ? RI_F_INFERENTIAL : 0u) | (operational ? RI_F_OPERATIONAL : 0u));
    long long *o = out + (size_t)s * RI_STRAT_COLS;
    o[RI_CLASSES] = (long long)attempted;
    o[RI_CLASSES + 1u] = (long long)completed;
    o[RI_CLASSES + 2u] = (long long)sums[(size_t)s * RI_SUMS + 2u];
    o[RI_CLASSES + 3u] = operational ? 1 : 0;
    o[RI_CLASSES + 4u] = inferential ? 1 : 0;
}

// :287: (count - index) * p, one double multiply
__global__ void fk_ri_holm_scale_kernel(const unsigned long long *__restrict__ sorted_keys, uint32_t count, double *__restrict__ scaled) {
#pragma clang fp contract(off)
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < count) scaled[k] = (double)(count - k) * __longlong_as_double((long long)sorted_keys[k]);
}

// :291-294, after the running maximum
__global__ void fk_ri_holm_scatter_kernel(const double *__restrict__ running, const uint32_t *__restrict__ sorted_vals, uint32_t count,
                                          double *__restrict__ adjusted, uint32_t *__restrict__ position) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const double a = running[k];
    adjusted[sorted_vals[k]] = a < 1.0 ? a : 1.0;
    position[sorted_vals[k]] = k + 1u;
}

struct DecideParams {
    double family_alpha, practical_delta, delta_equivalence /* NaN = off */, critical_ordinary;
};

// One lane per pair: flags, Holm's decisions, the class chain of :886-909; the class counts leave with one atomic per wave and class,
// the i side of the per-strategy counts with one per segment and class (ballots), the j side with one per lane.  Lanes of the asked
// slice write their row: the score test and the ordinary interval are computed again there, the simultaneous one is the stored one.
__global__ __launch_bounds__(256) void fk_ri_decide_kernel(const unsigned long long *__restrict__ acc, uint32_t n, uint64_t pair0, uint32_t n_pairs,
                                                           DecideParams par, const uint8_t *__restrict__ strat_flags,
                                                           const double2 *__restrict__ sim, const double *__restrict__ adjusted,
                                                           const uint32_t *__restrict__ position, unsigned long long *__restrict__ class_counts,
                                                           long long *__restrict__ strat_out, uint32_t row_first, uint32_t row_last,
                                                           fk_rr_pair_row *__restrict__ rows, uint8_t *__restrict__ cls_out /* nullable: [n_pairs] */) {
#pragma clang fp contract(off)
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // whole waves
    const bool live = p < n_pairs;
    uint32_t i = 0xffffffffu, j = 0xffffffffu, cls = 0xffffffffu;
    if (live) {
        fkrr::rr_unrank(n, pair0 + p, i, j);
        const PairCounts c = ri_pair_counts(acc + (size_t)p * 2u * RI_COLS);
        const bool operational = (strat_flags[i] & strat_flags[j] & RI_F_OPERATIONAL) != 0u;
        const bool eligible = c.viable && operational; // :754-756
        const double adj = adjusted[p];
        const bool reject_before = c.viable && adj <= par.family_alpha;
        const bool reject = reject_before && eligible;
        const double2 s = sim[p];
        Score sc{NAN, NAN, NAN, NAN};
        if (c.viable) sc = ri_score_test(c.x_ab, c.n_ab, c.x_ba, c.n_ba);
        const double effect = 0.5 * sc.difference;
        if (!eligible) cls = RI_C_NONVIABLE;
        else if (s.x > par.practical_delta) cls = RI_C_PRACTICAL_A;
        else if (s.y < -par.practical_delta) cls = RI_C_PRACTICAL_B;
        else if (reject) cls = effect > 0.0 ? RI_C_STATISTICAL_A : RI_C_STATISTICAL_B;
        else if (!isnan(par.delta_equivalence) && s.x > -par.delta_equivalence && s.y < par.delta_equivalence) cls = RI_C_EQUIVALENT;
        else cls = RI_C_UNRESOLVED;
        if (cls_out) cls_out[p] = (uint8_t)cls; // (fk_rr_dominance: the graph kernels read the classes on the device)
        if (rows && p >= row_first && p < row_last) {
            fk_rr_pair_row r;
            r.pair_id = pair0 + p;
            r.games_attempted = c.attempted, r.games_completed = c.completed, r.games_safety_limit = c.safety, r.n_completed_required = c.required;
            r.n_ab = c.n_ab, r.n_ba = c.n_ba, r.seat1_a_wins_ab = c.x_ab, r.seat1_b_wins_ba = c.x_ba, r.seat2_a_wins_ba = c.a_wins_ba;
            r.balanced_a_wins = c.x_ab + c.a_wins_ba;
            r.holm_order = c.viable ? (int64_t)position[p] : 0;
            r.completion_game_rate = (double)c.completed / (double)c.attempted;
            double low = NAN, high = NAN;
            r.q_ab = r.q_ba = r.balanced_a_win_rate = NAN;
            if (c.viable) {
                ri_interval(c.x_ab, c.n_ab, c.x_ba, c.n_ba, par.critical_ordinary, low, high);
                r.q_ab = (double)c.x_ab / (double)c.n_ab;
                r.q_ba = (double)c.x_ba / (double)c.n_ba;
                r.balanced_a_win_rate = (double)r.balanced_a_wins / (double)(c.n_ab + c.n_ba);
            }
            r.raw_order_rate_difference = sc.difference, r.d_ab = effect, r.score_null_proportion = sc.null_proportion;
            r.score_z = sc.z, r.score_p_value = sc.p;
            r.ordinary_d_low = 0.5 * low, r.ordinary_d_high = 0.5 * high;
            r.simultaneous_d_low = s.x, r.simultaneous_d_high = s.y;
            r.holm_adjusted_p = c.viable ? adj : NAN;
            r.strategy_a = i, r.strategy_b = j;
            r.flags = (uint8_t)((c.viable ? RI_F_INFERENTIAL : 0u) | (operational ? RI_F_OPERATIONAL : 0u) | (eligible ? RI_F_ELIGIBLE : 0u) |
                                (reject_before ? RI_F_REJECT_BEFORE : 0u) | (reject ? RI_F_REJECT : 0u));
            r.decision_class = (uint8_t)cls;
#pragma unroll
            for (uint32_t q = 0; q < 6u; ++q) r.pad[q] = 0u;
            rows[p - row_first] = r;
        }
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i_prev = __shfl_up(i, 1u, 64);
    const bool head = live && (lane == 0u || i_prev != i);
    const unsigned long long heads = __ballot(head), above = lane == 63u ? 0ull : heads >> (lane + 1u);
    const uint32_t seg_end = above ? lane + (uint32_t)__ffsll((long long)above) : 64u; // the next head's lane
    const unsigned long long seg = (seg_end == 64u ? ~0ull : ((1ull << seg_end) - 1ull)) & ~((1ull << lane) - 1ull);
#pragma unroll
    for (uint32_t k = 0; k < RI_CLASSES; ++k) {
        const unsigned long long m = __ballot(live && cls == k);
        if (lane == 0u && m) atomicAdd(&class_counts[k], (unsigned long long)__popcll(m));
        if (head && (m & seg)) atomicAdd((unsigned long long *)&strat_out[(size_t)i * RI_STRAT_COLS + k], (unsigned long long)__popcll(m & seg));
    }
    if (live) atomicAdd((unsigned long long *)&strat_out[(size_t)j * RI_STRAT_COLS + (cls < 4u ? (cls ^ 1u) : cls)], 1ull); // B's side of the pair
}

} // namespace
} // namespace fkri
