// fk_rr_root_diagnostics.h — the per-root diagnostics and the cross-root agreement of the round-robin inference
// (fk_rr_root_diagnostics), included by farkle_hip.hip behind fk_rr_inference.h.  What _root_specific_diagnostics of the reference's
// analysis/h2h_inference.py (:918-1059) does, over root states that stay on the device (option "rr_keep_roots"):
//
//   fk_ri_pair_kernel<false>  (fk_rr_inference.h) the COMBINED accumulator's viability and incident sums; fk_ri_strategy_kernel turns
//                             the sums into the strategies' flags.  No interval.
//   fk_rd_test_kernel         per kept root, one lane per pair: the score test on the root's own two state rows when the combined pair
//                             is viable; p's bit pattern as Holm's sort key (1.0 without a test), d_ab kept
//   (Holm)                    fk_rr_inference.h's: stable radix sort, fk_ri_holm_scale_kernel, max scan, fk_ri_holm_scatter_kernel
//   fk_rd_decide_kernel       per kept root: flags, holm_reject, the diagnostic decision (:945-953); the decision counts leave with one
//                             atomic per wave and class (ballots); d_ab's decision byte stays for the agreement pass; lanes of the
//                             asked slice compute the ordinary interval and write their row
//   fk_rd_agree_kernel        one lane per pair: the row of :1003-1057 from the two kept effects and decisions; counts per wave, the
//                             largest absolute discrepancy by atomicMax on the bit pattern (a non-negative double), as
//                             fk_root_stability.h takes its maxima
//
// rd_decision and rd_agreement are plain __host__ __device__ C++: tests/native/rr_root_diagnostics_host_check.hip runs them without a
// GPU.  Floating-point contraction is off wherever there is float arithmetic, as in fk_rr_inference.h.
#pragma once

#include <cmath>
#include <cstdint>

namespace fkri {
namespace {

constexpr uint32_t RD_MAX_ROOTS = 2;   // FK_RR_MAX_ROOTS
constexpr uint32_t RD_COLS = 12;       // FK_RR_AGREE_COLS
constexpr uint32_t RD_ROOT_COLS = 4;   // per root: the three decisions, tests performed
enum : uint32_t { RD_PAIRS = 0, RD_AVAILABLE, RD_DECISION_AGREE, RD_DIRECTION_AGREE, RD_ROOT0 };
enum : uint32_t { RD_D_NONE = 0, RD_D_ADVANTAGE_A = 1, RD_D_ADVANTAGE_B = 2, RD_D_ABSENT = 255 }; // FK_RR_DIAGNOSTIC_*
enum : uint32_t { RD_A_AVAILABLE = 1, RD_A_DECISION = 2, RD_A_DIRECTION = 4 };                    // FK_RR_AGREE_*
static_assert(sizeof(fk_rr_root_row) == 168 && sizeof(fk_rr_agreement_row) == 56, "the rows are fixed-size records without implicit padding");
static_assert(RD_MAX_ROOTS == FK_RR_MAX_ROOTS && RD_COLS == FK_RR_AGREE_COLS && RD_COLS == RD_ROOT0 + RD_MAX_ROOTS * RD_ROOT_COLS, "farkle_hip.h");

// :945-953.  A NaN d_ab (no test) cannot come with a rejection; it would read as advantage b, as np.where reads it.
__host__ __device__ inline uint32_t rd_decision(bool holm_reject, double d_ab) {
    if (!holm_reject) return RD_D_NONE;
    return d_ab > 0.0 ? RD_D_ADVANTAGE_A : RD_D_ADVANTAGE_B;
}

// int(np.sign(x)) of an effect that exists: -0.0 and 0.0 have sign 0
__host__ __device__ inline int rd_sign(double x) { return x > 0.0 ? 1 : (x < 0.0 ? -1 : 0); }

struct Agreement {
    double discrepancy, absolute; // NaN unless available
    uint32_t flags;               // RD_A_*
};
// :1023-1055 for two roots: a = the smaller seed's effect, b = the larger's; NaN is the reference's None
__host__ __device__ inline Agreement rd_agreement(double a, uint32_t decision_a, double b, uint32_t decision_b) {
#pragma clang fp contract(off)
    Agreement r{NAN, NAN, 0u};
    if (a != a || b != b) return r; // (a NaN, written so that host and device compile the same test)
    r.discrepancy = a - b;
    r.absolute = fabs(r.discrepancy);
    r.flags = RD_A_AVAILABLE | (decision_a == decision_b ? RD_A_DECISION : 0u) | (rd_sign(a) == rd_sign(b) ? RD_A_DIRECTION : 0u);
    return r;
}

// what a pair's two state rows of ONE root say (fk_round_robin.h: attempted, completed, safety, wins_seat1, wins_seat2)
struct RootCounts {
    int64_t attempted, completed, safety, n_ab, n_ba, x_ab, x_ba;
};
__host__ __device__ inline RootCounts rd_root_counts(const uint32_t *ab /* [2][RR_STATE] */) {
    const uint32_t *ba = ab + fkrr::RR_STATE;
    RootCounts c;
    c.attempted = (int64_t)ab[0] + (int64_t)ba[0];
    c.completed = (int64_t)ab[1] + (int64_t)ba[1];
    c.safety = (int64_t)ab[2] + (int64_t)ba[2];
    c.n_ab = (int64_t)ab[1], c.n_ba = (int64_t)ba[1];
    c.x_ab = (int64_t)ab[3], c.x_ba = (int64_t)ba[3];
    return c;
}

// One lane per pair of one root.  A viable combined pair has every cell complete, so both of the root's blocks hold their target (> 0).
__global__ __launch_bounds__(256) void fk_rd_test_kernel(const uint32_t *__restrict__ state, const uint8_t *__restrict__ viable, uint32_t n_pairs,
                                                         unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals,
                                                         double *__restrict__ effect) {
#pragma clang fp contract(off)
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    double p_value = 1.0, d_ab = NAN; // a pair without a test enters Holm's family as 1.0 (:864-868)
    if (viable[p]) {
        const RootCounts c = rd_root_counts(state + (size_t)p * 2u * fkrr::RR_STATE);
        const Score sc = ri_score_test(c.x_ab, c.n_ab, c.x_ba, c.n_ba);
        p_value = sc.p, d_ab = 0.5 * sc.difference;
    }
    keys[p] = (unsigned long long)__double_as_longlong(p_value);
    vals[p] = p;
    effect[p] = d_ab;
}

// One lane per pair of one root: `counts` is the root's RD_ROOT_COLS of the summary.  ROWS = false is the call without a row slice: the
// interval inversion is not compiled in, and the streaming rest keeps its few registers and full occupancy.
template <bool ROWS>
__global__ __launch_bounds__(256) void fk_rd_decide_kernel(const uint32_t *__restrict__ state, const uint8_t *__restrict__ viable, uint32_t n,
                                                           uint64_t pair0, uint32_t n_pairs, double family_alpha, double critical_ordinary,
                                                           const uint8_t *__restrict__ strat_flags, const double *__restrict__ effect,
                                                           const double *__restrict__ adjusted, const uint32_t *__restrict__ position,
                                                           unsigned long long *__restrict__ counts, uint8_t *__restrict__ decision_out,
                                                           uint32_t row_first, uint32_t row_last, fk_rr_root_row *__restrict__ rows) {
#pragma clang fp contract(off)
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // whole waves
    const bool live = p < n_pairs;
    uint32_t decision = RD_D_ABSENT;
    bool tested = false;
    if (live) {
        uint32_t i, j;
        fkrr::rr_unrank(n, pair0 + p, i, j);
        tested = viable[p] != 0u;
        const bool operational = (strat_flags[i] & strat_flags[j] & RI_F_OPERATIONAL) != 0u;
        const bool eligible = tested && operational;
        const double adj = adjusted[p];
        const bool reject_before = tested && adj <= family_alpha;
        const bool reject = reject_before && eligible;
        decision = rd_decision(reject, effect[p]);
        decision_out[p] = (uint8_t)decision;
        if (ROWS && p >= row_first && p < row_last) {
            const RootCounts c = rd_root_counts(state + (size_t)p * 2u * fkrr::RR_STATE);
            fk_rr_root_row r;
            r.pair_id = pair0 + p;
            r.games_attempted = c.attempted, r.games_completed = c.completed, r.games_safety_limit = c.safety;
            r.n_ab = c.n_ab, r.n_ba = c.n_ba, r.seat1_a_wins_ab = c.x_ab, r.seat1_b_wins_ba = c.x_ba;
            r.holm_order = tested ? (int64_t)position[p] : 0;
            r.completion_game_rate = (double)c.completed / (double)c.attempted;
            Score sc{NAN, NAN, NAN, NAN};
            double low = NAN, high = NAN;
            r.q_ab = r.q_ba = NAN;
            if (tested) {
                sc = ri_score_test(c.x_ab, c.n_ab, c.x_ba, c.n_ba);
                ri_interval(c.x_ab, c.n_ab, c.x_ba, c.n_ba, critical_ordinary, low, high);
                r.q_ab = (double)c.x_ab / (double)c.n_ab;
                r.q_ba = (double)c.x_ba / (double)c.n_ba;
            }
            r.d_ab = 0.5 * sc.difference, r.score_null_proportion = sc.null_proportion, r.score_z = sc.z, r.score_p_value = sc.p;
            r.ordinary_d_low = 0.5 * low, r.ordinary_d_high = 0.5 * high;
            r.holm_adjusted_p = tested ? adj : NAN;
            r.strategy_a = i, r.strategy_b = j;
            r.flags = (uint8_t)((tested ? RI_F_INFERENTIAL : 0u) | (operational ? RI_F_OPERATIONAL : 0u) | (eligible ? RI_F_ELIGIBLE : 0u) |
                                (reject_before ? RI_F_REJECT_BEFORE : 0u) | (reject ? RI_F_REJECT : 0u));
            r.diagnostic_decision = (uint8_t)decision;
#pragma unroll
            for (uint32_t q = 0; q < 6u; ++q) r.pad[q] = 0u;
            rows[p - row_first] = r;
        }
    }
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) {
        const unsigned long long m = __ballot(decision == k);
        if (lane == 0u && m) atomicAdd(&counts[k], (unsigned long long)__popcll(m));
    }
    const unsigned long long m = __ballot(tested);
    if (lane == 0u && m) atomicAdd(&counts[3], (unsigned long long)__popcll(m));
}

// One lane per pair.  effect / decision: [n_roots][n_pairs], ascending seed.  `summary` is [RD_COLS] and then the maximum's bits.
__global__ __launch_bounds__(256) void fk_rd_agree_kernel(uint32_t n, uint64_t pair0, uint32_t n_pairs, uint32_t n_roots,
                                                          const double *__restrict__ effect, const uint8_t *__restrict__ decision,
                                                          unsigned long long *__restrict__ summary, uint32_t row_first, uint32_t row_last,
                                                          fk_rr_agreement_row *__restrict__ rows) {
#pragma clang fp contract(off)
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // whole waves
    const bool live = p < n_pairs;
    Agreement g{NAN, NAN, 0u};
    if (live) {
        const double a = effect[p], b = n_roots > 1u ? effect[(size_t)n_pairs + p] : NAN;
        const uint32_t da = decision[p], db = n_roots > 1u ? (uint32_t)decision[(size_t)n_pairs + p] : (uint32_t)RD_D_ABSENT;
        if (n_roots > 1u) g = rd_agreement(a, da, b, db);
        if (rows && p >= row_first && p < row_last) {
            uint32_t i, j;
            fkrr::rr_unrank(n, pair0 + p, i, j);
            fk_rr_agreement_row r;
            r.pair_id = pair0 + p;
            r.root_a_d_ab = a, r.root_b_d_ab = b;
            r.effect_discrepancy_a_minus_b = g.discrepancy, r.absolute_effect_discrepancy = g.absolute;
            r.strategy_a = i, r.strategy_b = j;
            r.root_a_decision = (uint8_t)da, r.root_b_decision = (uint8_t)db, r.flags = (uint8_t)g.flags;
#pragma unroll
            for (uint32_t q = 0; q < 5u; ++q) r.pad[q] = 0u;
            rows[p - row_first] = r;
        }
    }
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long alive = __ballot(live);
    if (lane == 0u && alive) atomicAdd(&summary[RD_PAIRS], (unsigned long long)__popcll(alive));
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) { // RD_A_AVAILABLE, RD_A_DECISION, RD_A_DIRECTION -> RD_AVAILABLE ..
        const unsigned long long m = __ballot((g.flags >> k) & 1u);
        if (lane == 0u && m) atomicAdd(&summary[RD_AVAILABLE + k], (unsigned long long)__popcll(m));
    }
    // the wave's largest absolute discrepancy, as ordered bits (+0.0 for a lane without one)
    unsigned long long bits = (g.flags & RD_A_AVAILABLE) ? (unsigned long long)__double_as_longlong(g.absolute) : 0ull;
#pragma unroll
    for (uint32_t d = 32u; d > 0u; d >>= 1) {
        const unsigned long long other = __shfl_xor(bits, d, 64);
        bits = other > bits ? other : bits;
    }
    if (lane == 0u && bits) atomicMax(&summary[RD_COLS], bits);
}

} // namespace
} // namespace fkri
