// fk_buffers.h — host side: what a context (farkle_hip.hip: fk_ctx) holds its device memory in.  Dev<T> is one allocation, typed and
// owning; the structs below group the buffers of the analysis entries, one struct per entry and one named member per role.  Included
// behind the kernels' headers, whose types the members name.  The layouts of the buffers that hold several parts are in fk_layouts.h.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>

using ull = unsigned long long;

inline std::atomic<int64_t> g_device_bytes_held{0}; // option "device_bytes_held": `cap` summed over the live buffers of every context of the process

// One device allocation of a context, typed and owning.  ensure() sizes it in elements; `cap` is what it holds in bytes.
template <class T>
struct Dev {
    T *p = nullptr;
    size_t cap = 0;
    Dev() = default;
    Dev(const Dev &) = delete;
    Dev &operator=(const Dev &) = delete;
    ~Dev() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        g_device_bytes_held -= (int64_t)cap;
        p = nullptr;
        cap = 0;
    }
    // a typed view into a byte buffer that holds more than one type, `byte_off` bytes in
    template <class U>
    U *as(size_t byte_off = 0) const {
        static_assert(sizeof(T) == 1, "views are taken of byte buffers only");
        return reinterpret_cast<U *>(p + byte_off);
    }
};

// ---- the device buffers of the analysis entries, one struct per entry, one member per role ----
struct MatchupReduceBufs { // fk_matchup_reduce
    Dev<ull> digest, key, key_alt, s_digest;                 // [n] the records' digests, both sort-key buffers, the sorted digests
    Dev<uint16_t> seats, rounds, s_seats, s_rounds;          // [n][K] / [n] as given and sorted
    Dev<uint32_t> idx, order, heads, run_id, tuple_break, run_mixed; // [n] sort payloads (both buffers), run / segment heads and their scan
    Dev<uint8_t> mixed_flag;                                 // [n] the element lies in a run that holds more than one tuple
    Dev<uint32_t> mixed_pos, mixed_key, mixed_key_alt, mixed_a, mixed_b, order_before; // the elements of mixed runs and their LSD sort
    Dev<uint32_t> seg_start;                                 // [G + 1]
    Dev<uint8_t> eligible;                                   // [G]
    Dev<ull> prio, prio_sorted;                              // [G]
    Dev<int32_t> bin;                                        // [G]
    Dev<uint32_t> hist, sel, sel_sorted;                     // [H], [G] x 2
    Dev<ull> out_digest;                                     // [M] the selected groups ...
    Dev<uint16_t> out_seats;                                 // [M][K]
    Dev<long long> out_count, out_sums;                      // [M], [M][n_lags][SUM_COLS]
    Dev<int32_t> lags;
    Dev<uint32_t> num;                                       // hipcub's selected-count word
};
struct SeatBufs { // fk_tournament_run_seat_counts
    Dev<long long> counts;
    Dev<uint16_t> id_rank;                  // [S]
    Dev<ull> key, key_sorted;               // the call's mirror records: keys ...
    Dev<uint32_t> val, val_sorted;          // ... and payloads, two sort buffers each
    Dev<ull> fr, e_fr, sh, e_sh;            // mirror_reduce: [n + 1] indicators and their exclusive sums
    Dev<uint32_t> ph, e_ph, seg_start, pair_start;
    Dev<int32_t> seg_diff;
    Dev<uint16_t> pair_rank;                // [capacity][2]
    Dev<long long> pair_sums;               // [capacity][PAIR_COLS]
    Dev<ull> pair_count;
};
struct TraceBufs { // fk_trace_games
    Dev<int2> strat;       // the strategies in points
    Dev<uint32_t> ws;      // seat workspace
    Dev<long long> counts, begin; // [n + 1] events per game and their exclusive scan
    Dev<uint8_t> rows;
    Dev<ull> err;
    Dev<uint4> events;
};
struct CensusBufs { // fk_census_games / fk_tournament_run_census
    Dev<int2> strat;  // the strategies in points
    Dev<uint32_t> ws; // seat workspace of one chunk
    Dev<ull> tables;  // the four tables + the error word (fkcn::CensusArgs::tables)
};
struct RoundRobinBufs { // fk_h2h_round_robin
    Dev<uint2> table;      // the n-row table, packed
    Dev<uint8_t> patience;
    Dev<uint32_t> state;   // window states
    Dev<ull> need, off;    // [rows + 1] games each block needs and their scan
    Dev<uint32_t> flag, aidx, act; // playing flags, their scan, the playing rows
    Dev<fkrr::RrError> err;
    Dev<uint32_t> bounds;  // [passes][2]
    Dev<ull> summary;
};
struct RrInferenceBufs { // fk_h2h_round_robin_resident, fk_rr_counts_add, fk_rr_inference, fk_rr_root_diagnostics
    Dev<ull> counts;               // the accumulator: [pairs][2][fkri::RI_COLS], resident between calls
    Dev<uint32_t> staged;          // one call's states [pairs][2][RR_STATE], added to `counts` when the call has succeeded
    Dev<ull> sums;                 // [n][fkri::RI_SUMS] per-strategy incident sums
    Dev<uint8_t> strat_flags;      // [n]
    Dev<ull> key, key_sorted;      // [pairs] the p-values' bit patterns, both sort buffers
    Dev<uint32_t> val, val_sorted; // [pairs] pair positions, both sort buffers
    Dev<double2> sim;              // [pairs] the simultaneous interval's halved bounds
    Dev<double> scaled, running, adjusted; // [pairs] (count - index) p and its running maximum in Holm's order; adjusted p in pair order
    Dev<uint32_t> position;        // [pairs] Holm's positions in pair order
    Dev<ull> class_counts;         // [fkri::RI_CLASSES]
    Dev<long long> strat_out;      // [n][fkri::RI_STRAT_COLS]
    Dev<fk_rr_pair_row> rows;      // the asked slice
    // option "rr_keep_roots" and fk_rr_root_diagnostics
    Dev<uint32_t> root_states[FK_RR_MAX_ROOTS]; // the root slots: one adding call's states each, [pairs][2][RR_STATE], in arrival order
    Dev<uint8_t> viable;           // [pairs] the combined pair's viability
    Dev<double> root_effect;       // [roots][pairs] d_ab per root, ascending seed (NaN without a test)
    Dev<uint8_t> root_decision;    // [roots][pairs] the diagnostic decisions
    Dev<ull> agree_summary;        // [fkri::RD_COLS] and the largest absolute discrepancy's bits
    Dev<fk_rr_root_row> root_rows; // [roots][the asked slice]
    Dev<fk_rr_agreement_row> agree_rows; // the asked slice
};
struct DominanceBufs { // fk_dominance_graph, fk_rr_dominance
    Dev<uint8_t> cls;             // [pairs] decision classes
    Dev<double2> sim;             // [pairs] the simultaneous bounds handed in (fk_rr_dominance reads RrInferenceBufs::sim)
    Dev<double> rate;             // [pairs] balanced_a_win_rate
    Dev<ull> mats;                // fkl::DominanceMats
    Dev<ull> keys;                // fkl::DominanceKeys
    Dev<uint32_t> comp, comp_deg; // [2][n] the component of a node; at a component's smallest row, the edges that enter it
    Dev<uint32_t> rank, unrank;   // [n] the tie-break order and its inverse
    Dev<fk_dom_node> nodes;       // [n]
    Dev<fk_dom_extreme> extremes; // [2][n]
};
struct AgreementBufs { // fk_agreement_pairs, fk_rr_agreement, fk_rank_concordance
    Dev<uint8_t> cls, codes; // [pairs] decision classes (fk_rr_agreement: written by the inference's chain); the pair codes
    Dev<int2> ranks;         // [n] (win_rate_rank, trueskill_rank) of every table row
    Dev<ull> counts;         // [fkag::AG_COUNTS]
    Dev<int32_t> x, y;       // [m] the keys of fk_rank_concordance
    Dev<ull> concordance;    // [fkag::CC_COUNTS]
};
struct PowerPlanBufs { // fk_score_power_scan
    Dev<double> lf;         // log-factorial table: lf[k] = log k! (long-double lgamma, rounded), k = 0 .. lf_n - 1; filled once, grown with the largest n seen
    size_t lf_n = 0;        // entries of `lf` that are filled
    Dev<fkpp::Cell> cells;  // the call's cells, largest n first
    Dev<double> power;      // [n_cells] in the caller's order
    Dev<double> workspace;  // the tails of the cells beyond LDS: one slot of 2 (n_max + 1) doubles per workgroup
};
struct BootBufs { // fk_performance_bootstrap, fk_root_stability_bootstrap
    Dev<int64_t> wins, exposures; // the stacked matrices
    Dev<fkb::KDesc> kd;
    Dev<uint32_t> counts;  // one block's multiplicity rows
    Dev<double> scores;    // one block's score rows (one per root)
    Dev<int32_t> bad;      // flag: a replicate without complete-support exposure
    Dev<ull> counters;     // performance: the rank kernel's four counters
    Dev<double> contrast;  // performance: [2][n_controls][S] contrast sums and squares
    Dev<int32_t> controls;
    Dev<double> params;    // root stability: fkl::RootParams
    Dev<ull> maxima, root_counters; // root stability: one block's maxima (as ordered bits); four counters per root
    Dev<uint8_t> member;   // root stability: one block's membership rows
};
struct PerformanceBufs { // fk_performance_by_k, fk_performance_across_k
    Dev<int64_t> wins, exposures, completed, safety; // by k: the four [B][S] matrices
    Dev<long long> totals;   // by k: [6][S] wins | exposures | completed | safety | losses | positive batches
    Dev<double> sums;        // by k: [2][S] rate_sum | ssd
    Dev<double> deltas, variances; // across k: [n][d]
    Dev<double> stats;       // across k: [3][n] delta_sum | variance_sum | minimum
    Dev<int32_t> worst;      // across k: [n]
    Dev<uint8_t> member;     // across k: [n]
    Dev<ull> best;           // across k: the largest minimum's ordered key; behind it the leader row
};
struct RootWindowBufs { // fk_root_window_estimates
    Dev<int64_t> wins, exposures, completed, safety; // the cells' [B][S] matrices, stacked in cell order (fkl::RootWindowCells)
    Dev<fkw::Cell> cells;       // [n_cells]
    Dev<fkw::Group> groups;     // the windows grouped by (cell, row_begin)
    Dev<fkw::Snap> snaps;       // [n_windows] in group order, ascending row_end within a group
    Dev<fkw::PairTask> pairs;   // the windows with pairwise columns
    Dev<long long> totals;      // fkl::RootWindowOut: [n_windows][6][S]
    Dev<double> sums;           // fkl::RootWindowOut: [n_windows][3][S]
};
struct ProbeBufs { // the fk_debug_* probes and fk_coordinate_seeds: the kernel's buffer arguments in their order, bytes
    Dev<uint8_t> a, b, c, d, e;
};
