// fk_layouts.h — host side: the composite device buffers of the engine, each as a plain struct that computes its offsets once
// from its shape.  The same struct serves the buffer's ensure, the kernel arguments and the copies home (farkle_hip.hip).
// Plain arithmetic, no HIP: tests/native/layouts_host_check.hip evaluates them on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

namespace fkl {

constexpr size_t GAME_COUNTS = 4; // = fkg::N_COUNTS (asserted where both are visible)

// fk_tournament_run_game_stats: u64 [S][4] counts | [S][rb] rounds | [S][mb] runner-up | [S][mb] spread | [4] game counts |
// [rb] game rounds | [mb] game runner-up | spill count, then the spill entries (int32 [cap][3]).  Offsets in u64 units.
struct GameStatsOut {
    size_t s_counts, s_rounds, s_runner, s_spread, g_counts, g_rounds, g_runner, spill_count, n_u64;
    GameStatsOut(size_t S, size_t rb, size_t mb)
        : s_counts(0), s_rounds(s_counts + S * GAME_COUNTS), s_runner(s_rounds + S * rb), s_spread(s_runner + S * mb), g_counts(s_spread + S * mb),
          g_rounds(g_counts + GAME_COUNTS), g_runner(g_rounds + rb), spill_count(g_runner + mb), n_u64(spill_count + 1) {}
    size_t spill_at() const { return n_u64 * 8; } // byte offset of the spill entries
    size_t bytes(int64_t spill_capacity) const { return spill_at() + (size_t)(spill_capacity > 1 ? spill_capacity : 1) * 12; }
};

// fk_tournament_run_rare_events: u64 [S][sb] second | [sb] game second | event total.  Offsets in u64 units.
struct RareOut {
    size_t s_second, g_second, total, n_u64;
    RareOut(size_t S, size_t sb) : s_second(0), g_second(S * sb), total(g_second + sb), n_u64(total + 1) {}
};

// The fingerprints a rows-mode call sends home with its tally: the game seeds, then (256-byte aligned) the shuffle seeds.
struct Fingerprints {
    size_t game_at, shuffle_at, bytes;
    Fingerprints(size_t game_seed_bytes, size_t shuffle_seed_bytes)
        : game_at(0), shuffle_at((game_seed_bytes + 255u) & ~(size_t)255u), bytes(shuffle_at + shuffle_seed_bytes) {}
};

// fk_root_stability_bootstrap's parameter block: weights [n_k] and, for the joint family, observed [n_k][S] | expected [n_k][S] |
// observed across k [S] | expected across k [S].  Offsets in doubles (the joint offsets are stated either way; only n says what exists).
struct RootParams {
    size_t weights, observed, expected, observed_across, expected_across, n;
    RootParams(size_t n_k, size_t S, bool joint)
        : weights(0), observed(n_k), expected(observed + n_k * S), observed_across(expected + n_k * S), expected_across(observed_across + S),
          n(n_k + (joint ? 2 * n_k * S + 2 * S : 0)) {}
};

// fk_root_window_estimates: the cells' [B][S] matrices stacked in cell order (one such buffer per matrix kind).  Offsets in int64 units.
struct RootWindowCells {
    size_t n_cells, S, n_i64;
    RootWindowCells(size_t n_cells, const int64_t *batch_counts, size_t S) : n_cells(n_cells), S(S), n_i64(0) {
        for (size_t i = 0; i < n_cells; ++i) n_i64 += (size_t)batch_counts[i] * S;
    }
    size_t cell_at(const int64_t *batch_counts, size_t cell) const {
        size_t at = 0;
        for (size_t i = 0; i < cell; ++i) at += (size_t)batch_counts[i] * S;
        return at;
    }
};

// fk_root_window_estimates' outputs, on the device and at the caller alike: totals int64 [n_windows][6][S] = wins | exposures | completed
// | safety | losses | positive batches, sums float64 [n_windows][3][S] = sum_w2 | sum_we | sum_e2.  Offsets in elements.
struct RootWindowOut {
    static constexpr size_t N_TOTALS = 6, N_SUMS = 3; // = fkw::N_TOTALS, fkw::N_SUMS (asserted where both are visible)
    size_t S, n_totals, n_sums;
    RootWindowOut(size_t n_windows, size_t S) : S(S), n_totals(n_windows * N_TOTALS * S), n_sums(n_windows * N_SUMS * S) {}
    size_t total_at(size_t window, size_t which) const { return (window * N_TOTALS + which) * S; }
    size_t sum_at(size_t window, size_t which) const { return (window * N_SUMS + which) * S; }
};

// fk_dominance_graph's bit matrices, rows of W = ceil(n / 64) words: adj [2][n][W] | adj_t [2][n][W] | reach [4][n][W] (the working
// copies that are closed) | panel [4][64][W] | dstar [4][64].  Offsets in u64 units; adj .. reach is one contiguous run.
struct DominanceMats {
    size_t W, plane, adj, adj_t, reach, panel, dstar, n_u64;
    explicit DominanceMats(size_t n)
        : W((n + 63) / 64), plane(n * W), adj(0), adj_t(2 * plane), reach(4 * plane), panel(8 * plane), dstar(panel + 4 * 64 * W), n_u64(dstar + 4 * 64) {}
};

// The keys of the extreme internal edges, [2][n] each: largest distance | smallest distance | strongest (rank, rank) | weakest.
struct DominanceKeys {
    size_t max_bits, min_bits, strong_key, weak_key, n_u64;
    explicit DominanceKeys(size_t n) : max_bits(0), min_bits(2 * n), strong_key(4 * n), weak_key(6 * n), n_u64(8 * n) {}
};

} // namespace fkl
