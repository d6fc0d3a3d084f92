/*
 * farkle_hip.h — C-ABI of the MI355X (gfx950) Farkle simulation engine.
 *
 * The reference (Isaac-McPadden/Farkle_II) is pure Python and has no FFI; its seams for
 * the simulation hot path are in-process callables.  Each entry point below replaces one
 * of those seams (citations are path:line under the reference's root):
 *
 *   fk_tournament_run  <-  _play_one_shuffle / _run_chunk / _run_chunk_metrics
 *                          src/farkle/simulation/run_tournament.py:301-393, 403-457, 473-585
 *   fk_play_games      <-  _play_game over an explicit coordinate list
 *                          src/farkle/simulation/simulation.py:576-655 (callers: simulate_many_games
 *                          :658-722, _measure_throughput run_tournament.py:593-619)
 *   fk_h2h_run         <-  _simulate_block_from_manifest attempt loop (the BlockRunner contract)
 *                          src/farkle/analysis/h2h_schedule.py:1149-1243, 1521
 *   fk_coordinate_seeds <- coordinate_seed (src/farkle/utils/random.py:190-232)
 *   fk_debug_*         <-  FarklePlayer._roll (src/farkle/game/engine.py:85-101) and
 *                          default_score / decide (src/farkle/game/scoring.py:618-693,
 *                          src/farkle/simulation/strategies.py:212-275): single-op probes of the
 *                          SAME device functions the game kernel uses, for parity tests.
 *
 * Conventions: plain C types, caller-allocated caller-owned HOST buffers, no callbacks.
 * Every function returns FK_OK (0) or a negative error code; fk_last_error() gives the
 * message (for FK_ERR_ROLL_LIMIT it names the offending game, mirroring the RuntimeError of
 * engine.py:242-243).  One context per process/GPU; calls on a context are serialised by the
 * caller.  There is NO CPU fallback: fk_init fails if no HIP device is usable.
 */
#ifndef FARKLE_HIP_H
#define FARKLE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    FK_OK = 0,
    FK_ERR_ROLL_LIMIT = -1,       /* a turn exceeded 1000 rolls (engine.py:36,242) */
    FK_ERR_ARG = -2,              /* invalid argument */
    FK_ERR_COUNTER_OVERFLOW = -3, /* a per-seat u16 counter left its guarded range: the game kernels stop a game whose seat holds more
                                   * than 64 000 rolls or more than 63 000 returned dice of either kind (n_smart_five_dice,
                                   * n_smart_one_dice), or whose turn is worth more than 65 500 points; fk_trace_games and the census
                                   * entries refuse a game with a row counter beyond 65 535.  The message names one offending game (its
                                   * index in the call, or in the launch for head-to-head attempts; trace and census: the smallest).
                                   * After this error the contents of the call's output buffers are
                                   * unspecified; buffers a call ADDS to (the resident tally accumulator, the summary of
                                   * fk_h2h_round_robin) are untouched, and the context serves the next call as if the failed one had
                                   * not been made (a hint given for it is spent). */
    FK_ERR_HIP = -4,              /* HIP runtime failure */
    FK_ERR_NO_DEVICE = -5,
    FK_ERR_COMM = -6,             /* RCCL not loadable / communicator failure */
    FK_ERR_IO = -7                /* a row shard could not be written (fk_write_row_shards) */
};

enum { FK_COMPLETED = 0, FK_SAFETY_LIMIT = 1 };

/* ThresholdStrategy (src/farkle/simulation/strategies.py:165-194), 20 bytes */
typedef struct {
    int32_t score_threshold;
    int32_t dice_threshold;
    uint8_t smart_five, smart_one, consider_score, consider_dice;
    uint8_t require_both, auto_hot_dice, run_up_score, favor_score; /* favor_score=1: FavorDiceOrScore.SCORE */
    int32_t strategy_id; /* carried, not interpreted */
} fk_strategy;

/* Per-seat part of a game row (PlayerStats, src/farkle/game/engine.py:360-406), 28 bytes */
typedef struct {
    int32_t score;
    int32_t strategy; /* INDEX into the strategy table of the call */
    uint16_t farkles, rolls, n_turns, highest_turn;
    uint16_t smart_five_uses, n_smart_five_dice, smart_one_uses, n_smart_one_dice, hot_dice;
    uint8_t rank;           /* 1-based; 0 = null (safety limit) */
    uint8_t hit_max_rounds; /* 0/1 */
} fk_seat;

/* Row = fk_row_hdr followed by k fk_seat records: 4 + 28*k bytes (simulation.py:628-655) */
typedef struct {
    uint16_t n_rounds;
    uint8_t status;     /* FK_COMPLETED / FK_SAFETY_LIMIT */
    int8_t winner_seat; /* 0-based; -1 = none */
} fk_row_hdr;

/* max_rounds override (src/farkle/simulation/game_profile.py:24-69).
 * Tournament: a=shuffle_index, b=game_index, k_or_order=k.  H2H: a=pair_id, b=attempt_index, k_or_order=order. */
typedef struct {
    uint64_t root_seed;
    uint64_t a, b;
    uint32_t k_or_order;
    uint32_t max_rounds;
} fk_override;

/* Seat-stream coordinate of one game (src/farkle/utils/random.py:80-124); seat_index is implied */
typedef struct {
    uint32_t purpose;
    uint32_t pad;
    uint64_t root_seed, k, shuffle_index, pair_id, order, game_index, seat_index, replicate_index;
} fk_coord;

/* The most seats a game may have, for every entry that plays games with a caller-chosen seat count (fk_tournament_run* and
 * fk_play_games): a row names its winner in an int8 (fk_row_hdr.winner_seat) and a rank in a uint8, and the device's result word
 * carries the winner's seat in seven bits.  More seats return FK_ERR_ARG before any device work. */
#define FK_MAX_PLAYERS 128
#define FK_SEAT_STAT_COLS 31 /* all-seat integer statistics per strategy, see fk_tournament_run_stats */
#define FK_LAG_COLS 11 /* lag sufficient statistics per (strategy, lag), see fk_tournament_run_lags */
#define FK_MAX_LAGS 16
#define FK_TALLY_COLS 26 /* wins, attempted, completed, safety, 11 metric sums, 11 square sums (run_tournament.py:109-121) */

typedef struct {
    char name[64];
    char arch[32];
    int32_t compute_units;
    int32_t clock_mhz;
    int32_t wavefront_size;
    int32_t lds_bytes_per_cu;
    uint64_t hbm_bytes;
} fk_device_info;

/* Timing of the last fk_tournament_run / fk_play_games / fk_h2h_run on this context, from HIP events
 * recorded on the context's stream. */
typedef struct {
    float perm_ms;    /* shuffle-permutation kernel(s) of the chunks prepared in front of their game kernel */
    float seed_ms;    /* SeedSequence -> PCG64DXSM seeding kernel(s) of the same chunks */
    float play_ms;    /* game kernel(s) */
    float total_ms;   /* first launch -> last kernel done (device time incl. memsets) */
    int32_t play_launches;
    int32_t play_block, play_grid, play_lds_bytes;
    int64_t games;
    int32_t prefetched_chunks; /* chunks whose permutations / seeding ran on the side stream behind an earlier game kernel:
                                  not in perm_ms / seed_ms */
    int32_t play_clock_mhz;    /* option "clock_stamps": shader clock of the call's last game kernel, measured inside it (median over
                                  its workgroups of d(s_memtime) / d(s_memrealtime) x 100 MHz); 0 = not measured */
    float play_block_end_p50_ms, play_block_end_max_ms; /* same option, same kernel: when the median and the last of its workgroups
                                  finished, from the first workgroup's start (100 MHz counter) — max - p50 is the launch's tail, the
                                  stretch in which the chip drains behind the longest games */
    int32_t play_mixed_flags;  /* the strategy-flag form of the last game kernel instance: 0 (every flag shared by the whole table: scalar),
                                  0xc000 (only require_both / favor_score differ) or 0xff00 (any flag may differ) */
    /* Hand-over counts of the call's fk_play_kernel launches, summed over their waves.  Only a measuring build of the library
     * (-DFK_COUNT_HANDOVER, never the product) fills them; 0 otherwise.  A trip is one pass of a wave through the roll loop. */
    int64_t ho_handovers, ho_lanes_served, ho_trips, ho_waiting_lane_trips, ho_rolling_lane_trips, ho_waves;
} fk_timing;

typedef struct fk_ctx fk_ctx;

int fk_init(int device_ordinal, fk_ctx **out);
void fk_destroy(fk_ctx *ctx);
const char *fk_last_error(fk_ctx *ctx);
int fk_get_device_info(fk_ctx *ctx, fk_device_info *out);
int fk_get_timing(fk_ctx *ctx, fk_timing *out);
/* The game-kernel instance of the last launch of the last fk_tournament_run* / fk_play_games / fk_h2h_run* call on this context — after
 * a replay (out-of-memory, counter guard) the replay's — as the compiler spells its template, e.g.
 * "fk_play_hc_kernel<768, 65280u, true, 12, 3, false, false, 12>"; "" when that call launched none.  Valid until the next call. */
const char *fk_last_play_instance(fk_ctx *ctx);
/* Page-locked host memory for the caller-owned output buffers (rows above all: 60 bytes per k=2 game).  A buffer from here is
 * copied to by one DMA per chunk at PCIe rate, while the next chunk plays; any other host pointer works too (staged by the HIP
 * runtime, about a third of the rate, the host thread waits).  Free with fk_host_free before fk_destroy.  The pages are anonymous
 * memory populated by the kernel and then registered with the HIP runtime (256 MB: ~15 + ~2 ms, and only the registration takes the
 * runtime's lock — hipHostMalloc, the fallback, holds it for ~45 ms); may be called from any thread. */
int fk_host_alloc(fk_ctx *ctx, size_t bytes, void **out);
int fk_host_free(fk_ctx *ctx, void *p);
/* Tunables: "chunk_bytes" (device workspace budget per chunk), "batch_threshold" (lanes that must be waiting
 * before a wave runs its game hand-over; 0, the default = auto: 8 up to eight seats, 12 at nine / ten, 16 at eleven / twelve), "use_lds_tally" (0/1/-1 auto), "block" (0 auto), "lean" (seat-record layout:
 * -1 auto, 0 full, 1 lean), "state_store" (-1 auto: seat records live in the HBM state store, with only the turn owner's staged in LDS, when
 * k of them do not fit LDS (k > 64); 0 the same; 1 always), "blocks_per_cu", "max_waves" (resident waves per SIMD the launch plan counts
 * on, default 6), "longest_first" (1 = deal
 * never-banking pairings first), "flat_handover" (1, default: two-seat tournament and game-list launches end and start games on the flat
 * path of fk_play_kernel; 0: on the general one, as a chunk too large for 32-bit record offsets does), "uniform_flags" (-1 auto: tables whose strategies share all flag bits run the scalar-flag
 * kernel instance, 0 never), "perm_split" (-1 auto), "columns_by_seat" (-1 auto: the column images of fk_tournament_run_columns by one thread per (game, seat) up to sixteen seats, per game beyond; 0 / 1 force), "perm_draw_wave" (-1 auto: a shuffle's Fisher-Yates draws by a whole wave in chunks of up to 32 768 shuffles, by one thread beyond; 0 / 1 force), "pipeline" (1, default: the next chunk / hinted call is prepared around the
 * current game kernel — permutations in front of it, schedule and seat seeding on a low-priority stream in its drain tail;
 * 0: every chunk is prepared on the main stream in front of its own game kernel), "hot_cold" (tournament launches of 4..12 seats on
 * the hot / cold game kernel, csrc/fk_play_hc.h: -1 auto, 0 never — the LDS-record kernel plays them), "comm_timeout_ms" (deadline of
 * fk_comm_init and of each collective, default 120 000 or the environment's FK_COMM_TIMEOUT_MS — a non-negative integer, consulted only
 * while this option has never been set; 0 = no deadline.  After a timed-out fk_comm_init the context keeps playing, a peer that joins
 * late meets a helper that aborts the orphan communicator itself, and the process should end when its work is done: a helper thread may
 * still sit inside librccl), "rows_chunk_games" (rows mode plays in chunks of about this many games,
 * default 4 000 000: chunk i's rows cross PCIe while chunk i + 1 plays), "resident_tally" (see fk_tally_resident_reduce), "clock_stamps" (1: every workgroup of a game kernel reads the
 * shader-clock and the 100 MHz reference counters at its first and last instruction; fk_timing.play_clock_mhz).  All of them
 * are scheduling / layout choices: results are identical for every setting. */
int fk_set_option(fk_ctx *ctx, const char *name, int64_t value);
/* Read back an option or a figure of the last call: "chunk_bytes", "workspace_percent" (a buffer set's workspace is at most this share of
 * the device memory the context can have — free now + its own per-chunk buffers — halved for the two sets; default 80), "last_budget" (the
 * bytes per buffer set the last tournament / H2H call planned with), "device_bytes_held" (the device memory, in bytes, that the buffers of
 * every live context of this PROCESS hold right now: it grows where a buffer grows and falls where one is freed, so a destroyed context
 * leaves it where it was before the context was created; memory held by fk_debug_hold_memory is not counted), "oom_replays" (how often that call met hipErrorOutOfMemory, gave
 * its workspace back and was replayed with half the budget: results are identical), "comm_timeout_ms" (the EFFECTIVE deadline: the option
 * if it was ever set, else a well-formed FK_COMM_TIMEOUT_MS, else 120 000), "rows_chunk_games". */
int fk_get_option(fk_ctx *ctx, const char *name, int64_t *value);

/* Tournament shuffles [shuffle_begin, shuffle_end) of the S-strategy table at k players.
 *   tally       int64 [n_batches][S][26], n_batches = ceil(n_shuffles / shuffles_per_batch); overwritten.
 *   rows        nullable; n_shuffles * (S/k) rows of 4+28k bytes, game-major in (shuffle, game) order.
 *   perms       nullable; int32 [n_shuffles][S] (the permutation of each shuffle; tests/diagnostics).
 * Requires 1 <= k <= FK_MAX_PLAYERS, S % k == 0 (run_tournament.py:274), S <= 65535, max_rounds <= 65535.  Targets above 3 200 000 points play with
 * full LDS records (lean ones carry the banked total / 50 in 16 bits): FK_ERR_ARG if k of those do not fit LDS, and for the
 * batched head-to-head entry points. */
int fk_tournament_run(fk_ctx *ctx, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                      uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch,
                      int32_t target_score, int32_t max_rounds, const fk_override *ov, int32_t n_ov,
                      int64_t *tally, void *rows, int32_t *perms);

/* ---- row shards without a host-side conversion -------------------------------------------------------------------------------
 * The reference persists rows as ONE PARQUET FILE PER SHUFFLE (`rows_<root>_<k>p_<shuffle:012d>.parquet`, run_tournament.py:530-558,
 * schema raw_simulation_schema_for(k), utils/schema_helpers.py:23-90).  fk_tournament_run_columns is fk_tournament_run with the rows
 * delivered as per-shuffle COLUMN IMAGES: every column of that schema that depends on the games, already in its Parquet physical type
 * (strategy ids resolved on the device through `strategy_ids`, ranks / margins / loss margins computed there).  Image of one shuffle,
 * fk_row_columns_bytes(k, gps) bytes (a multiple of 64), gps = S / k:
 *     int32 planes [4 + 13 k][gps]   winner_strategy, winning_score, victory_margin, n_rounds, then for seat 1..k: score, farkles, rolls,
 *                                    highest_turn, strategy, rank, loss_margin, smart_five_uses, n_smart_five_dice, smart_one_uses,
 *                                    n_smart_one_dice, hot_dice, n_turns                                   (the schema's column order)
 *     uint8 status[gps]              1 = safety limit: the row's nullable fields are null and every hit flag is set (engine.py:485-489)
 *     uint8 winner_seat[gps]         0-based; uint8 rank_order[gps][k]: seats in rank order (the seat_ranks list)
 *   columns     n_shuffles images, shuffle-major; k <= 64 (narrower than FK_MAX_PLAYERS).     strategy_ids   int32 [S]: the strategy_id of table row i. */
int fk_tournament_run_columns(fk_ctx *ctx, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                              uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch,
                              int32_t target_score, int32_t max_rounds, const fk_override *ov, int32_t n_ov,
                              int64_t *tally, const int32_t *strategy_ids, void *columns);
/* fk_tournament_run_columns that also delivers what a row shard carries besides the images: shuffle_seeds[n_shuffles] = the ns-100
 * fingerprint of each shuffle (the shards' manifest records, run_tournament.py:97-105) and game_seeds[n_shuffles][S / k] = the ns-102
 * fingerprint of each game (the game_seed column, run_tournament.py:340-350), as fk_game_seeds computes them; either may be null.
 * Complete on return (not subject to "rows_async"). */
int fk_tournament_run_columns_seeds(fk_ctx *ctx, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                                    uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score,
                                    int32_t max_rounds, const fk_override *overrides, int32_t n_overrides, int64_t *tally,
                                    const int32_t *strategy_ids, void *columns, uint32_t *shuffle_seeds, uint32_t *game_seeds);
size_t fk_row_columns_bytes(int32_t k, int32_t games_per_shuffle);
/* Option "rows_async" = 1: a call that delivers rows (AoS or column images) returns when its last device-to-host copy is QUEUED; the
 * buffer may be read after fk_rows_wait(ctx, slot) with slot = fk_get_option("rows_event") read right after that call (a ring of 4:
 * at most four calls' images may be outstanding).
 * The next call's game kernel then runs beside the copy (a caller with two destination buffers: `farkle run`, rows mode). */
int fk_rows_wait(fk_ctx *ctx, int32_t slot);

/* Column images -> the row-shard files, on `threads` host threads (no ctx: plain host code).  Each file is a complete Parquet file
 * (one row group, uncompressed PLAIN / RLE_DICTIONARY pages, no statistics) whose Arrow schema — restored by a reader from the
 * ARROW:schema entry — and rows equal what the reference writes for the same games.  The FileMetaData parts that only depend on the
 * schema come from the footer of a file Arrow wrote for raw_simulation_schema_for(k) (farkle_ii_amd/parquet_template.py): `footer_head`
 * = its fields 1-2 (version, schema), `footer_kv` = field 5 (key-value metadata), `footer_orders` = field 7 (column orders), as raw Thrift
 * spans; `leaf_type[i]` / `leaf_paths` (components '\0'-separated, each path '\0'-terminated) = physical type and path_in_schema of leaf i.
 * Outputs per shuffle: the file's size and SHA-256 (the manifest record's byte_length / data_sha256) and — with a contract-v3 sidecar
 * template (contract_v3.SimulationContract.shard_template: the text around size, digest and name) — the written sidecar's SHA-256.
 * `atomic`: write `<name>.tmp` and rename.  Returns FK_OK, FK_ERR_ARG or FK_ERR_IO with a message in `error`. */
typedef struct {
    int32_t k, games_per_shuffle, n_shuffles, threads, atomic, rng_purpose_namespace;
    uint64_t root_seed;
    const int64_t *shuffle_index;   /* [n_shuffles] */
    const int64_t *shuffle_seed;    /* [n_shuffles] namespace-100 fingerprints */
    const int32_t *batch_id;        /* [n_shuffles] deterministic_batch_id */
    const uint32_t *game_seed;      /* [n_shuffles][gps] namespace-102 fingerprints (fk_game_seeds) */
    const void *columns;            /* [n_shuffles] images, `shard_stride` bytes apart */
    size_t shard_stride;
    const char *directory;
    const uint8_t *footer_head; size_t footer_head_len;
    const uint8_t *footer_kv; size_t footer_kv_len;
    const uint8_t *footer_orders; size_t footer_orders_len;
    const int32_t *leaf_type;       /* [n_leaves], n_leaves = 18 + 14 k */
    const char *leaf_paths;
    int32_t n_leaves;
    const char *const *side_body;   /* nullable: 4 pieces */
    const char *const *side_full;   /* nullable: 5 pieces */
    const char *side_directory;     /* results-root-relative directory of the shards, with a trailing '/' */
} fk_shard_job;
int fk_write_row_shards(const fk_shard_job *job, int64_t *byte_length, uint8_t *sha256, uint8_t *sidecar_sha256, char *error, size_t error_len);
/* SHA-256 as the shard writer computes it (SHA-NI when the CPU has it; portable = 1 forces the scalar rounds; portable = 2: the two-message
 * lockstep form — digests of data[0 .. n/2) and data[n/2 .. n) into out32[0 .. 32) and out32[32 .. 64)): parity probe. */
int fk_debug_sha256(const void *data, size_t n, uint8_t *out32, int32_t portable);

/* fk_tournament_run (k <= FK_MAX_PLAYERS) plus the integer sufficient statistics of ALL seats (not winners only), per batch and strategy:
 *   seat_stats  nullable; int64 [n_batches][S][FK_SEAT_STAT_COLS]; overwritten.  Columns:
 *     0 exposures, 1 completed exposures, 2 safety-limit exposures (= max-round aborts), 3 wins,
 *     4/5 sum / sum of squares of the final score, 6/7 of n_turns, 8 exposures with n_turns != n_rounds,
 *     9/10 sum / sum of squares of (n_turns - n_rounds), then (sum, sum of squares) pairs of: rank, loss_margin (both over
 *     completed exposures only), rolls, farkles, highest_turn, hot_dice, smart_five_uses, n_smart_five_dice,
 *     smart_one_uses, n_smart_one_dice.
 * These are the integer accumulators of the reference's unconditional all-player batch metrics
 * (src/farkle/analysis/all_player_metrics.py:257-340), produced on the device from the state store without
 * materialising rows; its two ratio statistics (score / n_turns, score / n_rounds) are float64 sums in row order:
 * fk_tournament_run_all_player below. */
int fk_tournament_run_stats(fk_ctx *ctx, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                            uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch,
                            int32_t target_score, int32_t max_rounds, const fk_override *ov, int32_t n_ov,
                            int64_t *tally, void *rows, int32_t *perms, int64_t *seat_stats);

/* fk_tournament_run_stats (k <= FK_MAX_PLAYERS) plus the four float64 accumulators of the same table (all_player_metrics.py:308-321), per batch and strategy:
 *   seat_ratio_sums  double [n_batches][S][FK_SEAT_RATIO_COLS]; overwritten.  Columns: sum of score / n_turns over the strategy's
 *     exposures (0 where n_turns is 0), sum of its squares, sum of score / n_rounds, sum of its squares.
 * The reference adds them with np.add.at in source-row order (:174-177), i.e. one sequential float64 sum per strategy over its
 * exposures in (shuffle, game, seat) order.  A strategy sits once per shuffle: the device runs exactly that sequence — one thread
 * per (batch, strategy), ascending shuffles, one rounding per division, multiplication and addition — so the sums carry the bits the
 * reference's do whenever its curated rows are in (shuffle, game) order (pinned by tests/golden/all_player_vectors.json, the reference's
 * own _iter_batch_tables).  seat_stats is required (the digests both read are built once). */
#define FK_SEAT_RATIO_COLS 4
int fk_tournament_run_all_player(fk_ctx *ctx, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                                 uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch,
                                 int32_t target_score, int32_t max_rounds, const fk_override *ov, int32_t n_ov,
                                 int64_t *tally, void *rows, int32_t *perms, int64_t *seat_stats, double *seat_ratio_sums);

/* Scheduling hint: the next fk_tournament_run / fk_tournament_run_stats call on this context — the one AFTER the call that
 * follows this hint — will play shuffles [shuffle_begin, shuffle_end) of the same table, k and root seed (need_state != 0: it
 * will ask for rows or seat_stats).  The call that follows the hint prepares that range around its own game kernel
 * (permutations in front of it, schedule and seat seeding on a low-priority stream in its drain tail; option "pipeline" = 0
 * ignores hints).  Results never depend on hints; a hint that turns out wrong only wastes the preparation.  (The reference's process pool keeps `window = 4 * n_jobs` chunks in flight
 * for the same reason, run_tournament.py:1576-1586.) */
int fk_tournament_hint_next(fk_ctx *ctx, uint64_t shuffle_begin, uint64_t shuffle_end, int32_t need_state);

/* fk_tournament_run + the lag sufficient statistics of the reference's RNG diagnostics for the STRATEGY family
 * (analysis/rng_diagnostics.py: observation records :1870-1905, _OnlineMetric :2031-2076, stats rows :2110-2160).  A strategy is
 * seated exactly once per shuffle, so its observation series — win indicator and n_rounds of the game it sat in, ordered by
 * (root_seed, shuffle_index) — is indexed by the shuffle; for every lag the pairs (earlier x, later y) = (series[t - lag], series[t]).
 *   lags        n_lags (1 .. FK_MAX_LAGS) strictly increasing positive shuffle distances (analysis.rng_diagnostic_lags)
 *   lag_sums    int64 [S][n_lags][FK_LAG_COLS], overwritten: 0 pair_count; win indicator: 1 sum x, 2 sum y, 3 sum x^2, 4 sum y^2,
 *               5 sum xy; n_rounds: 6 sum x, 7 sum y, 8 sum x^2, 9 sum y^2, 10 sum xy — over the pairs whose BOTH shuffles lie in
 *               [shuffle_begin, shuffle_end).  Exact integers (the reference accumulates the same integers in float64).
 *   edge_head / edge_tail   uint16 [m][S], m = min(max lag, n_shuffles): the series values (n_rounds | won << 15) of the first / last m
 *               shuffles of the range, strategy-minor.  Two ranges that follow each other (launch groups, ranks: contiguous whole
 *               batches per rank) combine on the host: sums add, plus the pairs that straddle the cut, which need exactly the
 *               tail of the earlier and the head of the later range (farkle_ii_amd/rng_lags.py: LagSummary.merge).
 * The matchup family of the same module is fk_tournament_run_matchups + fk_matchup_reduce below.
 * Requires max_rounds (and every override) <= 32767 and k <= FK_MAX_PLAYERS. */
int fk_tournament_run_lags(fk_ctx *ctx, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                           uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score,
                           int32_t max_rounds, const fk_override *ov, int32_t n_ov, int64_t *tally, const int32_t *lags, int32_t n_lags,
                           int64_t *lag_sums, uint16_t *edge_head, uint16_t *edge_tail);

/* fk_tournament_run_lags (same outputs) + one record per game for the MATCHUP family of the RNG diagnostics
 * (analysis/rng_diagnostics.py: group key _extract_batch_arrays :1092-1150, digest _matchup_ids :1173-1185).  Records are in
 * coordinate order (shuffle-major, game within shuffle), game g of the range at index g:
 *   m_digest   uint64 [n_games]: blake2b(int32 LE [k, sorted seat strategy IDs, -1 padding to max_players], digest_size=8,
 *              person=b"farkle-m"), read little-endian
 *   m_seats    uint16 [n_games][k]: the seats' TABLE indices, ordered by ascending strategy_ids[index]
 *   m_rounds   uint16 [n_games]: n_rounds (15 bits; safety-limit games included)
 *   strategy_ids  int32 [S], unique: the IDs the digest and the order use; 1 <= k <= 16 (narrower than FK_MAX_PLAYERS),
 *              k <= max_players <= 31. */
int fk_tournament_run_matchups(fk_ctx *ctx, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                               uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score,
                               int32_t max_rounds, const fk_override *ov, int32_t n_ov, int64_t *tally, const int32_t *lags, int32_t n_lags,
                               int64_t *lag_sums, uint16_t *edge_head, uint16_t *edge_tail, const int32_t *strategy_ids, int32_t max_players,
                               uint64_t *m_digest, uint16_t *m_seats, uint16_t *m_rounds);

/* The matchup groups of one (root, k): the records of fk_tournament_run_matchups of the WHOLE range, in coordinate order
 * (n_obs < 2^31).  Groups are equal seat tuples; a group's series is its n_rounds in record order.
 *   counts      int64 [4]: observations, candidate groups, eligible groups (count >= lags[0] + 2), returned groups M
 *   histogram   uint64 [lags[0] + 2 + 64]: groups per _observation_histogram_bin code (rng_diagnostics.py:1568)
 *   cap         > 0: return the `cap` eligible groups of least priority (_priority :1281, group_type 1) and every group whose
 *               priority equals the last one's (the caller breaks such ties by the rest of the tuple); <= 0: every eligible group
 *   out_*       [out_capacity] groups in ascending priority: digest, m_seats tuple (uint16 [k]), count, and per lag the int64 sums
 *               out_sums [M][n_lags][6]: pairs, sum x, sum y, sum x^2, sum y^2, sum xy (x = observation i - lag, y = i)
 * M > out_capacity returns FK_ERR_ARG with counts[3] = M.  Option "matchup_sort_key_mask" (tests): the digest bits the sort uses;
 * groups stay exact (digest-collision runs are split by tuple). */
int fk_matchup_reduce(fk_ctx *ctx, int32_t k, int64_t n_obs, const uint64_t *digest, const uint16_t *seats, const uint16_t *rounds,
                      const int32_t *lags, int32_t n_lags, int64_t cap, int64_t out_capacity, int64_t *counts, uint64_t *histogram,
                      uint64_t *out_digest, uint16_t *out_seats, int64_t *out_count, int64_t *out_sums);

/* fk_tournament_run_all_player (seat_stats / seat_ratio_sums nullable: pass both, only seat_stats, or neither) + the sufficient
 * statistics of the reference's game-stats stage for this range (analysis/game_stats.py: _compute_k_game_stats :840-1220, margins
 * _compute_margin_arrays :3378-3406, rare-event summary sums _build_rare_event_summary_shard :2715-2880).  All outputs int64,
 * overwritten; margins are in units of 50 points (seat scores are multiples of 50):
 *   strategy_counts   [S][4]  over the strategy's seat exposures: attempted, completed, safety-limit, games where at least two seats
 *                             have score >= rare_target_score (analysis.rare_event_target_score)
 *   strategy_rounds   [S][rounds_bins]  n_rounds histogram of its exposures
 *   strategy_runner / strategy_spread   [S][margin_bins]  (max - second max) / 50 and (max - min) / 50 of the game's seat scores,
 *                             over its COMPLETED exposures of games with k >= 2
 *   game_counts [4], game_rounds [rounds_bins], game_runner [margin_bins]   the same over the range's games
 * Nothing is clamped: a value beyond its histogram (n_rounds >= rounds_bins, margin / 50 >= margin_bins) is an entry of
 *   spill   int32 [spill_capacity][3]: strategy table index (-1: the game level), kind (0 n_rounds, 1 runner-up, 2 spread), value
 * *spill_count = the entries the call produced; more than spill_capacity returns FK_ERR_ARG (call again with that capacity).
 * 1 <= rounds_bins <= 4096, 1 <= margin_bins <= 2048, k <= FK_MAX_PLAYERS.  Option "game_stats_window" (tests): > 0 narrows both device windows to that
 * many bins, so that values spill; results are the same.  Per workgroup the device gathers one strategy's exposures over a segment
 * of shuffles into LDS histograms (farkle_ii_amd/csrc/fk_game_stats.h); farkle_ii_amd/game_stats.py builds the reference's tables. */
int fk_tournament_run_game_stats(fk_ctx *ctx, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                                 uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch,
                                 int32_t target_score, int32_t max_rounds, const fk_override *ov, int32_t n_ov,
                                 int64_t *tally, void *rows, int32_t *perms, int64_t *seat_stats, double *seat_ratio_sums,
                                 int32_t rare_target_score, int32_t rounds_bins, int32_t margin_bins, int64_t *strategy_counts,
                                 int64_t *strategy_rounds, int64_t *strategy_runner, int64_t *strategy_spread, int64_t *game_counts,
                                 int64_t *game_rounds, int64_t *game_runner, int64_t spill_capacity, int64_t *spill_count,
                                 int32_t *spill);

/* fk_tournament_run_game_stats (every argument and output up to `spill` as there, the same bits) + what the reference's
 * rare-event shards need beyond the summary sums (analysis/game_stats.py: _build_rare_event_summary_shard :2715-2984,
 * _rare_event_details :2987-3153, _resolve_rare_event_thresholds :3293-3328):
 *   strategy_second [S][second_bins], game_second [second_bins]   int64 histograms of the game's second-highest seat score / 50
 *                             over ALL attempted games with k >= 2, safety-limit games included (_second_highest :3395-3406), per
 *                             seat exposure and per game as the runner-up histograms; k = 1 contributes nothing.  A value
 *                             >= second_bins is a spill entry of kind 3 in the same spill list.  1 <= second_bins <= 4096.
 *   margin_thresholds [n_thresholds]   0 .. 8 thresholds in points, any sign.  A game is an EVENT when
 *                             multi        at least two seats have score >= rare_target_score, or
 *                             margin_le[i] it completed, k >= 2 and its runner-up margin in points is <= margin_thresholds[i].
 *   event_head  uint32 [event_capacity][4]:  x = shuffle index - shuffle_begin;
 *                             y = game index | completed << 16 | multi << 17 | threshold mask << 18 (bit i = margin_le[i]);
 *                             z = runner-up margin / 50, w = score spread / 50 (both 0 unless completed with k >= 2)
 *   event_seats uint16 [event_capacity][k]:  the seats' strategy table indices in seat order
 * Events come out in ascending (shuffle, game) order, whatever the grid, the workspace chunking ("chunk_bytes") and the split of a
 * shuffle range over calls: the lists of a split, concatenated (x rebased), equal the list of the one call.  *event_count = the
 * events the call produced; more than event_capacity returns FK_ERR_ARG (call again with that capacity; when the spill list is
 * too small as well, both counts are reported by the same return).  k <= FK_MAX_PLAYERS.  event_capacity = 0 with n_thresholds = 0 and null lists is
 * the histograms-only call: no game is examined for events and *event_count = 0.  The range may hold at most 2^32 - 1 shuffles and
 * S / k at most 65536 games per shuffle.  The second score is kept in a second per-game record array (4 bytes per game), so the
 * 16-byte game records of fk_tournament_run_game_stats are unchanged; the list is an order-preserving stream compaction
 * (wave ballots, a one-workgroup scan of the workgroup counts carried across chunks, a scatter): farkle_ii_amd/csrc/fk_rare_events.h;
 * farkle_ii_amd/rare_events.py resolves the quantile thresholds and holds the host statement. */
int fk_tournament_run_rare_events(fk_ctx *ctx, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                                  uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch,
                                  int32_t target_score, int32_t max_rounds, const fk_override *ov, int32_t n_ov,
                                  int64_t *tally, void *rows, int32_t *perms, int64_t *seat_stats, double *seat_ratio_sums,
                                  int32_t rare_target_score, int32_t rounds_bins, int32_t margin_bins, int64_t *strategy_counts,
                                  int64_t *strategy_rounds, int64_t *strategy_runner, int64_t *strategy_spread, int64_t *game_counts,
                                  int64_t *game_rounds, int64_t *game_runner, int64_t spill_capacity, int64_t *spill_count,
                                  int32_t *spill, int32_t second_bins, int64_t *strategy_second, int64_t *game_second,
                                  int32_t n_thresholds, const int32_t *margin_thresholds, int64_t event_capacity,
                                  int64_t *event_count, uint32_t *event_head, uint16_t *event_seats);

/* fk_tournament_run (the same arguments, the same tally bits) + the sufficient statistics of the reference's seat-analysis stage
 * for this range (analysis/seat_analysis.py: _iter_seat_count_tables :170-235, _MirroredPartitionWriter.__call__ :618-714):
 *   seat_counts  int64 [n_batches][S][k][3], overwritten: per deterministic batch, strategy (table index) and seat its wins,
 *                completed exposures and safety-limit exposures (exposures = completed + safety; a cell of all zeros is a cell
 *                the reference does not emit).  1 <= k <= 16 (narrower than FK_MAX_PLAYERS).
 * Mirrored pairs, k = 2 only (every pair argument null / 0 otherwise, FK_ERR_ARG if not):
 *   id_rank      uint16 [S]: the rank of table index i by strategy ID (a permutation of 0 .. S - 1: IDs are unique)
 *   pair_index   uint16 [pair_capacity][2]: the pair's table indices, the lower strategy ID first
 *   pair_sums    int64 [pair_capacity][6]: paired games, P1-win difference sum, completed games, safety-limit games, unpaired
 *                forward games, unpaired reverse games — each the sum over the call's batches of the per-batch pairing: inside one
 *                (batch, pair) the i-th completed forward game (seat 1 = the lower ID) is paired with the i-th completed reverse
 *                game, in (shuffle, game) order, which is what the reference's two FIFO queues do.
 *   *pair_count  the pairs the call produced, rows in ascending (rank a, rank b); more than pair_capacity returns FK_ERR_ARG
 *                (call again with that capacity).
 * With pair outputs shuffle_begin must be a multiple of shuffles_per_batch (a call never starts inside a batch; it may end with a
 * short one) and the range may hold at most 2^31 - 2 games.  Results do not depend on "chunk_bytes".  The counts are gathered per
 * strategy from the 4-byte result word of its game (farkle_ii_amd/csrc/fk_seat_analysis.h); the pairs are one stable radix sort of
 * the range's games by (rank a, rank b, batch) and a segmented scan.  farkle_ii_amd/seat_analysis.py builds the reference's frames. */
int fk_tournament_run_seat_counts(fk_ctx *ctx, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                                  uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch,
                                  int32_t target_score, int32_t max_rounds, const fk_override *ov, int32_t n_ov,
                                  int64_t *tally, int64_t *seat_counts, const uint16_t *id_rank, int64_t pair_capacity,
                                  int64_t *pair_count, uint16_t *pair_index, int64_t *pair_sums);

/* Explicit game list: game g seats strategies table[seat_strategy[g*k+i]] with streams coords[g](seat i).
 * rows: n_games * (4+28k) bytes (required).  1 <= k <= FK_MAX_PLAYERS. */
int fk_play_games(fk_ctx *ctx, const fk_coord *coords, int64_t n_games, const fk_strategy *table, int32_t S,
                  const int32_t *seat_strategy, int32_t k, int32_t target_score, int32_t max_rounds, void *rows);

/* One roll of a traced game (fk_trace_games), 16 bytes.  What FarklePlayer.take_turn (src/farkle/game/engine.py:208-273) sees and does
 * at one trip of its loop: _roll (:85-101), _score_roll (:103-147), _apply_hot_dice (:149-154), _should_continue (:156-205). */
typedef struct {
    uint32_t dice;       /* bits 3i..3i+2, i < n_dice: face (1..6) of die i in DRAW order; bits 18..20: n_dice; rest 0 */
    int32_t  turn_score; /* the turn's points after this roll (0 after a farkle) */
    uint16_t points;     /* default_score's score for this roll, after discards; 0 = farkle */
    uint16_t round;      /* 1-based round the roll belongs to (the final round's turns carry the trigger's round) */
    uint8_t  seat;       /* 0-based */
    uint8_t  used_left;  /* low nibble: default_score's `used` (0 on a farkle); high nibble: dice the turn goes on with
                            (_score_roll's next_dice: 0 farkle, 6 hot dice, else reroll) */
    uint8_t  discards;   /* low nibble d5, high nibble d1 (default_score(return_discards=True)) */
    uint8_t  flags;      /* 1: strategy.decide was consulted (not on a farkle, not on an auto-hot-dice roll, not when
                            _should_continue banks on `final_round and running_total > score_to_beat and not run_up_score`);
                            2: the turn rolls again; 4: final_round; 8: this roll was continued by auto_hot_dice */
} fk_roll_event;
#define FK_EV_DECIDE 1
#define FK_EV_ROLL_AGAIN 2
#define FK_EV_FINAL_ROUND 4
#define FK_EV_AUTO_HOT 8

/* Roll-level trace of an explicit game list: the arguments and checks of fk_play_games, the same rows, plus per game the ordered
 * list of its roll events — FarkleGame.play / _run_final_round (src/farkle/game/engine.py:436-550) around FarklePlayer.take_turn
 * (:208-273), which is what `farkle watch` logs (src/farkle/simulation/watch_game.py:141-221).
 *   rows         n_games * (4+28k) bytes, required: byte for byte the rows fk_play_games returns for the same arguments
 *   event_begin  int64 [n_games + 1], required: game g owns events [event_begin[g], event_begin[g + 1]), in play order; games in
 *                input order; a game without a roll (max_rounds = 0) owns an empty range
 *   events       NULL = a counting call (rows and event_begin only); else event_capacity records.  A capacity below
 *                event_begin[n_games] returns FK_ERR_ARG with event_begin filled, nothing stored in `events` and the needed count
 *                in the error text (the convention of the spill and pair lists).
 * The trace is played by its own kernel (farkle_ii_amd/csrc/fk_trace.h) from the table-free device functions — sequential dice,
 * SWAR scorer, should_continue in points — and shares neither the score / discard tables nor the fast dice path with the game
 * kernels: equal rows are a cross-check of those kernels through an independent path, not a recording of their lanes.  A turn of
 * more than 1000 rolls returns FK_ERR_ROLL_LIMIT, a row counter beyond 65535 FK_ERR_COUNTER_OVERFLOW. */
int fk_trace_games(fk_ctx *ctx, const fk_coord *coords, int64_t n_games, const fk_strategy *table, int32_t S,
                   const int32_t *seat_strategy, int32_t k, int32_t target_score, int32_t max_rounds,
                   void *rows, int64_t *event_begin, fk_roll_event *events, int64_t event_capacity);

/* Roll census: exact integer tables over every roll and turn of the games of a call (farkle_ii_amd/csrc/fk_census.h).  "Raw" is the
 * roll's maximum immediate score and its scoring dice BEFORE Smart-5 / Smart-1 discards — the reference's
 * score_roll_cached(outcome)[:2] (src/farkle/analysis/roll_enumeration.py), whose exact law over the 6^n ordered outcomes has 127
 * cells.  The caller owns the four tables; a call SETS them (it does not add to them) and a failed call stores nothing in them.
 *   roll_cells      [6][61][7]      [dice rolled - 1][raw score / 50][raw dice used]: rolls
 *   strategy_dice   [S][6][3]       for the strategy whose turn it is, by dice rolled - 1: rolls, farkles (raw score 0), rolls in which
 *                                   every die scored (raw used == dice rolled)
 *   strategy_turns  [S][3]          turns, turns that ended on a farkle, sum of the turns' final turn_score in points (0 after a farkle)
 *   turn_hist       [S][turn_bins]  turns by final turn_score / 50, clamped to turn_bins - 1; 2 <= turn_bins <= 4096 */
typedef struct {
    int32_t turn_bins;
    uint64_t *roll_cells;       /* [6][61][7] */
    uint64_t *strategy_dice;    /* [S][6][3]  */
    uint64_t *strategy_turns;   /* [S][3]     */
    uint64_t *turn_hist;        /* [S][turn_bins] */
} fk_census;

/* The census of an explicit game list: the arguments and checks of fk_trace_games.  The tables are a pure function of the event
 * stream fk_trace_games returns for the same arguments (a turn ends at the event without FK_EV_ROLL_AGAIN; a roll's raw cell follows
 * from its faces), played by a kernel of its own that stores no event and no row.  The list is played in chunks that fit the
 * context's workspace budget; option "census_chunk_games" > 0 caps a chunk (tests).  A turn of more than 1000 rolls returns
 * FK_ERR_ROLL_LIMIT, a row counter beyond 65535 FK_ERR_COUNTER_OVERFLOW, naming the smallest offending game as fk_trace_games does. */
int fk_census_games(fk_ctx *ctx, const fk_coord *coords, int64_t n_games, const fk_strategy *table, int32_t S,
                    const int32_t *seat_strategy, int32_t k, int32_t target_score, int32_t max_rounds, fk_census *out);

/* The census of the games fk_tournament_run plays for the same range: the same permutations (made on the device by the same
 * kernels), seat streams (namespace 103) and max_rounds overrides.  shuffles_per_batch is checked and otherwise unused: the tables
 * cover the whole range.  Errors name the game's index in the range (shuffle - shuffle_begin) * (S / k) + game. */
int fk_tournament_run_census(fk_ctx *ctx, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                             uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score,
                             int32_t max_rounds, const fk_override *ov, int32_t n_ov, fk_census *out);

/* H2H block: attempts [state[0], min(max_attempts, state[0]+chunk_games)) of (root, pair, order) in
 * attempt order until `target` completed games; state = {attempted, completed, safety, wins_seat1,
 * wins_seat2} in/out (h2h_schedule.py:1165-1235). */
int fk_h2h_run(fk_ctx *ctx, const fk_strategy seats[2], uint64_t root_seed, uint64_t pair_id, uint32_t order,
               uint64_t target, uint64_t max_attempts, uint64_t chunk_games, int32_t target_score,
               int32_t max_rounds, const fk_override *ov, int32_t n_ov, uint64_t state[5]);

/* One (pair, order) block of a batched H2H call: the two seated strategies, the block's coordinates and limits, and its
 * progress {attempted, completed, safety, wins_seat1, wins_seat2} in/out (h2h_schedule.py:1088-1146, 1165-1235). */
typedef struct {
    fk_strategy seats[2];
    uint64_t pair_id;
    uint32_t order;
    uint32_t pad;
    uint64_t target, max_attempts;
    uint64_t state[5];
} fk_h2h_block;

/* Many H2H blocks of one root advanced together, each by at most chunk_games attempts, each exactly as fk_h2h_run would
 * advance it alone (same in-order prefix rule per block); all blocks share the kernel launches (the production H2H
 * schedule is tens of thousands of blocks of ~2 000 games: execute_h2h_schedule's block loop, h2h_schedule.py:2038-2093). */
int fk_h2h_run_blocks(fk_ctx *ctx, fk_h2h_block *blocks, int64_t n_blocks, uint64_t root_seed, uint64_t chunk_games,
                      int32_t target_score, int32_t max_rounds, const fk_override *ov, int32_t n_ov);

/* Head-to-head round robin: pairs [pair_begin, pair_end) of an n-row table, both seat orders, every (pair, order) block fresh and
 * played to its terminal status by the prefix rule (h2h_schedule.py:1172-1235): attempts 0, 1, ... in order until `target` games
 * have completed or `max_attempts` attempts are used.
 *   pair_id      the position of (i, j), i < j, in itertools.combinations(range(n), 2), as _schedule_frame numbers the pairs of
 *                sorted(candidates) (h2h_schedule.py:564): the caller passes the table sorted by strategy id
 *   seats        order 0 seats table[i] in seat 1 and table[j] in seat 2, order 1 swaps them (:567-568); seat streams from
 *                namespace 203 with (root_seed, k = 2, pair_id, order, attempt_index, seat), as fk_h2h_run_blocks
 *   block_state  written: [pair_end - pair_begin][2 orders][FK_RR_STATE_COLS] = attempted, completed, safety, wins_seat1,
 *                wins_seat2 — word for word what fk_h2h_run_blocks returns for a fresh block with these seats, pair_id, order,
 *                target and max_attempts at chunk_games = max_attempts
 *   summary      nullable, ADDED to (pair ranges and roots accumulate in the caller's buffer; nothing is added when the call
 *                fails): [n][FK_RR_SUMMARY_COLS] over the pairs of the range that contain strategy s, both orders —
 *                0 pairs | 1 pairs_resolved (both blocks reached target) | 2 games_completed | 3 games_safety | 4 wins (of s) |
 *                5 seat1_games_completed (s in seat 1) | 6 seat1_wins | 7 pairs_ahead (resolved pairs in which s won more games
 *                over both orders than its opponent)
 * Nothing per block crosses the bus on the way in: the table is uploaded once and the device unranks pair ids, plans its own
 * generations and passes (fk_round_robin.h) in windows of option "rr_window_blocks" blocks (even, 2 .. 2^22, default 2^22 — a
 * scheduling choice only, results are identical for every setting).  FK_ERR_ARG before any device work: n < 2; pair_begin >
 * pair_end or pair_end > n (n - 1) / 2; target == 0, target > max_attempts or max_attempts > 2^31 - 1; max_rounds outside
 * [0, 65535]; a target_score the batched H2H instance cannot play; an invalid strategy.  An empty range returns FK_OK and
 * touches nothing.  fk_timing and fk_last_play_instance are filled as for fk_h2h_run_blocks; an out-of-memory failure replays
 * the whole call with half the workspace budget.  max_rounds overrides (fk_override) are not part of this entry: they are a
 * test-oracle device keyed to one planned schedule (use fk_h2h_run_blocks for those). */
#define FK_RR_STATE_COLS 5
#define FK_RR_SUMMARY_COLS 8
int fk_h2h_round_robin(fk_ctx *ctx, const fk_strategy *table, int32_t n, uint64_t root_seed, uint64_t pair_begin,
                       uint64_t pair_end, uint64_t target, uint64_t max_attempts, int32_t target_score, int32_t max_rounds,
                       uint32_t *block_state, int64_t *summary);

/* ---- round-robin inference: the score test, the score intervals, Holm's adjustment and the decision class of every pair of a
 * resident pair range (src/farkle/analysis/h2h_inference.py), on counts that stay on the device ----
 *
 * The context owns ONE accumulator: for every (pair, order) of a pair range [pair_begin, pair_end) of an n-row table the 64-bit
 * sums over the roots added so far of games_attempted, games_completed, games_safety_limit, wins_seat1, wins_seat2,
 * n_completed_required (the block's target), max_attempts, the (root, order) cells added and those of them that ended `complete`
 * (completed == target) — what _combine_within_order (h2h_inference.py:563-635) sums across roots without mixing the orders.
 * The first adding call after fk_rr_counts_reset (or on a fresh context) fixes (n, pair_begin, pair_end), a hash of the table and
 * family_pair_count; every later one must repeat them (FK_ERR_ARG otherwise).  A failed call adds nothing.
 *
 * fk_h2h_round_robin_resident  fk_h2h_round_robin without block_state: the same windows, generations, passes, apply and summary
 *                              kernels play the same games; the states stay on the device and are added to the accumulator when the
 *                              whole call has succeeded (so that a failed or replayed call adds nothing, the summary's rule).
 *                              An empty range is FK_ERR_ARG here: there is nothing to keep resident.
 * fk_rr_counts_add             one root's host-held states [pair_end - pair_begin][2][FK_RR_STATE_COLS], as fk_h2h_round_robin
 *                              returned them for this target / max_attempts (earlier runs, other ranks), into the accumulator
 * fk_rr_counts_reset           forgets the accumulator's contents and what was fixed with them
 *
 * family_pair_count is the reference's unordered_pair_count (:711): it sizes the Bonferroni alpha of the simultaneous interval
 * (family_alpha / family_pair_count, :715) and is at least the resident range's pair count; a table-wide range passes the table's
 * pair count.  Holm's family is the resident range itself. */
int fk_h2h_round_robin_resident(fk_ctx *ctx, const fk_strategy *table, int32_t n, uint64_t root_seed, uint64_t pair_begin,
                                uint64_t pair_end, uint64_t target, uint64_t max_attempts, int32_t target_score, int32_t max_rounds,
                                int64_t *summary, uint64_t family_pair_count);
int fk_rr_counts_add(fk_ctx *ctx, const fk_strategy *table, int32_t n, uint64_t pair_begin, uint64_t pair_end, uint64_t target,
                     uint64_t max_attempts, const uint32_t *block_state, uint64_t family_pair_count);
int fk_rr_counts_reset(fk_ctx *ctx);

typedef struct {
    double family_alpha;                  /* head2head.family_alpha: Holm's level and the ordinary interval's alpha */
    double practical_delta;               /* > 0 */
    double delta_equivalence;             /* in (0, 1), or NaN: equivalence is off (the reference's None) */
    double min_candidate_completion_rate; /* in [0, 1] */
    double critical_ordinary;             /* norm.isf(family_alpha / 2), evaluated by the caller (:255) */
    double critical_simultaneous;         /* norm.isf(family_alpha / family_pair_count / 2) */
    uint64_t family_pair_count;           /* as fixed with the accumulator */
} fk_rr_inference_params;

/* One pair of _pairwise_estimates' frame (:739-860, :870-913), 224 bytes.  A is table[strategy_a], B is table[strategy_b],
 * strategy_a < strategy_b.  The counts are written for every pair; the doubles that the reference leaves None for a pair
 * without a test are NaN.  The d bounds are the halved interval bounds (:851-854). */
#define FK_RR_FLAG_INFERENTIALLY_VIABLE 1 /* = formal_test_performed */
#define FK_RR_FLAG_OPERATIONALLY_VIABLE 2
#define FK_RR_FLAG_CLAIM_ELIGIBLE 4
#define FK_RR_FLAG_HOLM_REJECT_BEFORE_VIABILITY 8
#define FK_RR_FLAG_HOLM_REJECT 16
enum {
    FK_RR_PRACTICAL_DOMINANCE_A = 0,
    FK_RR_PRACTICAL_DOMINANCE_B = 1,
    FK_RR_STATISTICAL_ONLY_ADVANTAGE_A = 2,
    FK_RR_STATISTICAL_ONLY_ADVANTAGE_B = 3,
    FK_RR_EQUIVALENT = 4,
    FK_RR_UNRESOLVED = 5,
    FK_RR_UNRESOLVED_NONVIABLE = 6
};
#define FK_RR_CLASSES 7
#define FK_RR_STRATEGY_COLS 12
typedef struct {
    uint64_t pair_id;
    int64_t games_attempted, games_completed, games_safety_limit, n_completed_required; /* both orders */
    int64_t n_ab, n_ba, seat1_a_wins_ab, seat1_b_wins_ba, seat2_a_wins_ba, balanced_a_wins;
    int64_t holm_order; /* 1-based position in Holm's stable order; 0 = no test performed */
    double completion_game_rate, q_ab, q_ba, raw_order_rate_difference, d_ab, score_null_proportion, score_z, score_p_value;
    double ordinary_d_low, ordinary_d_high, simultaneous_d_low, simultaneous_d_high, balanced_a_win_rate, holm_adjusted_p;
    uint32_t strategy_a, strategy_b; /* table rows */
    uint8_t flags;                   /* FK_RR_FLAG_* */
    uint8_t decision_class;          /* FK_RR_PRACTICAL_DOMINANCE_A .. FK_RR_UNRESOLVED_NONVIABLE */
    uint8_t pad[6];
} fk_rr_pair_row;

/* The inference over the resident range, in the stages of _viability_status (:638-700) and _pairwise_estimates (:703-915):
 *   viability   a pair is inferentially viable when every cell of both orders is complete and completed == required; a strategy is
 *               operationally viable when completed / attempted over its incident pairs (one IEEE division) is at least
 *               min_candidate_completion_rate, inferentially viable when all its incident pairs are; a pair is claim-eligible
 *               when it is viable and both its strategies are operationally viable (:754-756)
 *   score test  two_proportion_score_test (:68-99) on x_ab = A's wins in order 0, x_ba = B's wins in order 1, in the reference's
 *               statement order without contraction; p = erfc(|z| / sqrt 2)
 *   intervals   at family_alpha and at family_alpha / family_pair_count: the reference's own complete inversion
 *               (_score_difference_interval_fallback, :234-277) — the swap for a positive estimate, the dyadic bracket of
 *               _score_interval_bound (:191-231), a bracketing solver down to a bracket of 2^-44, the symmetric rule; the library
 *               route of score_difference_interval (confint_proportions_2indep, :118-138) is not reproduced
 *   Holm        _holm_adjust (:280-295) over ALL pairs of the range, a pair without a test entering as 1.0 (:864-868): a stable
 *               radix sort of the p-values' bit patterns, (count - index) * p, a running maximum, min(1, .)
 *   class       the chain of :886-909
 * Outputs:
 *   rows              nullable: the pairs [row_begin, row_end) (pair ids, inside the resident range), in order
 *   class_counts      [FK_RR_CLASSES] pairs of the range per decision class
 *   strategy_classes  nullable: [n][FK_RR_STRATEGY_COLS] per strategy, over its incident pairs of the range — 0 pairs it wins by
 *                     practical dominance | 1 loses by it | 2 wins by statistical-only advantage | 3 loses by it | 4 equivalent |
 *                     5 unresolved | 6 unresolved_nonviable | 7 games_attempted | 8 games_completed | 9 games_safety_limit |
 *                     10 operationally_viable | 11 inferentially_viable (the completion rate is 8 / 7)
 * fk_timing: play_ms = total_ms = the entry's device work between two events on the context's stream (the copies back excluded).
 * FK_ERR_ARG before any device work: no resident counts; a row range outside the resident one (with rows given); family_alpha
 * outside (0, 1); practical_delta <= 0; delta_equivalence outside (0, 1); min_candidate_completion_rate outside [0, 1];
 * family_pair_count smaller than the range or other than the one fixed with the counts; a critical value that is not positive
 * and finite; a range of 2^31 pairs or more. */
int fk_rr_inference(fk_ctx *ctx, const fk_rr_inference_params *params, fk_rr_pair_row *rows, uint64_t row_begin, uint64_t row_end,
                    int64_t *class_counts, int64_t *strategy_classes);

/* ---- round-robin inference, per root: the fixed-root diagnostics and the cross-root agreement of _root_specific_diagnostics
 * (h2h_inference.py:918-1059) ----
 *
 * The accumulator sums the roots away on arrival.  With option "rr_keep_roots" = 1 (0 / 1, default 0; FK_ERR_ARG while counts are
 * resident) every adding call that succeeds also keeps its states [pairs][2][FK_RR_STATE_COLS] on the device, in one of
 * FK_RR_MAX_ROOTS root slots, with (root_seed, target, max_attempts): fk_h2h_round_robin_resident under its own root_seed,
 * fk_rr_counts_add_root (fk_rr_counts_add plus the slot) under the one it is given.  A failed or replayed call keeps nothing.
 * FK_ERR_ARG before any device work, accumulator and slots untouched: a root_seed already kept; a root beyond FK_RR_MAX_ROOTS.
 * Plain fk_rr_counts_add with the option on adds as ever and marks the root set untracked (the accumulator then holds cells that no
 * slot holds; later calls keep nothing more).  fk_rr_counts_reset forgets the slots.  With the option at 0 nothing is kept and
 * fk_rr_counts_add_root is fk_rr_counts_add. */
#define FK_RR_MAX_ROOTS 2
int fk_rr_counts_add_root(fk_ctx *ctx, const fk_strategy *table, int32_t n, uint64_t pair_begin, uint64_t pair_end, uint64_t target,
                          uint64_t max_attempts, const uint32_t *block_state, uint64_t family_pair_count, uint64_t root_seed);

/* One (root, pair) of root_pairwise_diagnostics (:957-992), 168 bytes: fk_rr_pair_row's conventions, the counts those of this root
 * alone.  flags: FK_RR_FLAG_*; the three viability bits are the COMBINED ones (:937-943), the two Holm bits this root's. */
enum { FK_RR_DIAGNOSTIC_NO_ADJUSTED_REJECTION = 0, FK_RR_DIAGNOSTIC_ADVANTAGE_A = 1, FK_RR_DIAGNOSTIC_ADVANTAGE_B = 2 };
#define FK_RR_DIAGNOSTIC_NONE 255 /* fk_rr_agreement_row::root_b_decision when there is one root */
typedef struct {
    uint64_t pair_id;
    int64_t games_attempted, games_completed, games_safety_limit; /* both orders, this root */
    int64_t n_ab, n_ba, seat1_a_wins_ab, seat1_b_wins_ba;
    int64_t holm_order; /* 1-based position in this root's stable Holm order; 0 = no test performed */
    double completion_game_rate, q_ab, q_ba, d_ab, score_null_proportion, score_z, score_p_value;
    double ordinary_d_low, ordinary_d_high, holm_adjusted_p;
    uint32_t strategy_a, strategy_b; /* table rows */
    uint8_t flags;
    uint8_t diagnostic_decision; /* FK_RR_DIAGNOSTIC_* */
    uint8_t pad[6];
} fk_rr_root_row;

/* One pair of root_decision_agreement (:1003-1057), 56 bytes.  root_a is the root with the smaller seed (unsigned).  NaN where the
 * reference leaves None; with one root the root_b half is NaN / FK_RR_DIAGNOSTIC_NONE and no flag is set. */
#define FK_RR_AGREE_AVAILABLE 1 /* both effects exist */
#define FK_RR_AGREE_DECISION 2  /* available and the two diagnostic decisions are equal */
#define FK_RR_AGREE_DIRECTION 4 /* available and int(sign(a)) == int(sign(b)): a zero effect agrees only with another zero */
typedef struct {
    uint64_t pair_id;
    double root_a_d_ab, root_b_d_ab, effect_discrepancy_a_minus_b, absolute_effect_discrepancy;
    uint32_t strategy_a, strategy_b;
    uint8_t root_a_decision, root_b_decision; /* FK_RR_DIAGNOSTIC_* */
    uint8_t flags;                            /* FK_RR_AGREE_* */
    uint8_t pad[5];
} fk_rr_agreement_row;

/* The diagnostics over the kept roots, in ascending seed order:
 *   viability   the COMBINED accumulator's, as fk_rr_inference computes it (a pair that another root's block makes nonviable has no
 *               test in any root; operational viability is the all-roots completion rate); no simultaneous interval is computed
 *   per root    the score test on the root's own counts, Holm over all pairs of the range (1.0 without a test), holm_reject =
 *               performed and adjusted p <= family_alpha and claim-eligible, the diagnostic decision (:945-953), and for the rows of
 *               the asked slice the ordinary interval
 *   agreement   per pair, from the two roots' effects and decisions
 * Outputs:
 *   root_seeds  [FK_RR_MAX_ROOTS] the kept seeds, ascending as unsigned 64-bit (entries past n_roots are 0); n_roots 1 or 2
 *   rows        nullable: [n_roots][row_end - row_begin], roots in root_seeds' order
 *   agreement   nullable: [row_end - row_begin]
 *   summary     [FK_RR_AGREE_COLS] over the whole resident range: 0 pairs | 1 agreement available | 2 decision agreements |
 *               3 direction agreements (both over the available pairs) | per root r at 4 + 4 r: pairs without an adjusted rejection,
 *               with advantage a, with advantage b, tests performed
 *   max_abs_discrepancy  nullable: the largest absolute_effect_discrepancy over the available pairs, NaN when there is none
 * fk_timing as fk_rr_inference.  FK_ERR_ARG before any device work: every refusal of fk_rr_inference; no kept roots (the option is
 * off); an untracked root set; a row range outside the resident one (with rows or agreement given); a null root_seeds, n_roots or
 * summary. */
#define FK_RR_AGREE_COLS 12
int fk_rr_root_diagnostics(fk_ctx *ctx, const fk_rr_inference_params *params, uint64_t *root_seeds, int32_t *n_roots,
                           fk_rr_root_row *rows, uint64_t row_begin, uint64_t row_end, fk_rr_agreement_row *agreement,
                           int64_t *summary, double *max_abs_discrepancy);

/* ---- dominance graphs of a round robin: what src/farkle/analysis/dominance.py builds from the pairwise decision classes, for
 * both of its graphs in one call — index 0 practical (edges of practical_dominance_*), index 1 statistical (edges of every class
 * ending _a / _b), dominance.py:285-334.  Node ids are table rows; a pair's A is its smaller row.  Device side: fk_dominance.h. ----
 *
 * fk_dom_node, per table row (64 bytes), [g] per graph:
 *   component[g]       the smallest row of the node's strongly connected component ("cycle group" when its size is above 1)
 *   component_size[g]
 *   front[g]           1-based layer of the component in the condensation: one more than the largest front among the components
 *                      with an edge into it (:118-136)
 *   cycle_length[g]    length of the shortest directed cycle through the node inside its component; 0 for a component of one
 *   wins[g], losses[g] edges out of and into the node (:386-389)
 *   rate_count, rate_mean  the pairs of the node with a rate, and the mean over them of balanced_rate (as A) / 1 - balanced_rate
 *                      (as B), summed in pair-id order from 0.0 and divided once (:357-395); NaN when there is none
 * fk_dom_extreme, [g][row] (32 bytes): at a component's smallest row the practical edge with both ends inside the component whose
 *   practical_distance_beyond_threshold (:315-319: simultaneous_d_low - practical_delta for an edge won by A, -simultaneous_d_high -
 *   practical_delta for one won by B) is largest / smallest, ties to the smallest (rank[winner], rank[loser]) (:504-520).  Winners
 *   and losers UINT32_MAX and distances NaN at every other row and for a component without such an edge.
 * adjacency, nullable: [2][n][W] 64-bit words, W = ceil(n / 64); bit j of row i of graph g: i beats j.  Padding bits are zero.
 *
 * The closure behind the components is a blocked Warshall over 64-bit words, the fronts are Kahn's rounds in one workgroup's LDS,
 * the cycle lengths one breadth-first search per node: n is at most FK_DOM_MAX_N. */
#define FK_DOM_MAX_N 8192
typedef struct {
    uint32_t component[2], component_size[2], front[2], cycle_length[2], wins[2], losses[2];
    uint64_t rate_count;
    double rate_mean;
} fk_dom_node;
typedef struct {
    uint32_t strongest_winner, strongest_loser, weakest_winner, weakest_loser;
    double strongest_distance, weakest_distance;
} fk_dom_extreme;

/* The graph stage alone, on host arrays in pair-id order (P = n (n - 1) / 2): decision_class (FK_RR_PRACTICAL_DOMINANCE_A ..),
 * the simultaneous d bounds, balanced_a_win_rate (NaN: the pair has none).  rank, nullable: rank[row] = the position of the row's
 * strategy in the order that breaks ties between equal distances (the reference orders strategies as strings); NULL = table order.
 * fk_timing: play_ms = total_ms = the device work (copies excluded); perm_ms of it builds the edges, seed_ms closes the matrices.
 * FK_ERR_ARG before any device work: a null array; n < 2 or n > FK_DOM_MAX_N; a class above 6; a practical class whose bound
 * (low for _a, high for _b) is not finite; practical_delta that is not positive; rank that is not a permutation of 0 .. n - 1. */
int fk_dominance_graph(fk_ctx *ctx, int32_t n, const uint8_t *decision_class, const double *sim_d_low, const double *sim_d_high,
                       const double *balanced_rate, double practical_delta, const uint32_t *rank, fk_dom_node *nodes,
                       fk_dom_extreme *extremes, uint64_t *adjacency);

/* fk_rr_inference's chain over the resident counts, its classes, simultaneous bounds and rates fed to the same graph kernels on the
 * device: no pair row comes to the host.  params and class_counts as fk_rr_inference; the other arguments as fk_dominance_graph.
 * The resident range must be the whole table (pair_begin == 0, pair_end == n (n - 1) / 2): a graph of an incomplete family is
 * refused, as the reference refuses it (:202-207).  FK_ERR_ARG before any device work: every refusal of fk_rr_inference; a partial
 * resident range; n > FK_DOM_MAX_N; rank that is not a permutation.  fk_timing: play_ms = total_ms = inference and graph together;
 * perm_ms and seed_ms as fk_dominance_graph. */
int fk_rr_dominance(fk_ctx *ctx, const fk_rr_inference_params *params, const uint32_t *rank, fk_dom_node *nodes,
                    fk_dom_extreme *extremes, uint64_t *adjacency, int64_t *class_counts);

/* ---- method agreement of a round robin: what src/farkle/analysis/structure_agreement.py computes per pair (_pair_agreement
 * :73-125) and over the scored population (kendalltau's pair counts), from the decision classes and the two screening ranks of the
 * frozen candidate membership.  Device side: fk_agreement.h. ----
 *
 * A pair's code, one byte: bits 0-1 h2h_direction, bits 2-3 win_rate_preference, bits 4-5 trueskill_preference, each 0 = none,
 * 1 = a, 2 = b.  The direction is a for classes 0 and 2, b for 1 and 3, none for 4 .. 6 (:65-70).  A preference is none when either
 * rank is null (FK_AGREE_NO_RANK) or the two are equal, otherwise a when A's rank is the smaller (:55-62); A is the pair's smaller
 * table row.  The reference's three agreement tri-states are functions of the code: available when both fields are not none, and
 * then whether they are equal.
 * counts [FK_AGREE_COUNTS]: 0 pairs | 1 directional pairs | 2 classes 5 and 6 | 3 class 6 | 4 class 4 | 5, 6 win rate against
 * TrueSkill: available, agree | 7, 8 H2H against win rate | 9, 10 H2H against TrueSkill. */
#define FK_AGREE_COUNTS 11
#define FK_AGREE_NO_RANK 0
#define FK_CONCORDANCE_COUNTS 5
#define FK_CONCORDANCE_MAX_M 65536
#define FK_CONCORDANCE_TILE 256 /* the concordance kernel's tile edge: the item counts at which it changes shape are its multiples */

/* The pair pass alone, on host arrays: decision_class in pair-id order, the ranks per table row (at least 1, or FK_AGREE_NO_RANK).
 * codes, nullable: every pair's code.  fk_timing: play_ms = total_ms = the device work, perm_ms the pair kernel in it.  FK_ERR_ARG before any device
 * work: a null required array; n < 2, or 2^31 pairs or more; a class above 6; a negative rank. */
int fk_agreement_pairs(fk_ctx *ctx, int32_t n, const uint8_t *decision_class /* [n (n - 1) / 2] */, const int32_t *win_rate_rank /* [n] */,
                       const int32_t *trueskill_rank /* [n] */, uint8_t *codes /* [pairs], nullable */, int64_t *counts);

/* fk_rr_inference's chain over the resident counts, its class array fed to the pair kernel on the device: no pair row comes to the
 * host.  params and class_counts as fk_rr_inference; the other arguments as fk_agreement_pairs.  The resident range must be the
 * whole table: the reference refuses an inference whose support differs from the finalists (:82-83).  FK_ERR_ARG before any device
 * work: every refusal of fk_rr_inference; a partial resident range; a null or negative rank array.  fk_timing: play_ms = total_ms =
 * inference and pair pass together; perm_ms of it is the pair pass. */
int fk_rr_agreement(fk_ctx *ctx, const fk_rr_inference_params *params, const int32_t *win_rate_rank, const int32_t *trueskill_rank,
                    uint8_t *codes /* nullable */, int64_t *counts, int64_t *class_counts);

/* Kendall's pair counts of m items with the keys x, y (each at least 1), over all i < j: counts [FK_CONCORDANCE_COUNTS] = 0
 * concordant | 1 discordant | 2 tied in x only | 3 tied in y only | 4 tied in both.  They sum to m (m - 1) / 2; the entry checks
 * that and returns FK_ERR_HIP if the device lost a pair.  fk_timing: play_ms = total_ms = the kernel.  FK_ERR_ARG before any device
 * work: a null array; m < 2 or m > FK_CONCORDANCE_MAX_M; a key below 1. */
int fk_rank_concordance(fk_ctx *ctx, int32_t m, const int32_t *x, const int32_t *y, int64_t *counts);

/* ---- multi-GPU: one process per GPU, one context per process, ONE exchange ----
 * The (seed x shuffle x game) space partitions with no data dependency; the only collective of the path is the integer
 * SUM of the per-strategy tally to one rank — the analogue of OutcomeCounter.absorb + _reduce_metric_chunk_payloads
 * (src/farkle/simulation/run_tournament.py:197-213, 1023-1042).  It runs as ncclReduce(sum, int64) on the context's
 * stream over RCCL/xGMI; librccl is loaded on first use.
 *   rank 0:     fk_comm_unique_id(&id); ship the 128 bytes to every rank (any channel: env, file, socket)
 *   every rank: fk_comm_init(ctx, &id, rank, world)           (collective: all ranks call it)
 *               fk_reduce_tally(ctx, tally, n, root)          (collective; `tally` is overwritten with the sum on root) */
typedef struct {
    char bytes[128];
} fk_comm_id;
int fk_comm_unique_id(fk_comm_id *out);
int fk_comm_init(fk_ctx *ctx, const fk_comm_id *id, int32_t rank, int32_t world_size);
int fk_reduce_tally(fk_ctx *ctx, int64_t *tally, int64_t n, int32_t root_rank);
/* Device-resident form of the same reduction.  With fk_set_option(ctx, "resident_tally", 1) every fk_tournament_run* call also
 * adds its [n_batches][S][26] tally to an accumulator in HBM (calls of one shape; a shape change starts a new accumulator).
 * fk_tally_resident_reduce sums the accumulators of all ranks with ncclReduce on the engine's stream — the tally does not leave
 * the device before it is reduced — copies the total to `out` on `root_rank` only (out may be NULL elsewhere) and clears the
 * accumulator.  Without a communicator (one rank) it is the plain copy.  n = elements the accumulator holds.
 * Replaces: OutcomeCounter.absorb over worker results (run_tournament.py:197-213). */
int fk_tally_resident_reduce(fk_ctx *ctx, int64_t *out, int64_t n, int32_t root_rank);
/* Ranks of the context's communicator as RCCL counts them (ncclCommCount); 1 when there is none. */
int fk_comm_ranks(fk_ctx *ctx);
int fk_comm_destroy(fk_ctx *ctx);

/* SeedSequence fingerprints of n coordinates (all nine coordinate words of the record, seat_index included):
 * seed32[i] = generate_state(1, uint32)[0], seed64[i] = generate_state(1, uint64)[0]; either may be NULL.
 * Replaces coordinate_seed (src/farkle/utils/random.py:190-232): the shuffle_seed (namespace 100) and game_seed
 * (namespace 102) columns of rows and manifests (run_tournament.py:318-351), the per-game seed of
 * simulate_many_games (namespace 1, simulation.py:700-713). */
int fk_coordinate_seeds(fk_ctx *ctx, int64_t n, const fk_coord *coords, uint32_t *seed32, uint64_t *seed64);
/* The same uint32 fingerprints for the games of a shuffle range without a coordinate list: seed32[(s - shuffle_begin) * gps + g] =
 * coordinate_seed(purpose, root_seed, k, shuffle_index = s, game_index = g) — the game_seed column of the row contract
 * (run_tournament.py:340-350; purpose 102 for tournaments). */
int fk_game_seeds(fk_ctx *ctx, uint32_t purpose, uint64_t root_seed, uint64_t k, uint64_t shuffle_begin, uint64_t n_shuffles,
                  uint32_t games_per_shuffle, uint32_t *seed32);

/* Hold device memory on purpose until about leave_free bytes are free (leave_free < 0: give everything back); free_now / total as
 * hipMemGetInfo reports them afterwards (either may be NULL).  Tests of the workspace budget and of the out-of-memory replay. */
int fk_debug_hold_memory(fk_ctx *ctx, int64_t leave_free, int64_t *free_now, int64_t *total);

/* The deadline handshake of fk_comm_init with a stand-in for ncclCommInitRank that takes init_ms: out[0] = 1 when the caller received the
 * communicator in time, 0 when it gave up at timeout_ms; out[1] = communicators torn down as orphans by the helper thread.  Host code. */
int fk_debug_deadline_handshake(int32_t init_ms, int32_t timeout_ms, int64_t *out);

/* ---- single-op probes of the device functions (parity tests) ---- */
/* n rolls: roll i scores faces[i*6 .. i*6+len[i]) for strategy[i] with turn_score_pre[i];
 * out[i*5..] = score, used, reroll, d5, d1 (default_score(return_discards=True)). */
int fk_debug_score(fk_ctx *ctx, int64_t n, const uint8_t *faces, const int32_t *len, const int32_t *turn_score_pre,
                   const fk_strategy *strategy, int32_t *out);
/* n decisions: args[i*6..] = turn_score, dice_left, has_scored, final_round, score_to_beat, player_score
 * -> out[i] = FarklePlayer._should_continue (engine.py:156-205) */
int fk_debug_should_continue(fk_ctx *ctx, int64_t n, const int32_t *args, const fk_strategy *strategy, int32_t *out);
/* n streams: coordinate -> PCG64DXSM state; then n_calls dice rolls of sizes[c] each (same sizes for all
 * streams); faces out: n * sum(sizes) bytes; raw64 (nullable): first 4 raw outputs of each stream. */
int fk_debug_dice(fk_ctx *ctx, int64_t n, const fk_coord *coords, int32_t n_calls, const int32_t *sizes,
                  uint8_t *faces, uint64_t *raw64);
/* Same but from explicit generator states: state[i*6..] = state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger. */
int fk_debug_dice_state(fk_ctx *ctx, int64_t n, const uint64_t *state, int32_t n_calls, const int32_t *sizes,
                        uint8_t *faces, uint64_t *state_out);
/* The game kernels' own dice path from explicit generator states: keys[i * n_calls + c] = the 18-bit key of call c (six 3-bit
 * face counts, face 1 in the low bits — what the score table is indexed by), produced by the roll_counts<3> instantiation of
 * fk_play_kernel / fk_play_hc_kernel incl. its Lemire-rejection replay (engine.py:101 -> Generator.integers). */
int fk_debug_dice_keys(fk_ctx *ctx, int64_t n, const uint64_t *state, int32_t n_calls, const int32_t *sizes, uint32_t *keys,
                       uint64_t *state_out);

/* The device's bounded draw (farkle_ii_amd/csrc/fk_bootstrap.h: bounded_draw, the function fk_performance_bootstrap resamples
 * with): out[i * n_draws + j] = draw j of Generator(PCG64DXSM(coords[i])).integers(0, bound, size = n_draws), i.e. numpy's
 * buffered_bounded_lemire_uint32 on the buffered 32-bit stream (low half of a 64-bit output first).  1 <= bound <= 2^32 - 1; bound 1
 * draws nothing from the stream (every result 0).  A bound such as 2^31 + 1 rejects about half the draws, which no batch count does. */
int fk_debug_bounded_draws(fk_ctx *ctx, int64_t n, const fk_coord *coords, uint64_t bound, int32_t n_draws, uint32_t *out);

/* The two consumers of a shuffle's accepted Fisher-Yates draws, driven by a draw list of the caller instead of the generator:
 * perms[sh * S + e] (n_sh x S, int32) = the result of  a = arange(S); for n = 0 .. S - 2: i = S - 1 - n, swap(a[i], a[draws[sh][n]])
 * from host draws[n_sh][S - 1] (uint16; draw n is the j of step S - 1 - n).  path 1: fk_perm_apply_kernel (the swap chains), path 2:
 * fk_perm_parallel_kernel + fk_perm_block_kernel (bucket sort + pointer jumping), each launched exactly as a tournament chunk launches
 * it.  The host packs the draws into the path's device layout — groups of eight 16-bit draws per 16 bytes, a last partial group
 * right-aligned in the top halves behind the draws before it; path 1 group-major over n_sh rounded up to 64, path 2 one row of
 * ceil((S - 1) / 8) + 1 groups per shuffle — and reads the blocked result back as fk_tournament_run does for `perms`.
 * Precondition, checked on the host before anything is launched: draws[sh][n] <= S - 1 - n (the kernels index LDS with the draws).
 * FK_ERR_ARG, with perms untouched: S outside [1, 65535], n_sh < 1, a path other than 1 or 2, path 2 at an S beyond the chain-free
 * kernel's LDS reach (14 S bytes > the launch limit less 1 KiB), a draw beyond its bound. */
int fk_debug_perm_from_draws(fk_ctx *ctx, int32_t S, int64_t n_sh, const uint16_t *draws, int32_t path, int32_t *perms);

/* The performance stage's joint deterministic-batch bootstrap (analysis/performance.py: _BootstrapRangeWriter.__call__ :838-928,
 * _reduce_bootstrap_ranges :1013-1111; _joint_batch_resampling :715-833) for replicates [replicate_begin, replicate_end).
 * Inputs: n_k player counts in the caller's (ascending) order; per player count i its k = ks[i], its ELIGIBLE batches
 * batch_counts[i] (the caller has projected to complete-support strategies and dropped every batch in which one of them has no
 * exposure, :861-868) and two row-major int64 [batch_counts[i]][S] matrices wins[i] / exposures[i] (raw_wins,
 * raw_player_game_exposures); S strategy columns in ascending strategy id; top_n in [0, S]; delta (screening.delta_across_k);
 * n_controls column indices.  Per replicate r and player count: stream (purpose 400, root_seed, k, replicate_index r), B_k draws
 * in [0, B_k) (B_k = 1 draws nothing), exact int64 resampled totals, score[r][s] = (sum over k of (double)wins / (double)exposures
 * - 1.0 / k) / n_k as separate IEEE operations, in the given order of player counts.
 * Outputs (caller-owned host memory):
 *   scores               float64 [replicate_end - replicate_begin][S], nullable: the payload of the range writer's .npy
 *   rank_sum, rank_square_sum, top_counts, shortlist_counts   int64 [S], required, overwritten: over the call's replicates, rank =
 *                        position in lexsort((strategies, -score)) from 1 (ties: ascending column), top = rank <= top_n,
 *                        shortlist = score >= max(score) - delta
 *   contrast_sum, contrast_square_sum   float64 [n_controls][S], IN / OUT: the call continues the sums it is given with
 *                        d = score[r][s] - score[r][controls[c]]; sum += d; square_sum += d * d, replicate by replicate in ascending
 *                        order, so a range split over several calls gives the bits of one call.  Nullable when n_controls = 0.
 * A resampled exposure total <= 0 (the reference's ValueError), a negative count or one whose total could pass 2^63 returns
 * FK_ERR_ARG.  Option "bootstrap_block" > 0 caps the replicates of one device block (default: from the workspace budget); results do
 * not depend on it. */
int fk_performance_bootstrap(fk_ctx *ctx, uint64_t root_seed, int32_t n_k, const int32_t *ks, const int64_t *batch_counts,
                             const int64_t *const *wins, const int64_t *const *exposures, int32_t S, int64_t replicate_begin,
                             int64_t replicate_end, int32_t top_n, double delta, int32_t n_controls, const int32_t *controls,
                             double *scores, int64_t *rank_sum, int64_t *rank_square_sum, int64_t *top_counts, int64_t *shortlist_counts,
                             double *contrast_sum, double *contrast_square_sum);

/* The two-root stability stage's bootstrap families (analysis/root_stability.py: _RootTopNRangeWriter.__call__ :816-906 and
 * _JointDiscrepancyRangeWriter.__call__ :1201-1311, reduced by _root_bootstrap_top_n_inclusion :909-992 and
 * _joint_discrepancy_bootstrap :1314-1426) for replicates [replicate_begin, replicate_end).
 * Inputs: roots[2] = (a, b), a < b; n_k player counts ks[] in the caller's (ascending) order with their weights[] (_k_weights
 * :501-513); 2 * n_k cells in (root, k) order — root a's player counts, then root b's — each with its ELIGIBLE batches
 * batch_counts[cell] (every batch in which each strategy has an exposure) and two row-major int64 [batch_counts[cell]][S] matrices
 * wins[cell] / exposures[cell]; S strategy columns in ascending strategy id, the same for every cell; top_n in [0, S].
 * observed / expected: float64 [n_k][S] (raw_difference / expected_mcse of the by-k discrepancy rows), observed_across /
 * expected_across: float64 [S]; the four are nullable AS A GROUP (top-N family only).  observed must be finite; a column whose
 * expected is NaN or <= 0 is no estimand.
 * Per replicate r and cell: stream (purpose 401, root, k, replicate_index r), B draws in [0, B) (B = 1 draws nothing), exact int64
 * resampled totals, rate = (double)wins / (double)exposures - 1.0 / k.  Both families use the same streams.
 * Outputs (caller-owned host memory):
 *   top_counts   int64 [2][S], required, overwritten: per root the replicates in which the column is among the first top_n of
 *                lexsort((strategies, -score)), score = 0.0 then score += weights[i] * rate for each player count in order
 *   maxima       float64 [replicate_end - replicate_begin], required with the group of four: per replicate the maximum of
 *                |(rate_a - rate_b - observed[k]) / expected[k]| over the valid columns of every k and
 *                |(sum_k weights[k] * (rate_a - rate_b) - observed_across) / expected_across| over the valid columns (the sum runs
 *                0 + t_1 + t_2 ... left to right); 0.0 when nothing is valid.  Without the group it is filled with 0.0 when given.
 *   membership   uint8 [replicate_end - replicate_begin][2][S], nullable: the payload of the top-N range writer's .npy
 * Every operation is a separate IEEE operation.  Counts are integers and maxima are per replicate, so a range split over several
 * calls or device blocks gives the bits of one call.  Bad shapes, roots not ascending, a non-finite weight or observed, a resampled
 * exposure total <= 0 (the reference's ValueError), a negative count or one whose total could pass 2^63 return FK_ERR_ARG.  Option
 * "bootstrap_block" as for fk_performance_bootstrap. */
int fk_root_stability_bootstrap(fk_ctx *ctx, const uint64_t *roots, int32_t n_k, const int32_t *ks, const int64_t *batch_counts,
                                const int64_t *const *wins, const int64_t *const *exposures, int32_t S, const double *weights,
                                int64_t replicate_begin, int64_t replicate_end, int32_t top_n, const double *observed,
                                const double *expected, const double *observed_across, const double *expected_across,
                                int64_t *top_counts, double *maxima, uint8_t *membership);

/* Exact power of the round robin's two-sided score test, the quantity the reference's power plan scans block sizes by
 * (analysis/h2h_schedule.py: implemented_score_test_power :324-358 over _fixed_first_count_boundary_arrays :273-295, scanned by
 * _minimum_block_games :393-420).  Per cell: n completed games per order, X1 ~ Bin(n, q_ab) and X2 ~ Bin(n, q_ba) independent;
 * power[i] = sum over c1 = 0 .. n of pmf(X1 = c1) * [ P(X2 <= lower(c1)) + P(X2 >= upper(c1)) ], clamped to [0, 1], where lower / upper are
 * the reference's closed-form rejecting count boundaries at critical_value = norm.isf(alpha / 2): the roots of the quadratic in count2,
 * ceil - 1 and floor + 1 of them, clipped to [-1, n] and [0, n + 1], -1 at c1 = 0 and n + 1 at c1 = n.  The boundaries are NumPy's
 * integer for integer (the same fp64 operations in the same order, never fused); the probabilities are fp64 from a log-factorial table
 * the context keeps, the lower tail a prefix sum and the upper tail a suffix sum of the probability masses.  The conditional-Fisher
 * cross-check the reference adds at n <= 64 is not made.  A cell's result does not depend on the other cells or on their order.
 * Cells of n <= FK_POWER_LDS_MAX_N keep their tails in LDS, larger ones in a workspace of the context.
 * FK_ERR_ARG, with power untouched: n < 1 or n > FK_POWER_MAX_N, a q outside (0, 1) or not finite, a critical_value that is not finite
 * and positive, n_cells < 0, a null pointer with n_cells > 0.  n_cells = 0 succeeds and touches nothing. */
#define FK_POWER_MAX_N 1048576
#define FK_POWER_LDS_MAX_N 3071
typedef struct fk_power_cell {
    int32_t n;        /* completed games per order */
    int32_t reserved; /* 0 */
    double q_ab;      /* P(seat 1 wins) in order a-b */
    double q_ba;      /* ... and in order b-a */
} fk_power_cell;
int fk_score_power_scan(fk_ctx *ctx, const fk_power_cell *cells, int64_t n_cells, double critical_value, double *power);

/* The performance stage's per-k point estimates from one player count's batch matrix (analysis/performance.py:
 * _estimate_one_k_matrix :425-542), as far as they are sums over batches.
 * Inputs: k (the player count, named in the messages); four row-major int64 [B][S] matrices wins / exposures / completed / safety
 * (raw_wins, raw_player_game_exposures, raw_completed_player_game_exposures, raw_safety_limit_player_game_exposures) of ALL B batches in
 * ascending batch id, S strategy columns in ascending strategy id.  The matrices are unprojected: a cell without an exposure is allowed
 * and leaves the float sums, as the reference's `exposures > 0` mask does.
 * Outputs (caller-owned host memory, [S] each, all required):
 *   total_wins, total_exposures, total_completed, total_safety   int64 column sums; total_losses = total_exposures - total_wins
 *   positive_batches   int64: rows with exposures > 0 (raw_batches)
 *   rate_sum           float64: np.add.reduce of r_b = (double)wins / (double)exposures over the positive rows in ascending batch order
 *   ssd                float64: np.add.reduce of (r_b - mean) * (r_b - mean), mean = rate_sum / positive_batches: what
 *                      np.std(rates, ddof = 1) sums.  The caller finishes batch_mcse = sqrt(ssd / (count - 1)) / sqrt(count), the t
 *                      quantile and the Wilson interval (S values each; farkle_ii_amd/performance.py: by_k_frame).
 * Both float sums run in NumPy's order over the compacted contiguous vector (csrc/fk_performance.h: np_add_reduce: buffers of 8 192,
 * the pairwise tree down to blocks of 128, eight accumulators per block), every operation a separate IEEE operation, so the caller's
 * mcse is the reference's bit for bit.  No result depends on the launch shape (option "performance_grid" > 0 caps the workgroups).
 * FK_ERR_ARG before any device work, with the outputs untouched: k < 1, B < 1 or B > 2^31 - 1, S outside [1, 2^24], a null pointer, a
 * negative count, wins > completed, exposures != completed + safety, a column total beyond 2^62, a column whose total exposure is <= 0
 * (the reference's ValueError "strategies have no positive exposure support"). */
int fk_performance_by_k(fk_ctx *ctx, int32_t k, int64_t B, int32_t S, const int64_t *wins, const int64_t *exposures,
                        const int64_t *completed, const int64_t *safety, int64_t *total_wins, int64_t *total_exposures,
                        int64_t *total_completed, int64_t *total_safety, int64_t *total_losses, int64_t *positive_batches,
                        double *rate_sum, double *ssd);

/* The performance stage's across-k estimates of the complete-support strategies (analysis/performance.py: _across_k_estimates
 * :575-687, _pareto_membership :547-572).
 * Inputs: n rows in ascending strategy id, d required player counts (1 <= d <= 16) in the caller's order; two row-major float64 [n][d]
 * arrays: deltas (chance_delta per player count) and variances (the caller's batch_mcse ** 2, squared on the host as the reference
 * squares it — Python's float power, i.e. libm's pow, which differs from the IEEE product in about one value in 1 200 — NaN where a
 * column has fewer than two positive batches).
 * Outputs (caller-owned host memory, [n] each, all required):
 *   delta_sum, variance_sum   float64: np.add.reduce over the row's d elements (the caller divides: equal_k_score = delta_sum / d,
 *                             equal_k_mcse = sqrt(variance_sum / d^2)); d = 8 is where NumPy's eight accumulators start
 *   minimum, worst_index      float64, int32: the row's smallest delta and its first position (np.argmin)
 *   pareto_member             uint8: 1 unless another row is >= in every coordinate and > in at least one.  Equal rows do not dominate
 *                             each other.  This is the set the reference's incremental frontier ends with.
 *   leader_row                one int32: the smallest row whose minimum lies within 1e-15 of the largest minimum
 *                             (np.isclose(rtol = 0, atol = 1e-15)): the maximin leader
 * Every float operation is a separate IEEE operation; no result depends on the launch shape (option "performance_grid").
 * FK_ERR_ARG before any device work, with the outputs untouched: n < 1 or n > 2^24, d outside [1, 16], a null pointer, a delta that is
 * not finite, a variance that is negative or infinite. */
int fk_performance_across_k(fk_ctx *ctx, int32_t n, int32_t d, const double *deltas, const double *variances, double *delta_sum,
                            double *variance_sum, double *minimum, int32_t *worst_index, uint8_t *pareto_member, int32_t *leader_row);

/* The two-root stability stage's estimates over row windows of its cells, as far as they are sums over batches
 * (analysis/root_stability.py: _estimate_matrix_cells :411-433, which _scope_estimates, _matched_count_convergence :1429-1513 and
 * _half_drift :1516-1628 call for the full cells, for prefixes and for halves).  One call takes all windows of a stage.
 * Inputs: n_cells cells (1 to FK_ROOT_WINDOW_MAX_CELLS), each with batch_counts[cell] rows and four row-major int64
 * [batch_counts[cell]][S] matrices wins / exposures / completed / safety, unprojected, as fk_performance_by_k takes them; S strategy
 * columns, the same for every cell.  windows: int64 [n_windows][4] = (cell, row_begin, row_end, pairwise_begin) per window: rows
 * [row_begin, row_end) of the cell; pairwise_begin in [0, S] is the first column whose float sums take NumPy's pairwise order, because
 * the reference's column chunking (chunk = max(1, min(S, max_bytes // max(1, rows * 57)))) leaves it in a chunk of width 1
 * (farkle_ii_amd/root_stability.py: window_pairwise_begin).  Windows may repeat and overlap in any way.
 * Outputs (caller-owned host memory, both required):
 *   totals   int64 [n_windows][6][S]: the column sums of wins, exposures, completed, safety; losses = exposures - wins; positive_batches
 *            = rows with exposures > 0
 *   sums     float64 [n_windows][3][S]: sum(w * w), sum(w * e), sum(e * e) over the window's rows, w and e the row's counts as doubles
 *            (a row without an exposure adds 0.0).  Columns below pairwise_begin: 0.0, then one addition per row in ascending row order
 *            (np.sum(axis=0) over a chunk of two or more columns).  Columns from pairwise_begin: np.add.reduce over the window's rows as a
 *            vector (csrc/fk_performance.h: np_add_reduce).  Every product and every addition is a separate IEEE operation.
 * Windows of one cell with one row_begin share one pass over the rows (snapshots of the running sums), which changes no bit.  No result
 * depends on the launch shape (option "root_windows_grid" > 0 caps the workgroups).
 * FK_ERR_ARG before any device work, with the outputs untouched: a null pointer, n_cells outside [1, FK_ROOT_WINDOW_MAX_CELLS], n_windows
 * < 1, S outside [1, 2^24], a cell with B < 1 or B > 2^31 - 1, a window of an unknown cell, empty or reaching beyond its cell,
 * pairwise_begin outside [0, S], a negative count, wins > completed, exposures != completed + safety, a column total of a cell beyond 2^62,
 * a window in which some column's total exposure is <= 0 (the reference's ValueError "root stability scope contains a strategy without
 * positive exposure"). */
#define FK_ROOT_WINDOW_MAX_CELLS 256
int fk_root_window_estimates(fk_ctx *ctx, int32_t n_cells, const int64_t *batch_counts, const int64_t *const *wins,
                             const int64_t *const *exposures, const int64_t *const *completed, const int64_t *const *safety, int32_t S,
                             int64_t n_windows, const int64_t *windows, int64_t *totals, double *sums);

#ifdef __cplusplus
}
#endif
#endif
