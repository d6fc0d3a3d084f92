// farkle_hip.hip — host side of the C-ABI (include/farkle_hip.h) of the Farkle simulation engine: context, device
// buffers, launch planning and the extern "C" entry points.  The kernels are in fk_kernels.h, the per-roll device
// functions in fk_device.h.  Per chunk of work, on the context's stream: memset -> fk_perm_kernel ->
// fk_class_count_kernel + fk_seed_kernel -> fk_play_kernel (-> fk_finalize_tally), one host sync at the end.
//
// No MFMA (integer/table work), no CPU fallback.
#include "fk_kernels.h" // device side: every kernel of the engine (pulls in farkle_hip.h, fk_device.h, hip_runtime.h)
#include "fk_shard_writer.h" // host side: column images -> row-shard Parquet files
#include "fk_perm_wave.h"    // device side: a shuffle's Fisher-Yates draws by a whole wave (small launches)
#include "fk_row_columns_seats.h" // device side: column images with one thread per (game, seat)
#include "fk_matchups.h"      // device side: RNG-diagnostics matchup family (key post-pass, grouped lag reduce)
#include "fk_game_stats.h"    // device side: game-stats stage (game-record pass, per-strategy LDS histogram gather)
#include "fk_rare_events.h"   // device side: rare-event game list (ordered stream compaction), second-highest-score histograms
#include "fk_bootstrap.h"     // device side: performance stage's joint batch bootstrap (draws, integer product, ranks, contrasts)
#include "fk_root_stability.h" // device side: two-root stability stage's bootstrap families (rates of both roots, maxima, top-N membership)
#include "fk_seat_analysis.h"  // device side: seat-analysis stage (per-seat counts from rec0, mirrored-pair sort-and-segment reduce)
#include "fk_trace.h"          // device side: roll-level game trace (its own table-free game loop, events at scanned offsets)
#include "fk_census.h"         // device side: roll census (the trace's game loop, counting instead of recording)
#include "fk_round_robin.h"    // device side: head-to-head round robin (window tables by unranking, generation planner, apply, summary)
#include "fk_rr_inference.h"   // device side: round-robin inference (resident pair counts, score test, intervals, Holm, decision classes)
#include "fk_rr_root_diagnostics.h" // device side: the inference per kept root and the cross-root agreement
#include "fk_dominance.h"      // device side: dominance graphs of a round robin (bit matrices, closure, components, fronts, cycles, extremes)
#include "fk_agreement.h"      // device side: method agreement of a round robin (pair codes and their counts, Kendall's pair counts)
#include "fk_power_plan.h"     // device side: exact power of the round robin's score test per (sample size, scenario) cell
#include "fk_performance.h"    // device side: performance stage's point estimates (by-k column sums in NumPy's order, across-k sums, Pareto front, maximin)
#include "fk_root_windows.h"   // device side: two-root stability stage's window estimates (sequential column walk with snapshots, NumPy's pairwise order for width-1 chunks)
#include "fk_plan.h"           // host side: the game kernel's instance table and launch planner
#include "fk_layouts.h"        // host side: the composite device buffers' layouts
#include "fk_buffers.h"        // host side: the typed, owning device buffer and the named buffer groups of the analysis entries

#include <dlfcn.h>
#include <rccl/rccl.h> // TYPES ONLY (ncclConfig_t, result codes): the library itself is bound with dlopen on first use
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <memory>
#include <mutex>
#include <sys/mman.h>
#include <unordered_map>
#include <utility>
#include <thread>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

using namespace fk;
static_assert(fkl::GAME_COUNTS == fkg::N_COUNTS, "fk_layouts.h states the game-stats count columns on its own");

// ========================================================================================
// host side
// ========================================================================================
constexpr int FK_ROWS_EVENTS = 4; // completion events of async rows calls: a ring (a caller may have this many calls' images not yet awaited)

// Everything a chunk's preparation (permutations, schedule, seat seeding) writes and its game kernel reads.  There are two
// sets: the next chunk (of this call, or — after fk_tournament_hint_next — of the next call) is prepared into the other set
// around the game kernel of the current one (option "pipeline", default 1).  Its permutations run in front of that game
// kernel on the main stream: they want most of a CU's LDS, which the resident persistent game kernel holds (on the side
// stream they only started when it ended, with the seeding queued behind them).  Its schedule and seat seeding go to a
// low-priority stream; their kernels allocate ~1 KB of LDS per block, so they are placed as the game kernel's blocks retire,
// i.e. they fill its drain tail.  Measured (rocprofv3 traces + tools/time_pipeline.py, round 2): 10.33 -> 10.16 ms per
// config-2 step, 193.4 -> 191.6 ms per config-3 step.  Running the seeding BESIDE the game kernel instead (an LDS-free
// seed kernel) is zero-sum — both are VALU-issue bound: game kernel 178 -> 184 ms while a 6 ms seeding ran beside it — and
// stalled one run by 120 ms per step behind the low-priority queue: not done.
struct ChunkDesc {
    uint64_t epoch = 0, root = 0, sh0 = 0; // strategy-table upload epoch, root seed, first shuffle
    uint32_t n_sh = 0, S = 0, k = 0, state_dw = 0, sched = 0, slots = 0;
    bool operator==(const ChunkDesc &o) const {
        return epoch == o.epoch && root == o.root && sh0 == o.sh0 && n_sh == o.n_sh && S == o.S && k == o.k && state_dw == o.state_dw &&
               sched == o.sched && slots == o.slots;
    }
};

struct ChunkSet {
    Dev<uint16_t> perm, seat_idx;
    Dev<uint8_t> draws; // a split launch's draws (DrawLayout: uint4 groups, read as 16-bit values by fk_perm_block_kernel); free again after the
                        // permutations, the post-passes keep the chunk's inverse permutations (16-bit) in it
    uint4 *draw_groups() const { return draws.as<uint4>(); }
    uint16_t *draws16() const { return draws.as<uint16_t>(); }
    Dev<uint32_t> state, order, classes;
    Dev<uint4> inc, pools;
    Dev<uint8_t> misc; // 512 bytes, zeroed per chunk: the words below
    uint32_t *ticket() const { return misc.as<uint32_t>(0); }      // ticket counter (hammered by atomics)
    int32_t *err() const { return misc.as<int32_t>(16); }          // error record of the game kernel
    ull *hcount() const { return misc.as<ull>(128); }              // (measuring build) six hand-over counts
    uint32_t *sched_ctr() const { return misc.as<uint32_t>(256); } // schedule class cursors of the seed kernel
    Dev<DevBlock> blocks;                 // batched H2H: the pass's block table ...
    Dev<uint32_t> game_block, game_row;   // ... and game -> block / table-row maps
    hipEvent_t ready = nullptr;                       // recorded behind the preparation kernels
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; // permutation begin / end, seeding begin / end (timing)
    bool prepared = false;
    bool side = false; // prepared on the side stream: its event intervals include waiting behind a game kernel
    ChunkDesc desc;
    SeedArgs sa{}; // the prepared chunk's buffers as the kernels see them
};

// fk_tournament_run_game_stats: host pointers of the request (histogram rows of rounds_bins / margin_bins int64 each)
struct GameStatsReq {
    int64_t rare_target;
    uint32_t rounds_bins, margin_bins;
    int64_t *s_counts, *s_rounds, *s_runner, *s_spread; // [S][4], [S][rounds_bins], [S][margin_bins] x 2
    int64_t *g_counts, *g_rounds, *g_runner;           // [4], [rounds_bins], [margin_bins]
    int64_t spill_capacity;
    int64_t *spill_count; // entries the call produced (also when they did not fit)
    int32_t *spill;       // [spill_capacity][3]
};

// fk_tournament_run_rare_events (beside the GameStatsReq of the same call)
struct RareReq {
    uint32_t second_bins;
    int64_t *s_second, *g_second; // [S][second_bins], [second_bins]
    fkre::Thresholds thr;
    bool events; // false: the histograms-only call
    int64_t event_capacity;
    int64_t *event_count; // events the call produced (also when they did not fit)
    uint32_t *event_head; // [event_capacity][4]
    uint16_t *event_seats; // [event_capacity][k]
};

// fk_tournament_run_seat_counts: host pointers of the request
struct SeatReq {
    int64_t *counts;          // [n_batches][S][k][3]
    const uint16_t *id_rank;  // null: no mirrored pairs
    int64_t pair_capacity;
    int64_t *pair_count;      // pairs the call produced (also when they did not fit)
    uint16_t *pair_index;     // [pair_capacity][2]
    int64_t *pair_sums;       // [pair_capacity][6]
};

struct LagReq { // fk_tournament_run_lags: host pointers of the request
    const int32_t *lags;
    int32_t n_lags, max_lag;
    int64_t *sums;
    uint16_t *head, *tail;
    // fk_tournament_run_matchups (null otherwise): the caller's strategy IDs, max_players, and the per-game records of the range
    const int32_t *ids = nullptr;
    int32_t max_players = 0;
    uint64_t *m_digest = nullptr;
    uint16_t *m_seats = nullptr, *m_rounds = nullptr;
};

// One tournament call, as its entry point has checked it: every fk_tournament_run* entry fills one on its stack and the call path
// (tournament_call, tournament_run_impl) reads it by const reference.  Members left out are null.
struct TournamentCall {
    const fk_strategy *strategies;
    int32_t S, k;
    uint64_t root_seed, shuffle_begin, shuffle_end;
    uint32_t shuffles_per_batch;
    int32_t target_score, max_rounds;
    const fk_override *ov;
    int32_t n_ov;
    int64_t *tally;
    void *rows;          // AoS rows, or (with columns_ids) per-shuffle column images
    int32_t *perms;
    int64_t *seat_stats;
    double *seat_ratios;
    const int32_t *columns_ids;          // fk_tournament_run_columns: the strategy ids the images name
    uint32_t *shuffle_seeds, *game_seeds; // fk_tournament_run_columns_seeds: host destinations
    const LagReq *lag;
    const GameStatsReq *gstats;
    const RareReq *rare; // (with gstats)
    const SeatReq *seats;
};

struct fk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t prep_stream = nullptr; // low priority: preparation of the next chunk
    ChunkSet sets[2];
    int cur = 0;
    uint64_t table_epoch = 0;
    bool hint_valid = false;           // fk_tournament_hint_next
    uint64_t hint_begin = 0, hint_end = 0;
    int32_t hint_state = 0, pipeline = 1;
    hipDeviceProp_t prop{};
    std::string err;
    fk_timing timing{};
    std::string play_instance; // the game-kernel instance of the call's last launch (fk_last_play_instance)
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // see TimerSlot
    int32_t *err_host = nullptr;    // pinned: the error record of a call's last game kernel (read with the tally)
    hipEvent_t main_idle = nullptr; // recorded on the main stream in front of a game kernel: what a side-stream preparation waits for
    struct PendingTimer {
        float *acc;
        hipEvent_t a, b;
    };
    std::vector<PendingTimer> pending; // kernel timers recorded on the stream, read after the chunk's one sync
    Dev<uint2> strat;
    Dev<uint32_t> recs, rec0, inv, score_lut;
    Dev<ull> tally, block_out;
    Dev<uint8_t> rows, slow, discard_lut; // (discard_lut: the byte table and, behind it, the wide one)
    Dev<DevOverride> ov;
    Dev<int32_t> seatlist;
    Dev<fk_coord> coords;
    Dev<long long> stats;
    Dev<double> ratios;
    Dev<uint4> digest;
    Dev<uint8_t> seeds; // fkl::Fingerprints: the game / shuffle seeds of a rows-mode call (fk_game_seeds: its game seeds)
    Dev<uint8_t> cub;   // hipcub's scratch (FK_CUB)
    ProbeBufs dbg;
    std::vector<uint2> strat_host;   // the packed table currently resident in `strat` (uploaded once per table)
    int32_t longest_first = 1;
    int32_t blocks_per_cu = 0; // 0 = as many as fit
    int32_t max_waves = 6;     // resident waves per SIMD the launch plan may count on
    int32_t lean = -1;         // -1 auto, 0 full 17-dword seat records, 1 lean 11-dword records
    int32_t gs = -1;           // -1 / 0: LDS records whenever k of them fit a wave's share of LDS, 1: state-store instances always
    int32_t flat_handover = 1;      // 0: two-seat launches take the general hand-over (A/B, tests of the general copy of the loop nest)
    int32_t uniform_flags_opt = -1; // -1 auto (scalar-flag instance when the table allows it), 0 never
    uint32_t table_flags = 0;            // set by upload_strategies: flag bits shared by the whole table ...
    uint32_t table_mixed_flags = 0xff00u; // ... and the flag bits that differ between its strategies
    int64_t chunk_bytes = (int64_t)48 << 30;
    // The workspace budget of one buffer set is min(chunk_bytes, workspace_percent % of the memory this context can have — what is free now
    // plus what its own per-chunk buffers already hold — divided by the two sets); a call that still meets hipErrorOutOfMemory (another
    // process took the memory in between) releases its workspace, halves the budget and is replayed (round-5 finding: four ranks sharing
    // one device each sized two 48-GiB sets and rank 2 died in hipMalloc).
    int32_t workspace_percent = 80; // option "workspace_percent" (tests set it above 100 to provoke the replay)
    int64_t chunk_limit = 0;        // the replay's halved budget (0: none)
    int64_t last_budget = 0;        // the budget the last call planned with (fk_timing has no room: read through option "last_budget")
    bool oom = false;               // ensure() met hipErrorOutOfMemory
    std::vector<void *> hog;        // fk_debug_hold_memory: device memory held on purpose (tests of the budget / the replay)
    int32_t oom_replays = 0;        // how many times the last call was replayed with a smaller workspace
    int32_t batch_threshold = 0;  // 0 = auto: 8 waiting lanes up to eight seats, 12 at nine / ten, 16 at eleven / twelve (swept per k)
    int32_t use_lds_tally = -1;
    int32_t block = 0;
    int32_t hc = -1;           // hot / cold game kernel (fk_play_hc.h): -1 auto, 0 never, 1 whenever the table allows it
    Dev<uint8_t> lds_tables;   // their LDS image (fk_play_hc.h)
    Dev<uint4> cold;
    int32_t clock_stamps = 0;  // option "clock_stamps": every game-kernel block stamps s_memtime / s_memrealtime at both ends
    Dev<ull> clk;              // [grid][4] stamps of the last game kernel
    int clk_grid = 0;
    Dev<uint16_t> lag_v, lag_edge, lag_tmp; // fk_tournament_run_lags: value matrix, head / tail rows, the carry's scratch copy
    Dev<long long> lag_out;                 // ... its sums
    Dev<int32_t> lag_lags, m_ids;           // ... its lag list; fk_tournament_run_matchups: strategy IDs
    Dev<ull> m_dig;                         // ... and one chunk's game records
    Dev<uint16_t> m_seat, m_rnd;
    MatchupReduceBufs mr;
    uint64_t matchup_sort_mask = ~0ull;  // option "matchup_sort_key_mask": the bits of the digest the reduce sorts by (tests)
    Dev<uint4> g_rec;                    // fk_tournament_run_game_stats: one chunk's game records
    Dev<uint8_t> g_out;                  // ... the call's histograms + spill list (fkl::GameStatsOut)
    int64_t game_stats_window = 0;       // option "game_stats_window": > 0 caps both histogram windows (tests drive the spill path)
    Dev<uint32_t> r_sec, r_blk;          // fk_tournament_run_rare_events: one chunk's second scores; workgroup counts ...
    Dev<ull> r_base, r_out;              // ... and bases; second histograms + event total (fkl::RareOut)
    Dev<uint4> r_head;                   // the event list
    Dev<uint16_t> r_seats;
    SeatBufs sa;
    TraceBufs tr;
    CensusBufs cn;
    int64_t census_chunk_games = 0;      // option "census_chunk_games": > 0 caps the games of one census chunk (tests drive the chunk loop)
    RoundRobinBufs rr;
    int64_t rr_window_blocks = (int64_t)1 << 22; // option "rr_window_blocks": blocks of one round-robin window (even, 2 .. 2^22; scheduling only)
    RrInferenceBufs ri;
    bool ri_valid = false;               // the accumulator holds counts; what the first adding call fixed with them:
    int32_t ri_n = 0;
    uint64_t ri_begin = 0, ri_end = 0, ri_hash = 0, ri_family = 0;
    bool ri_keep_roots = false;          // option "rr_keep_roots": adding calls keep their states in RrInferenceBufs::root_states
    bool ri_untracked = false;           // the accumulator holds cells that no root slot holds (fk_rr_counts_add with the option on)
    int32_t ri_roots = 0;                // root slots in use, in arrival order, and what each was kept with:
    uint64_t ri_root_seed[FK_RR_MAX_ROOTS] = {0, 0}, ri_root_target[FK_RR_MAX_ROOTS] = {0, 0}, ri_root_cap[FK_RR_MAX_ROOTS] = {0, 0};
    DominanceBufs dm;
    AgreementBufs ag;
    int64_t agreement_grid = 0;          // option "agreement_grid": > 0 caps the pair kernel's grid lower (tests drive second trips)
    PowerPlanBufs pp;
    BootBufs boot;
    PerformanceBufs pf;
    int64_t performance_grid = 0;        // option "performance_grid": > 0 caps the workgroups of the performance kernels (tests drive the grid strides)
    RootWindowBufs rw;
    int64_t root_windows_grid = 0;       // option "root_windows_grid": > 0 caps the workgroups of the window kernels (tests drive the task strides)
    int64_t bootstrap_block = 0;         // option "bootstrap_block": > 0 caps the replicates of one device block (tests drive the block carry)
    bool ran_hc = false;       // the current tournament call launched the hot / cold kernel
    int32_t perm_split = -1;   // -1 auto, 0 one-kernel Fisher-Yates, 1 draws + serial swap chains, 2 draws + chain-free kernel
    int32_t columns_by_seat = -1; // column images: -1 one thread per (game, seat) up to sixteen seats, per game beyond; 0 per game; 1 per (game, seat)
    int32_t perm_draw_wave = -1; // the draws of a shuffle by -1: a wave up to WAVE_DRAW_MAX_SH shuffles per chunk, a thread beyond; 0: a thread; 1: a wave
    void *comm = nullptr;      // RCCL communicator (fk_comm_init), one per context / GPU
    int comm_rank = 0, comm_world = 1;
    bool comm_async = false;   // (non-blocking communicators: every RCCL call settled by polling; not used — see fk_comm_init)
    bool comm_lost = false;    // a collective failed or timed out and the communicator was aborted: reductions fail until fk_comm_init
    bool comm_timeout_set = false;    // "comm_timeout_ms" was set explicitly: the environment default no longer applies
    int32_t comm_timeout_ms = 120000; // option "comm_timeout_ms" (FK_COMM_TIMEOUT_MS): deadline of communicator creation and of each
                                      // collective; 0 = the blocking calls of round 3 (no deadline)
    Dev<uint8_t> comm_buf;
    // resident tally (option "resident_tally"): every tournament call adds its [n_batches][S][26] tally to this device
    // accumulator; fk_tally_resident_reduce sums it over the communicator on the device (the tally never leaves HBM before
    // the reduce; one D2H, on the root)
    // rows mode: the device row buffer exists twice and a copy stream moves chunk i's rows to the host while chunk i + 1 plays
    Dev<uint8_t> rows_alt;
    // fk_tournament_run_columns: the rows buffer receives per-shuffle column images (fk_row_columns_kernel); the strategy ids they name
    Dev<int32_t> ids;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_rows[2] = {nullptr, nullptr}, ev_copy[2] = {nullptr, nullptr};
    // option "rows_async": a rows call returns when its last copy to the host is QUEUED, not done; fk_rows_wait(slot) waits for it.  The caller
    // (farkle run: two page-locked buffers) then starts the next launch group at once, whose game kernel runs beside that copy.
    int32_t rows_async = 0;
    hipEvent_t ev_call_copy[FK_ROWS_EVENTS] = {};
    uint32_t rows_calls = 0;      // rows calls made in async mode: call n records ev_call_copy[n % FK_ROWS_EVENTS]
    // The mailbox: page-locked host memory the device STORES small results into (tallies, error records, game seeds) while a rows DMA
    // is in flight — a copy-engine transfer would queue behind those 256 MB and the call would wait for them after all (measured: an
    // async call took exactly as long as a waiting one until its tally left this way).
    uint8_t *mail = nullptr;
    size_t mail_cap = 0, mail_used = 0;
    struct Letter { void *dst; size_t off, bytes; };
    std::vector<Letter> letters;
    int32_t last_rows_event = -1; // ... and this is the slot of the last one (option "rows_event")
    int64_t rows_chunk_games = 4000000; // rows mode plays in chunks of about this many games (overlap granularity)
    int32_t resident = 0;
    size_t last_tally_bytes = 0; // bytes of the last successful tournament call's tally in `tally`
    Dev<ull> acc;
    size_t acc_n = 0;
};

#define CSET(c) ((c)->sets[(c)->cur])

namespace {

int fail(fk_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIPCHK(c, expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return fail((c), FK_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// ensure()'s slow path: a buffer that holds `cap` bytes at `p` gives them back and gets `bytes` (256 at least)
int grow(fk_ctx *c, void *&p, size_t &cap, size_t bytes) {
    if (p) HIPCHK(c, hipFree(p));
    g_device_bytes_held -= (int64_t)cap;
    p = nullptr;
    cap = 0;
    size_t want = std::max<size_t>(bytes, 256);
    const hipError_t e = hipMalloc(&p, want);
    if (e == hipErrorOutOfMemory) {
        c->oom = true;
        p = nullptr;
        (void)hipGetLastError(); // (the sticky error would fail the next, unrelated call)
        return fail(c, FK_ERR_HIP, "hipMalloc(%zu bytes) failed: out of memory", want);
    }
    HIPCHK(c, e);
    cap = want;
    g_device_bytes_held += (int64_t)want;
    return FK_OK;
}

// room for `count` elements
template <class T>
inline int ensure(fk_ctx *c, Dev<T> &b, size_t count) {
    if (count * sizeof(T) <= b.cap) return FK_OK;
    void *p = b.p;
    const int rc = grow(c, p, b.cap, count * sizeof(T));
    b.p = static_cast<T *>(p);
    return rc;
}

// ensure() for (buffer, count) pairs in their order; the first failure ends it
template <class T, class... Rest>
int ensure_all(fk_ctx *c, Dev<T> &b, size_t count, Rest &&...rest) {
    if (const int rc = ensure(c, b, count)) return rc;
    if constexpr (sizeof...(rest) > 0) return ensure_all(c, rest...);
    else return FK_OK;
}

// per-chunk buffers: what workspace_budget counts as this context's own and release_workspace gives back
template <class F>
static void for_workspace_buffers(fk_ctx *c, F f) {
    for (auto &cs : c->sets) {
        f(cs.perm), f(cs.draws), f(cs.state), f(cs.inc), f(cs.seat_idx), f(cs.order), f(cs.classes), f(cs.misc), f(cs.pools), f(cs.blocks);
        f(cs.game_block), f(cs.game_row);
    }
    // (only buffers that every call sizes and ensures per chunk: c->slow — the patience table upload_strategies fills once per TABLE — is not one)
    f(c->recs), f(c->rec0), f(c->rows), f(c->rows_alt), f(c->digest), f(c->inv), f(c->lag_v), f(c->lag_tmp), f(c->cn.ws);
}

// bytes one buffer set of a call may plan for (see fk_ctx::workspace_percent)
static int64_t workspace_budget(fk_ctx *c) {
    int64_t budget = c->chunk_bytes;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        size_t held = 0;
        for_workspace_buffers(c, [&](auto &b) { held += b.cap; });
        const double have = (double)free_b + (double)held;
        budget = std::min<int64_t>(budget, std::max<int64_t>((int64_t)(have * (double)c->workspace_percent / 100.0 / 2.0), (int64_t)32 << 20));
    } else {
        (void)hipGetLastError();
    }
    if (c->chunk_limit > 0) budget = std::min(budget, c->chunk_limit);
    c->last_budget = budget;
    return budget;
}

static void release_workspace(fk_ctx *c) {
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    for_workspace_buffers(c, [](auto &b) { b.release(); });
    for (auto &cs : c->sets) cs.prepared = false;
    c->hint_valid = false;
}

uint2 pack_strategy(const fk_strategy &s) {
    uint32_t bits = (uint32_t)(uint8_t)(int8_t)s.dice_threshold;
    if (s.smart_five) bits |= SF_SMART_FIVE;
    if (s.smart_one) bits |= SF_SMART_ONE;
    if (s.consider_score) bits |= SF_CONSIDER_SCORE;
    if (s.consider_dice) bits |= SF_CONSIDER_DICE;
    if (s.require_both) bits |= SF_REQUIRE_BOTH;
    if (s.auto_hot_dice) bits |= SF_AUTO_HOT;
    if (s.run_up_score) bits |= SF_RUN_UP;
    if (s.favor_score) bits |= SF_FAVOR_SCORE;
    return make_uint2((uint32_t)ceil_div50(s.score_threshold), bits); // the kernels compare turn scores in units of 50 (fk_device.h)
}

int validate_strategies(fk_ctx *c, const fk_strategy *s, int64_t S) {
    for (int64_t i = 0; i < S; ++i) {
        if (s[i].dice_threshold < -128 || s[i].dice_threshold > 127)
            return fail(c, FK_ERR_ARG, "strategy %lld: dice_threshold %d outside [-128, 127]", (long long)i, s[i].dice_threshold);
        if (s[i].smart_one && !s[i].smart_five) // strategies.py:198
            return fail(c, FK_ERR_ARG, "strategy %lld: smart_one requires smart_five", (long long)i);
        if (s[i].require_both && !(s[i].consider_score && s[i].consider_dice)) // strategies.py:202
            return fail(c, FK_ERR_ARG, "strategy %lld: require_both requires consider_score and consider_dice", (long long)i);
    }
    return FK_OK;
}

// patience class of a strategy (upload_strategies explains it)
uint8_t patience_of(const fk_strategy &s) {
    if (!(s.consider_dice && (s.require_both || !s.consider_score))) return 0;
    return s.dice_threshold < 1 ? 3 : s.dice_threshold == 1 ? 2 : s.dice_threshold == 2 ? 1 : 0;
}

// The packed table (+ the per-strategy patience of the longest-first schedule) goes to the device once per TABLE: a call
// whose table equals the resident one uploads nothing.
int upload_strategies(fk_ctx *c, const fk_strategy *s, int64_t S) {
    int rc = validate_strategies(c, s, S);
    if (rc) return rc;
    std::vector<uint2> packed((size_t)S);
    for (int64_t i = 0; i < S; ++i) packed[(size_t)i] = pack_strategy(s[i]);
    if (packed.size() == c->strat_host.size() && memcmp(packed.data(), c->strat_host.data(), packed.size() * sizeof(uint2)) == 0)
        return FK_OK;
    c->strat_host.clear();
    c->table_epoch += 1; // anything prepared for the previous table is void
    for (auto &cs : c->sets) cs.prepared = false;
    if (c->prep_stream) HIPCHK(c, hipStreamSynchronize(c->prep_stream));
    rc = ensure(c, c->strat, (size_t)S);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->strat.p, packed.data(), sizeof(uint2) * (size_t)S, hipMemcpyHostToDevice, c->stream));
    uint32_t f_and = 0xff00u, f_or = 0u;
    for (int64_t i = 0; i < S; ++i) {
        f_and &= packed[(size_t)i].y;
        f_or |= packed[(size_t)i].y & 0xff00u;
    }
    c->table_mixed_flags = f_or & ~f_and;
    c->table_flags = f_and;
    // Patience of a strategy, for the longest-first schedule only (fk_kernels.h, schedule_class).  It never banks
    // voluntarily outside the final round (3) iff should_continue's threshold term is always true: dice are considered
    // with dice_threshold < 1 (dice_left >= 1 always exceeds it) and the score threshold cannot veto (require_both, or
    // score not considered).  With the same "either condition keeps rolling" rule and dice_threshold 1 / 2 it rolls
    // down to one / two dice before it may bank (2 / 1).
    std::vector<uint8_t> patience((size_t)S, 0);
    for (int64_t i = 0; i < S; ++i) patience[(size_t)i] = patience_of(s[i]);
    rc = ensure(c, c->slow, patience.size());
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->slow.p, patience.data(), patience.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // host vectors go out of scope
    c->strat_host.swap(packed);
    return FK_OK;
}

SeedPool seed_prefix(uint32_t purpose, uint64_t root_seed, uint64_t k) {
    SeedPool p;
    ss_begin(p, 2u /* RNG_SCHEME_VERSION */, purpose, (uint32_t)root_seed, (uint32_t)(root_seed >> 32));
    ss_absorb64(p, k);
    return p;
}

// the options and the device figure the launch plan (fk_plan.h) depends on
PlanKnobs plan_knobs(const fk_ctx *c) {
    PlanKnobs kn;
    kn.cus = c->prop.multiProcessorCount;
    kn.max_waves = c->max_waves;
    kn.blocks_per_cu = c->blocks_per_cu;
    kn.block = c->block;
    kn.lean = c->lean;
    kn.gs = c->gs;
    kn.hc = c->hc;
    kn.use_lds_tally = c->use_lds_tally;
    return kn;
}

// LDS image of the score / discard tables (fk_play_hc.h), from the same __host__ __device__ functions that build the
// global tables (fk_device.h: lt_build_image — also what tests/native/device_header_host_check.hip checks the LDS path on)
std::vector<uint8_t> build_lds_tables() {
    std::vector<uint8_t> img(LT_BYTES, 0);
    lt_build_image(img.data());
    return img;
}

constexpr size_t LDS_LIMIT = 160 * 1024; // the dynamic LDS a game-kernel launch may ask for
static_assert(LDS_LIMIT == PLAN_LDS_LIMIT, "the launch plan (fk_plan.h) seats blocks in the LDS a launch may ask for");

constexpr uint32_t MIXED_ALL = 0xff00u, MIXED_NONE = 0u, MIXED_RB_FAV = SF_REQUIRE_BOTH | SF_FAVOR_SCORE;
constexpr uint32_t MIXED_FORMS[3] = {MIXED_NONE, MIXED_RB_FAV, MIXED_ALL};
// the narrowest form whose MIXED set covers the flags that actually vary in this table
inline int mixed_form(uint32_t varying) { return varying == MIXED_NONE ? 0 : (varying & ~MIXED_RB_FAV) == 0u ? 1 : 2; }

// One game-kernel instance on the stream: a persistent grid of at most p.grid blocks.
template <auto KERNEL>
hipError_t launch_instance(const LaunchPlan &p, const PlayArgs &a, hipStream_t s, const std::string &name) {
    static int configured_dev = -1; // the dynamic-LDS ceiling of an instance is raised once per device, not per launch
    static size_t occ_lds = ~(size_t)0;
    static int occ_blocks = 0;
    const void *fn = reinterpret_cast<const void *>(KERNEL);
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (configured_dev != dev) { // a context on another device of this process: the attribute and the occupancy are per device
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT);
        if (e != hipSuccess) return e;
        configured_dev = dev;
        occ_lds = ~(size_t)0;
    }
    const size_t lds = std::max<size_t>(p.lds, 16);
    if (occ_lds != lds) { // resident blocks per CU as the runtime counts them (registers, LDS, wave slots)
        int nb = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, p.block, lds);
        if (e != hipSuccess) return e;
        occ_blocks = std::max(nb, 1);
        occ_lds = lds;
    }
    // blocks beyond the resident ones would only queue behind them
    const int grid = std::min(p.grid, occ_blocks * p.cus);
    p.launched_grid = grid;
    p.instance = name.c_str();
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3((unsigned)p.block), lds, s, a);
    return hipGetLastError();
}

// an instance as the compiler spells its template (fk_last_play_instance; tests/kernel_instances.py parses it)
std::string instance_name(const PlayRow &r, uint32_t mixed) {
    auto tf = [](bool v) { return v ? "true" : "false"; };
    char b[96];
    if (r.hc) snprintf(b, sizeof(b), "fk_play_hc_kernel<%d, %uu, %s, %d, %d, %s, %s, %d>", r.block, mixed, tf(r.lt), r.ki, r.wpe, tf(r.pkr), tf(r.cl), r.ns);
    else snprintf(b, sizeof(b), "fk_play_kernel<%d, %s, %d, %uu, %s, %s, %d>", r.block, tf(r.lean), r.wpe, mixed, tf(r.gs), tf(r.blk), r.kc);
    return b;
}

// row ROW of the instance table (fk_plan.h) in flag form FORM
template <int ROW, int FORM>
hipError_t launch_row(const LaunchPlan &p, const PlayArgs &a, hipStream_t s) {
    constexpr PlayRow R = PLAY_ROWS[ROW];
    constexpr uint32_t MIXED = MIXED_FORMS[FORM];
    static const std::string name = instance_name(R, MIXED);
    if constexpr (R.hc) return launch_instance<&fk_play_hc_kernel<R.block, MIXED, R.lt, R.ki, R.wpe, R.pkr, R.cl, R.ns>>(p, a, s, name);
    else return launch_instance<&fk_play_kernel<R.block, R.lean, R.wpe, MIXED, R.gs, R.blk, R.kc>>(p, a, s, name);
}

using LaunchFn = hipError_t (*)(const LaunchPlan &, const PlayArgs &, hipStream_t);
template <size_t... I>
constexpr std::array<LaunchFn, sizeof...(I)> launch_table(std::index_sequence<I...>) {
    return {{&launch_row<(int)(I / 3), (int)(I % 3)>...}};
}

// plan -> row -> instance: a plan can only name a compiled instance
hipError_t launch_play(const LaunchPlan &p, const PlayArgs &a, hipStream_t s) {
    static constexpr auto LAUNCH = launch_table(std::make_index_sequence<3 * N_PLAY_ROWS>{});
    if (p.row < 0 || p.lds > LDS_LIMIT) return hipErrorInvalidValue; // (a plan without an instance: the callers refuse it first)
    return LAUNCH[(size_t)p.row * 3 + (size_t)mixed_form(p.mixed_flags)](p, a, s);
}

// Event pairs: kernels of one chunk are enqueued back to back (no host wait between them); their timers are read
// after the stream sync that ends the chunk (collect_timers).
enum TimerSlot : int { SLOT_PERM = 0, SLOT_SEED = 2, SLOT_PLAY = 4, SLOT_CALL = 6 };

struct Timer {
    fk_ctx *c;
    float *acc;
    hipEvent_t a, b;
    Timer(fk_ctx *ctx, float *dst, int slot) : c(ctx), acc(dst), a(ctx->ev[slot]), b(ctx->ev[slot + 1]) {
        (void)hipEventRecord(a, c->stream);
    }
    void stop() {
        (void)hipEventRecord(b, c->stream);
        c->pending.push_back({acc, a, b});
    }
};

hipError_t collect_timers(fk_ctx *c) { // the stream has been synchronised
    hipError_t first = hipSuccess;
    for (const auto &t : c->pending) {
        float ms = 0.f;
        const hipError_t e = hipEventElapsedTime(&ms, t.a, t.b);
        if (e == hipSuccess) *t.acc += ms;
        else if (first == hipSuccess) first = e;
    }
    c->pending.clear();
    return first;
}

// the error record of a game kernel, once it is on the host
int report_device_error(fk_ctx *c, const int32_t *h, int64_t game_base, const char *what) {
    if (h[0] == FK_ERR_ROLL_LIMIT)
        return fail(c, FK_ERR_ROLL_LIMIT, "Turn exceeded 1000 rolls - aborting. (%s game %lld)", what,
                    (long long)(game_base + h[1]));
    if (h[0] == FK_ERR_COUNTER_OVERFLOW)
        return fail(c, FK_ERR_COUNTER_OVERFLOW, "per-seat u16 counter left its guarded range (%s game %lld)", what,
                    (long long)(game_base + h[1]));
    if (h[0] != 0) return fail(c, h[0], "device error %d (%s game %lld)", h[0], what, (long long)(game_base + h[1]));
    return FK_OK;
}

// Device -> mailbox by stores (no copy engine), 4-byte words.
__global__ void fk_mail_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, uint32_t n_words) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

// Is a rows DMA (option "rows_async") in flight or about to be queued?  Then small results leave through the mailbox.
bool rows_dma_pending(fk_ctx *c) { return c->rows_async || (c->rows_calls && hipStreamQuery(c->copy_stream) == hipErrorNotReady); }

// `bytes` (a multiple of 4) of device memory -> `dst` on the host, behind what is queued on the main stream; complete after the
// stream has been synchronised AND deliver_mail() has run.  Through the mailbox while a rows DMA is pending, else one async copy.
int post_d2h(fk_ctx *c, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return FK_OK;
    if ((bytes & 3u) == 0 && bytes < ((size_t)1 << 31) && rows_dma_pending(c)) {
        const size_t off = (c->mail_used + 63u) & ~(size_t)63u;
        if (off + bytes > c->mail_cap && c->letters.empty()) { // grow (nothing of the old one is awaited)
            if (c->mail) (void)hipHostFree(c->mail);
            c->mail = nullptr;
            c->mail_cap = 0;
            const size_t cap = std::max<size_t>((size_t)4 << 20, (bytes + 4095u) & ~(size_t)4095u);
            if (hipHostMalloc(reinterpret_cast<void **>(&c->mail), cap, hipHostMallocDefault) == hipSuccess) c->mail_cap = cap;
            else (void)hipGetLastError();
        }
        if (off + bytes <= c->mail_cap) {
            const uint32_t n_words = (uint32_t)(bytes / 4);
            hipLaunchKernelGGL(fk_mail_kernel, dim3(std::min<uint32_t>((n_words + 255u) / 256u, 1024u)), dim3(256), 0, c->stream,
                               static_cast<const uint32_t *>(src), reinterpret_cast<uint32_t *>(c->mail + off), n_words);
            HIPCHK(c, hipGetLastError());
            c->letters.push_back({dst, off, bytes});
            c->mail_used = off + bytes;
            return FK_OK;
        }
    }
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return FK_OK;
}

// Room for `bytes` of letters before the first one is posted (a letter that does not fit goes by the copy engine — behind a rows DMA).
void reserve_mail(fk_ctx *c, size_t bytes) {
    if (!c->letters.empty() || bytes <= c->mail_cap || !rows_dma_pending(c)) return;
    if (c->mail) (void)hipHostFree(c->mail);
    c->mail = nullptr;
    c->mail_cap = 0;
    const size_t cap = std::max<size_t>((size_t)4 << 20, (bytes + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1));
    if (hipHostMalloc(reinterpret_cast<void **>(&c->mail), cap, hipHostMallocDefault) == hipSuccess) c->mail_cap = cap;
    else (void)hipGetLastError();
}

void deliver_mail(fk_ctx *c) { // the main stream has been synchronised
    for (const auto &l : c->letters) std::memcpy(l.dst, c->mail + l.off, l.bytes);
    c->letters.clear();
    c->mail_used = 0;
}

int check_device_error(fk_ctx *c, const int32_t *d_err, int64_t game_base, const char *what) {
    int32_t h[2] = {0, 0};
    const int rc = post_d2h(c, h, d_err, sizeof(h));
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    deliver_mail(c);
    return report_device_error(c, h, game_base, what);
}

// ---- what every playing entry states once ----
// A call begins: nothing of the call before it counts any more.  (fk_trace_games and fk_census_games / fk_tournament_run_census used
// to leave out the last two lines.  That was an omission without effect: they neither post nor deliver a letter, and every entry
// that does starts here.)
void begin_call(fk_ctx *c) {
    c->timing = fk_timing{};
    c->play_instance.clear();
    c->pending.clear();
    c->letters.clear(); // (a failed call may have left some)
    c->mail_used = 0;
}

int check_players(fk_ctx *c, int32_t k) { // the result word's seven winner-seat bits, the row's int8 winner_seat (REC_SAFETY is the next bit up)
    if (k > FK_MAX_PLAYERS)
        return fail(c, FK_ERR_ARG, "games have at most %d seats (a row names its winner's seat in an int8), got %d", FK_MAX_PLAYERS, (int)k);
    return FK_OK;
}

int check_max_rounds(fk_ctx *c, int32_t max_rounds) {
    if (max_rounds < 0 || max_rounds > 65535) return fail(c, FK_ERR_ARG, "max_rounds must be in [0, 65535]");
    return FK_OK;
}

int check_override_list(fk_ctx *c, const fk_override *ov, int32_t n_ov) {
    if (n_ov < 0 || (n_ov > 0 && !ov)) return fail(c, FK_ERR_ARG, "bad override list");
    return FK_OK;
}

// The argument checks of the game-list entries, in two halves (each entry has checks of its own between them): the list's shape ...
int check_list_shape(fk_ctx *c, int64_t n_games, int32_t S, int32_t k, int32_t max_rounds, int64_t max_seats) {
    if (k < 1 || S < 1 || n_games < 0 || n_games > max_seats / std::max(k, 1)) return fail(c, FK_ERR_ARG, "bad k / S / n_games");
    if (int rc = check_players(c, k)) return rc;
    return check_max_rounds(c, max_rounds);
}

// ... and its games
int check_list_games(fk_ctx *c, const fk_coord *coords, int64_t n_games, const int32_t *seat_strategy, int32_t S, int32_t k) {
    for (int64_t i = 0; i < n_games * k; ++i)
        if (seat_strategy[i] < 0 || seat_strategy[i] >= S) return fail(c, FK_ERR_ARG, "seat_strategy[%lld] out of range", (long long)i);
    for (int64_t i = 0; i < n_games; ++i) {
        if (coords[i].k != (uint64_t)k) // simulation.py:438
            return fail(c, FK_ERR_ARG, "Player RNG coordinate k does not match the number of seated strategies");
        if (coords[i].seat_index != 0) return fail(c, FK_ERR_ARG, "game coordinates carry seat_index 0 (seats are implied)");
    }
    return FK_OK;
}

// The argument checks of the tournament-range entries, in two halves for the same reason: the table's seating ...
int check_seating(fk_ctx *c, int32_t S, int32_t k) {
    if (k < 1 || S < k || S % k != 0) return fail(c, FK_ERR_ARG, "n_players must divide %d", S); // run_tournament.py:274
    return check_players(c, k);
}

// ... and the range
int check_range(fk_ctx *c, int32_t S, int32_t max_rounds, uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch,
                const fk_override *ov, int32_t n_ov) {
    if (S > 65535) return fail(c, FK_ERR_ARG, "S=%d exceeds 65535 strategies", S);
    if (int rc = check_max_rounds(c, max_rounds)) return rc;
    if (shuffle_end < shuffle_begin || shuffles_per_batch == 0) return fail(c, FK_ERR_ARG, "bad shuffle range / batch size");
    return check_override_list(c, ov, n_ov);
}

// shuffles per permutation block: what fits LDS beside the table's 2-byte rows
uint32_t perm_slots(int32_t S) { return (uint32_t)std::max<size_t>(1, std::min<size_t>(PERM_BLOCK, LDS_LIMIT / ((size_t)S * 2))); }

// the fields every game-kernel launch fills from the context and the call
PlayArgs table_args(const fk_ctx *c, int32_t target_score, int32_t max_rounds) {
    PlayArgs pa{};
    pa.strat = c->strat.p;
    pa.score_lut = c->score_lut.p;
    pa.discard_lut = c->discard_lut.p;
    pa.lds_tables = c->lds_tables.p;
    pa.target50 = ceil_div50(target_score);
    pa.beat50 = floor_div50(target_score);
    pa.max_rounds = (uint32_t)max_rounds;
    return pa;
}

// The strategies as the table-free game loops (fk_trace.h, fk_census.h) take them: thresholds in points.  A score threshold is only ever compared with
// turn totals in [50, 3 000 000] (1000 rolls of at most 3000 points), so clamping it to [0, 2^30] changes no comparison and
// keeps `turn + roll - threshold` inside int32.
std::vector<int2> strategies_in_points(const fk_strategy *table, int32_t S) {
    std::vector<int2> packed((size_t)S);
    for (int32_t i = 0; i < S; ++i)
        packed[(size_t)i] = make_int2(std::min(std::max(table[i].score_threshold, 0), 1 << 30), (int)pack_strategy(table[i]).y);
    return packed;
}

// the error word of the trace and census kernels (fk_trace.h: TR_*), once it is on the host
int report_plain_error(fk_ctx *c, unsigned long long err, const char *what) {
    if (err == fktr::TR_NO_ERROR) return FK_OK;
    const int32_t h[2] = {(err & 0xffu) == fktr::TR_ERR_ROLL_LIMIT ? FK_ERR_ROLL_LIMIT : FK_ERR_COUNTER_OVERFLOW, 0};
    return report_device_error(c, h, (int64_t)(err >> 8), what);
}

// The caller's overrides that concern a chunk -> chunk-local game ids, sorted by game id, on the device; `n_dev` of them.
// `locate(o, games)` says whether `o` is about this chunk at all and appends the games it names.  The last entry for a game wins.
template <class Locate>
int map_overrides(fk_ctx *c, const fk_override *ov, int32_t n_ov, uint32_t &n_dev, Locate locate) {
    std::vector<DevOverride> dov;
    std::vector<uint32_t> games;
    for (int32_t i = 0; i < n_ov; ++i) {
        games.clear();
        if (!locate(ov[i], games)) continue;
        if (ov[i].max_rounds > 65535u) return fail(c, FK_ERR_ARG, "override max_rounds must be <= 65535");
        for (const uint32_t game : games) {
            bool replaced = false;
            for (auto &dv : dov)
                if (dv.game == game) {
                    dv.max_rounds = ov[i].max_rounds;
                    replaced = true;
                }
            if (!replaced) dov.push_back(DevOverride{game, ov[i].max_rounds});
        }
    }
    n_dev = (uint32_t)dov.size();
    if (dov.empty()) return FK_OK;
    std::sort(dov.begin(), dov.end(), [](const DevOverride &x, const DevOverride &y) { return x.game < y.game; });
    int rc = ensure(c, c->ov, dov.size());
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->ov.p, dov.data(), dov.size() * sizeof(DevOverride), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FK_OK;
}

// ... for shuffles [sh0, sh0 + n_sh) of a tournament: game = (shuffle - sh0) * gps + game of the shuffle
int map_tournament_overrides(fk_ctx *c, const fk_override *ov, int32_t n_ov, uint64_t root_seed, int32_t k, uint64_t sh0, uint32_t n_sh,
                             uint32_t gps, uint32_t &n_dev) {
    return map_overrides(c, ov, n_ov, n_dev, [&](const fk_override &o, std::vector<uint32_t> &games) {
        if (o.root_seed != root_seed || o.k_or_order != (uint32_t)k) return false;
        if (o.a < sh0 || o.a >= sh0 + n_sh || o.b >= gps) return false;
        games.push_back((uint32_t)((o.a - sh0) * gps + o.b));
        return true;
    });
}

// Plays a call; after an out-of-device-memory failure (the budget was sized from hipMemGetInfo: somebody else's allocation came in
// between) gives the workspace back, plans with half and plays it again from its start.  `run` restores whatever a failed run changed.
template <class Run>
int replay_on_oom(fk_ctx *c, Run run) {
    c->oom = false;
    c->oom_replays = 0;
    c->chunk_limit = 0;
    int rc = run();
    while (rc == FK_ERR_HIP && c->oom && c->oom_replays < 8 && c->last_budget > ((int64_t)32 << 20)) {
        c->oom = false;
        ++c->oom_replays;
        release_workspace(c);
        c->chunk_limit = c->last_budget / 2;
        if (getenv("FK_DEBUG_REPLAY")) fprintf(stderr, "out of device memory: replay %d with a %lld-byte workspace\n", c->oom_replays, (long long)c->chunk_limit);
        rc = run();
    }
    c->chunk_limit = 0;
    return rc;
}


// Preparation of one chunk into chunk set `si` on `st`: (batched H2H) game -> block map, schedule class sizes, seat seeding.
// Fills the pointers of `sa`.  `full_state`: 48-byte state records (state-store instances, rows, all-seat statistics).
int seed_stage(fk_ctx *c, int si, hipStream_t st, SeedArgs &sa, bool full_state, bool timed) {
    ChunkSet &cs = c->sets[si];
    sa.state_dw = full_state ? STATE_DW : 4u;
    int rc = ensure_all(c, cs.state, (size_t)sa.n_games * sa.k * sa.state_dw, cs.inc, (size_t)sa.n_games * sa.k, cs.misc, 512);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(cs.misc.p, 0, 512, st));
    sa.state = cs.state.p;
    sa.inc = cs.inc.p;
    sa.seat_idx = nullptr;
    if (sa.perm_T && !full_state) { // the seats' strategy indices, resolved once by the seed kernel
        rc = ensure(c, cs.seat_idx, (size_t)sa.n_games * sa.k);
        if (rc) return rc;
        sa.seat_idx = cs.seat_idx.p;
    }
    if (sa.blocks) { // batched H2H: game -> block map first (the schedule classes and the seed kernel read it)
        hipLaunchKernelGGL(fk_block_map_kernel, dim3((sa.n_games + 255u) / 256u), dim3(256), 0, st, sa.blocks, sa.n_blocks,
                           sa.n_games, const_cast<uint32_t *>(sa.game_block), const_cast<uint32_t *>(sa.game_row));
        HIPCHK(c, hipGetLastError());
    }
    if ((sa.perm_T || sa.blocks) && c->longest_first) {
        rc = ensure(c, cs.order, (size_t)sa.n_games);
        if (rc) return rc;
        sa.sched = cs.order.p;
        sa.sched_ctr = cs.sched_ctr();
        rc = ensure(c, cs.classes, 16);
        if (rc) return rc;
        HIPCHK(c, hipMemsetAsync(cs.classes.p, 0, 64, st));
        sa.class_ctr = cs.classes.p;
        sa.patience = c->slow.p;
    } else {
        sa.sched = nullptr;
    }
    if (timed) (void)hipEventRecord(cs.ev[2], st);
    sa.pools = nullptr;
    if (!sa.coords) { // the pool every game of a shuffle / of a block starts from
        const uint32_t n = sa.blocks ? sa.n_blocks : (sa.gps ? (sa.n_games + sa.gps - 1u) / sa.gps : 1u);
        rc = ensure(c, cs.pools, (size_t)n);
        if (rc) return rc;
        sa.pools = cs.pools.p;
        hipLaunchKernelGGL(fk_pool_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, sa.prefix, sa.shuffle0, sa.pair, sa.order, sa.blocks, n, cs.pools.p);
    }
    if (sa.sched) // class sizes first: a game's ticket is class offset + rank
        hipLaunchKernelGGL(fk_class_count_kernel, dim3(std::min<uint32_t>((sa.n_games + SEED_BLOCK - 1u) / SEED_BLOCK, 1024u)), dim3(SEED_BLOCK), 0, st,
                           sa.perm_T, sa.perm_slots, sa.S, sa.k, sa.n_sh, sa.n_games, sa.patience, sa.blocks ? sa.game_row : nullptr, cs.classes.p);
    hipLaunchKernelGGL(fk_seed_kernel, dim3((sa.n_games + SEED_BLOCK - 1u) / SEED_BLOCK), dim3(SEED_BLOCK), 0, st, sa);
    if (timed) (void)hipEventRecord(cs.ev[3], st);
    HIPCHK(c, hipGetLastError());
    return FK_OK;
}

// bytes of device workspace one game needs in a chunk (state records, increments, schedule, result record, row)
size_t game_workspace_bytes(int32_t k, bool full_state, bool recs, bool rows) {
    return (size_t)k * ((full_state ? STATE_DW * 4 : 18) + 16) + 8 + (recs ? REC_DW * 4 + 4 : 0) +
           (rows ? sizeof(fk_row_hdr) + sizeof(fk_seat) * (size_t)k : 0);
}

// The game kernel of the chunk prepared in the current chunk set, on the main stream.  `want_state`: the final state records
// of every seat must be in the state store afterwards (rows, all-seat statistics); `want_rec0` / `want_recs`: the rec0 word /
// the full result record of every game.  Launch only: the caller checks the error record (finish_play).
int launch_play_stage(fk_ctx *c, const SeedArgs &sa, PlayArgs &pa, const LaunchPlan &plan, bool want_state, bool want_rec0, bool want_recs) {
    ChunkSet &cs = CSET(c);
    int rc;
    if (want_rec0) {
        rc = ensure(c, c->rec0, (size_t)sa.n_games);
        if (rc) return rc;
    }
    if (want_recs) {
        rc = ensure(c, c->recs, (size_t)sa.n_games * REC_DW);
        if (rc) return rc;
    }
    pa.sched = sa.sched;
    pa.seat_idx = sa.seat_idx;
    pa.state = sa.state;
    pa.state_dw = sa.state_dw;
    pa.inc = sa.inc;
    pa.rec0 = want_rec0 ? c->rec0.p : nullptr;
    pa.recs = want_recs ? c->recs.p : nullptr;
    pa.gs_out = (want_state && !plan.shape().gs) ? 1u : 0u;
    pa.ticket = cs.ticket();
    pa.err = cs.err();
    // hand-over threshold: the measured optimum is 8 up to eight seats (rounds 1 - 3) and grows with the game length beyond (round 5,
    // 5 160-strategy grid: k = 12 at 16 -1.5 %, k = 10 at 12 -0.6 % kernel time against 8)
    const int auto_thr = sa.k >= 11 ? 16 : sa.k >= 9 ? 12 : 8;
    pa.batch_threshold = (uint32_t)std::max(1, std::min(64, c->batch_threshold > 0 ? c->batch_threshold : auto_thr));
    pa.use_lds_tally = plan.lds_tally ? 1u : 0u;
    pa.no_flat = c->flat_handover ? 0u : 1u;
#ifdef FK_COUNT_HANDOVER // measuring build: the hand-over counts of fk_play_kernel, six zeroed words of the chunk's misc block
    pa.hcount = cs.hcount();
#else
    pa.hcount = nullptr;
#endif
    pa.clk = nullptr;
    c->clk_grid = 0;
    if (c->clock_stamps) {
        const size_t bytes = (size_t)std::max(plan.grid, 1) * 4 * sizeof(ull);
        rc = ensure(c, c->clk, bytes / sizeof(ull));
        if (rc) return rc;
        HIPCHK(c, hipMemsetAsync(c->clk.p, 0, bytes, c->stream));
        pa.clk = c->clk.p;
    }
    {
        Timer t(c, &c->timing.play_ms, SLOT_PLAY);
        LaunchPlan lp = plan;
        lp.mixed_flags = (c->uniform_flags_opt != 0) ? c->table_mixed_flags : 0xff00u;
        pa.uflags = c->table_flags;
        hipError_t e = launch_play(lp, pa, c->stream);
        t.stop();
        HIPCHK(c, e);
        c->play_instance = lp.instance ? lp.instance : "";
        c->timing.play_grid = lp.launched_grid;
        c->timing.play_mixed_flags = (int32_t)MIXED_FORMS[mixed_form(lp.mixed_flags)];
        if (pa.clk) c->clk_grid = lp.launched_grid;
    }
    c->timing.play_launches += 1;
    c->timing.play_block = plan.block;
    c->timing.play_lds_bytes = (int32_t)plan.lds;
    c->timing.games += sa.n_games;
    return FK_OK;
}

// the kernel timers of the chunk just played (incl. those of its preparation); the main stream has been synchronised
int finish_timers(fk_ctx *c) {
    HIPCHK(c, collect_timers(c));
    if (c->clk_grid > 0) { // shader clock of the last game kernel: median over its blocks of d(s_memtime) / d(s_memrealtime) x 100 MHz
        std::vector<unsigned long long> h((size_t)c->clk_grid * 4);
        HIPCHK(c, hipMemcpy(h.data(), c->clk.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        std::vector<double> mhz, ends;
        unsigned long long first = ~0ull;
        for (int b = 0; b < c->clk_grid; ++b) {
            const unsigned long long t0 = h[(size_t)b * 4], r0 = h[(size_t)b * 4 + 1], t1 = h[(size_t)b * 4 + 2], r1 = h[(size_t)b * 4 + 3];
            if (r1 > r0 && t1 > t0) {
                mhz.push_back(100.0 * (double)(t1 - t0) / (double)(r1 - r0));
                ends.push_back((double)r1);
                first = r0 < first ? r0 : first;
            }
        }
        if (!mhz.empty()) {
            std::nth_element(mhz.begin(), mhz.begin() + (std::ptrdiff_t)(mhz.size() / 2), mhz.end());
            c->timing.play_clock_mhz = (int32_t)(mhz[mhz.size() / 2] + 0.5);
            std::nth_element(ends.begin(), ends.begin() + (std::ptrdiff_t)(ends.size() / 2), ends.end());
            c->timing.play_block_end_p50_ms = (float)((ends[ends.size() / 2] - (double)first) * 1e-5); // 100 MHz ticks -> ms
            c->timing.play_block_end_max_ms = (float)((*std::max_element(ends.begin(), ends.end()) - (double)first) * 1e-5);
        }
        c->clk_grid = 0;
    }
    ChunkSet &cs = CSET(c);
    float ms = 0.f;
    // the permutations of a pipelined chunk ran on the main stream, in front of the previous game kernel: a clean interval
    if (hipEventElapsedTime(&ms, cs.ev[0], cs.ev[1]) == hipSuccess) c->timing.perm_ms += ms;
    if (cs.side) { // seeded behind another game kernel: no kernel-time reading for it (the interval includes the sharing)
        c->timing.prefetched_chunks += 1;
    } else if (hipEventElapsedTime(&ms, cs.ev[2], cs.ev[3]) == hipSuccess) {
        c->timing.seed_ms += ms;
    }
    return FK_OK;
}

// waits for the game kernel, reads its error record and the kernel timers
int finish_play(fk_ctx *c, const PlayArgs &pa, int64_t game_base, const char *what) {
    const int rc_dev = check_device_error(c, pa.err, game_base, what); // synchronises the main stream
    if (pa.hcount) { // (measuring build only)
        unsigned long long h[6] = {0, 0, 0, 0, 0, 0};
        HIPCHK(c, hipMemcpy(h, pa.hcount, sizeof(h), hipMemcpyDeviceToHost));
        c->timing.ho_handovers += (int64_t)h[0], c->timing.ho_lanes_served += (int64_t)h[1], c->timing.ho_trips += (int64_t)h[2];
        c->timing.ho_waiting_lane_trips += (int64_t)h[3], c->timing.ho_rolling_lane_trips += (int64_t)h[4], c->timing.ho_waves += (int64_t)h[5];
    }
    const int rc = finish_timers(c);
    return rc_dev ? rc_dev : rc;
}

// Seeds + games of one chunk (explicit game lists, batched H2H): preparation and game kernel back to back on the main stream.
int run_chunk(fk_ctx *c, const SeedArgs &sa_in, PlayArgs pa, const LaunchPlan &plan, bool want_state, bool want_rec0, bool want_recs,
              int64_t game_base, const char *what) {
    SeedArgs sa = sa_in;
    ChunkSet &cs = CSET(c);
    cs.prepared = false;
    cs.side = false;
    HIPCHK(c, hipStreamWaitEvent(c->stream, cs.ready, 0)); // an unused side-stream preparation may still own the set
    (void)hipEventRecord(cs.ev[0], c->stream); // no permutations here: an empty interval
    (void)hipEventRecord(cs.ev[1], c->stream);
    int rc = seed_stage(c, c->cur, c->stream, sa, plan.shape().gs || want_state, true);
    if (rc) return rc;
    rc = launch_play_stage(c, sa, pa, plan, want_state, want_rec0, want_recs);
    if (rc) return rc;
    return finish_play(c, pa, game_base, what);
}

// Pass `i` of a generation: how many blocks and games it holds; with `dst`, also writes its DevBlocks there on `st`.
using PassBlocks = std::function<int(size_t i, DevBlock *dst, hipStream_t st, uint32_t &n_blocks, uint32_t &n_games)>;
// Pass `i`'s pass-local max_rounds overrides, uploaded to c->ov; `n_dev` of them.
using PassOverrides = std::function<int(size_t i, uint32_t &n_dev)>;

// The passes (launches) of one generation of batched H2H blocks (fk_h2h_run_blocks, fk_h2h_round_robin): the games of every pass
// are played and their results added to c->block_out by block row, S / 2 rows of two strategies each.  The passes of a generation
// do not depend on each other's results, so with `pipelined` pass i + 1 is prepared (block table, game -> block map, pools,
// schedule classes, seat seeding) into the other chunk set on the low-priority stream while pass i plays, as tournament chunks are
// (15.5 ms of seeding per 6 x 10^8-attempt launch of BASELINE config 5 used to sit between the game kernels).  Without it — the
// caller's choice, or its per-pass override lists, which live in one device buffer — each pass is finished before the next is
// prepared on the main stream.  `overrides` may be empty: no pass has any.
int play_block_passes(fk_ctx *c, size_t n_passes, const LaunchPlan &plan, uint64_t root_seed, uint32_t S, int32_t target_score,
                      int32_t max_rounds, bool pipelined, const PassBlocks &blocks, const PassOverrides &overrides) {
    const SeedPool seat_prefix = seed_prefix(203u /* H2H_PLAYER */, root_seed, 2u);
    // preparation of pass `i` into chunk set `si` on stream `st`
    auto prepare = [&](size_t i, int si, hipStream_t st, SeedArgs &sa) -> int {
        ChunkSet &cs = c->sets[si];
        uint32_t nb = 0, games = 0;
        int rc2 = blocks(i, nullptr, st, nb, games);
        if (rc2) return rc2;
        cs.prepared = false;
        rc2 = ensure(c, cs.blocks, (size_t)nb);
        if (!rc2) rc2 = ensure(c, cs.game_block, (size_t)games);
        if (!rc2) rc2 = ensure(c, cs.game_row, (size_t)games);
        if (!rc2) rc2 = blocks(i, cs.blocks.p, st, nb, games);
        if (rc2) return rc2;
        sa = SeedArgs{};
        sa.prefix = seat_prefix;
        sa.gps = 0;
        sa.k = 2;
        sa.n_games = games;
        sa.blocks = cs.blocks.p;
        sa.n_blocks = nb;
        sa.game_block = cs.game_block.p;
        sa.game_row = cs.game_row.p;
        rc2 = seed_stage(c, si, st, sa, false, true);
        if (rc2) return rc2;
        HIPCHK(c, hipEventRecord(cs.ready, st));
        cs.side = (st == c->prep_stream);
        return FK_OK;
    };

    int rc;
    std::vector<SeedArgs> sas(n_passes);
    std::vector<int> set_of(n_passes);
    set_of[0] = c->cur;
    HIPCHK(c, hipStreamWaitEvent(c->stream, CSET(c).ready, 0)); // an unused side-stream preparation may still own the set
    (void)hipEventRecord(CSET(c).ev[0], c->stream);             // no permutations here: an empty interval
    (void)hipEventRecord(CSET(c).ev[1], c->stream);
    if ((rc = prepare(0, c->cur, c->stream, sas[0]))) return rc;
    for (size_t i = 0; i < n_passes; ++i) {
        c->cur = set_of[i];
        uint32_t n_ov = 0;
        if (overrides && (rc = overrides(i, n_ov))) return rc;
        HIPCHK(c, hipEventRecord(c->main_idle, c->stream)); // everything that used the other chunk set is in front of this point
        if (i + 1 < n_passes) {
            set_of[i + 1] = c->cur ^ 1;
            if (pipelined) {
                HIPCHK(c, hipStreamWaitEvent(c->prep_stream, c->main_idle, 0));
                (void)hipEventRecord(c->sets[c->cur ^ 1].ev[0], c->prep_stream);
                (void)hipEventRecord(c->sets[c->cur ^ 1].ev[1], c->prep_stream);
                if ((rc = prepare(i + 1, c->cur ^ 1, c->prep_stream, sas[i + 1]))) return rc;
            }
        }
        PlayArgs pa = table_args(c, target_score, max_rounds);
        pa.game_block = sas[i].game_row; // the kernel wants table rows: seat s of a game plays strategy 2 * row + s
        pa.ov = overrides ? c->ov.p : nullptr;
        pa.n_ov = n_ov;
        pa.mode = MODE_BLOCKS;
        pa.n_games = sas[i].n_games;
        pa.gps = 1;
        pa.n_sh = 1;
        pa.k = 2;
        pa.S = S;
        HIPCHK(c, hipStreamWaitEvent(c->stream, CSET(c).ready, 0));
        if ((rc = launch_play_stage(c, sas[i], pa, plan, false, true, false))) return rc;
        hipLaunchKernelGGL(fk_h2h_reduce_kernel, dim3((pa.n_games + 256u * H2H_RUN - 1u) / (256u * H2H_RUN)), dim3(256), 0, c->stream,
                           c->rec0.p, pa.n_games, S / 2u, c->block_out.p);
        HIPCHK(c, hipGetLastError());
        if (!pipelined) { // (the next pass may re-use the one override buffer)
            if ((rc = finish_play(c, pa, 0, "h2h attempt (pass-local index)"))) return rc;
            if (i + 1 < n_passes) {
                (void)hipEventRecord(c->sets[c->cur ^ 1].ev[0], c->stream);
                (void)hipEventRecord(c->sets[c->cur ^ 1].ev[1], c->stream);
                if ((rc = prepare(i + 1, c->cur ^ 1, c->stream, sas[i + 1]))) return rc;
            }
        } else {
            // the pass's error record and timers are read before the next launch reuses the kernel timer events
            HIPCHK(c, hipMemcpyAsync(c->err_host, pa.err, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            rc = report_device_error(c, c->err_host, 0, "h2h attempt (pass-local index)");
            const int rc_t = finish_timers(c);
            if (rc) return rc;
            if (rc_t) return rc_t;
        }
    }
    return FK_OK;
}

// The accepted Fisher-Yates draws of a split launch as they lie in cs.draws: groups of eight 16-bit draws in one uint4, draw n of a
// shuffle = the j of step S - 1 - n (so draws[n] <= S - 1 - n), oldest in the low half; a last partial group is right-aligned in the top
// halves, behind the draws before it.  Group g of shuffle sh is the uint4 at g * g_stride + sh * sh_stride:
//   path 1 (fk_perm_apply_kernel, the swap chains): group-major, g_stride = n_sh rounded up to 64;
//   path 2 (fk_perm_parallel_kernel + fk_perm_block_kernel): one row of groups + 1 uint4 per shuffle (a row also takes the S results).
struct DrawLayout {
    uint32_t groups, g_stride, sh_stride;
    size_t bytes;
};

DrawLayout draw_layout(int path, uint32_t S, uint32_t n_sh) {
    const uint32_t groups = (S - 1u + 7u) / 8u;
    if (path == 2) return DrawLayout{groups, 1u, groups + 1u, (size_t)n_sh * (groups + 1u) * 16};
    const uint32_t n_sh_pad = (n_sh + 63u) & ~63u;
    return DrawLayout{groups, n_sh_pad, 1u, (size_t)groups * n_sh_pad * 16};
}

// the chain-free kernel holds a shuffle in 14 B of LDS per strategy (+ its static words)
bool perm_parallel_fits(int32_t S) { return (size_t)S * 14 <= LDS_LIMIT - 1024; }

int configure_perm_kernels(fk_ctx *c) {
    static int perm_configured = -1; // per device (a second context may sit on another GPU of this process)
    if (perm_configured != c->device) {
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&fk_perm_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&fk_perm_apply_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&fk_perm_parallel_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_LIMIT - 1024))); // + its static words
        perm_configured = c->device;
    }
    return FK_OK;
}

// First step of a split launch: the draws of shuffles [d.sh0, d.sh0 + d.n_sh) into cs.draws (ensured here) in layout `dl`.  A wave per
// shuffle while the launch is small (fk_perm_wave.h: ~20 us instead of the thread-per-shuffle kernel's 1 ms latency), a thread per
// shuffle when there are enough shuffles to fill the chip with them.
int launch_perm_draws(fk_ctx *c, ChunkSet &cs, hipStream_t st, const ChunkDesc &d, const DrawLayout &dl) {
    const uint32_t n_sh = d.n_sh;
    const SeedPool perm_prefix = seed_prefix(101u /* SHUFFLE_PERMUTATION */, d.root, (uint64_t)d.k);
    const bool wave_draw = c->perm_draw_wave == 1 || (c->perm_draw_wave < 0 && n_sh <= WAVE_DRAW_MAX_SH);
    const int rc = ensure(c, cs.draws, dl.bytes);
    if (rc) return rc;
    if (wave_draw)
        hipLaunchKernelGGL(fk_perm_draw_wave_kernel, dim3((n_sh + WAVE_DRAW_BLOCK / 64 - 1u) / (WAVE_DRAW_BLOCK / 64)), dim3(WAVE_DRAW_BLOCK), 0, st,
                           perm_prefix, d.sh0, n_sh, d.S, dl.g_stride, dl.sh_stride, cs.draw_groups());
    else
        hipLaunchKernelGGL(fk_perm_draw_kernel, dim3((n_sh + DRAW_BLOCK - 1u) / DRAW_BLOCK), dim3(DRAW_BLOCK), 0, st,
                           perm_prefix, d.sh0, n_sh, d.S, dl.g_stride, dl.sh_stride, cs.draw_groups());
    return FK_OK;
}

// Second step: the permutations of n_sh shuffles from the draws in cs.draws (layout `dl` of `path`) into cs.perm (blocked layout); the
// caller has ensured both buffers.  Shared with fk_debug_perm_from_draws, which uploads the draws instead of drawing them.
void launch_perm_consumers(ChunkSet &cs, hipStream_t st, int path, const DrawLayout &dl, uint32_t n_sh, uint32_t S, uint32_t slots) {
    const uint32_t perm_blocks = (n_sh + slots - 1u) / slots;
    if (path == 2) {
        hipLaunchKernelGGL(fk_perm_parallel_kernel, dim3(n_sh), dim3(PP_BLOCK), (size_t)S * 14, st, cs.draw_groups(), dl.sh_stride, n_sh, S);
        hipLaunchKernelGGL(fk_perm_block_kernel, dim3((S + 255u) / 256u, perm_blocks), dim3(256), 0, st, cs.draws16(), dl.sh_stride * 8u, n_sh, S, slots,
                           cs.perm.p);
    } else {
        hipLaunchKernelGGL(fk_perm_apply_kernel, dim3(perm_blocks), dim3(PERM_BLOCK), (size_t)slots * S * 2, st, cs.draw_groups(), dl.g_stride, n_sh, S, slots,
                           cs.perm.p);
    }
}

// The permutation kernels of shuffles [d.sh0, d.sh0 + d.n_sh) into cs.perm (blocked layout, perm_at()) on `st`; the caller has
// ensured cs.perm.  Shared by the tournament chunks and the roll census (fk_tournament_run_census).
int launch_perm_kernels(fk_ctx *c, ChunkSet &cs, hipStream_t st, const ChunkDesc &d) {
    const int32_t S = (int32_t)d.S;
    const uint32_t n_sh = d.n_sh, slots = d.slots;
    int rc = configure_perm_kernels(c);
    if (rc) return rc;
    // large tables: the draws at full occupancy first (fk_perm_draw_kernel); then either the chain-free
    // permutation (fk_perm_parallel_kernel, one workgroup per shuffle, 14 B of LDS per strategy) or, for tables
    // beyond its LDS reach, the bare swap chains over LDS arrays (fk_perm_apply_kernel)
    const bool split = c->perm_split >= 1 || (c->perm_split < 0 && S >= 1024 && n_sh >= 256);
    if (split) {
        const int path = (c->perm_split != 1 && perm_parallel_fits(S)) ? 2 : 1;
        const DrawLayout dl = draw_layout(path, d.S, n_sh);
        if ((rc = launch_perm_draws(c, cs, st, d, dl))) return rc;
        launch_perm_consumers(cs, st, path, dl, n_sh, d.S, slots);
    } else {
        const uint32_t perm_blocks = (n_sh + slots - 1u) / slots;
        hipLaunchKernelGGL(fk_perm_kernel, dim3(perm_blocks), dim3(PERM_BLOCK), (size_t)slots * S * 2, st, seed_prefix(101u /* SHUFFLE_PERMUTATION */, d.root,
                           (uint64_t)d.k), d.sh0, n_sh, d.S, slots, cs.perm.p);
    }
    HIPCHK(c, hipGetLastError());
    return FK_OK;
}

// Tournament chunk into chunk set `si`: permutations of shuffles [d.sh0, d.sh0 + d.n_sh) on the main stream, then schedule +
// seat seeding on `st`.  `sa` comes back with every pointer the game kernel and the post-passes need.
//   st == main stream: the chunk is about to be played.
//   st == prep_stream: the chunk is the NEXT one; the caller launches the current game kernel right after this returns.  The
//   permutation kernels want most of a CU's LDS, which a resident persistent game kernel does not leave them (on the side
//   stream they would only start when it ends, with the seeding behind them): they go in front of that game kernel on the
//   main stream (0.1 ms at 64 strategies, 5 ms per 10^8 games at 5 160), and only the LDS-free part — schedule classes and
//   seat seeding — shares the chip with the game kernel.
int prep_tournament_chunk(fk_ctx *c, int si, hipStream_t st_seed, const ChunkDesc &d, SeedArgs &sa) {
    ChunkSet &cs = c->sets[si];
    cs.prepared = false;
    hipStream_t st = c->stream;
    HIPCHK(c, hipStreamWaitEvent(st, cs.ready, 0)); // an unused side-stream preparation may still own the set
    const int32_t S = (int32_t)d.S;
    const uint32_t n_sh = d.n_sh, slots = d.slots, gps = d.S / d.k;
    const uint32_t perm_blocks = (n_sh + slots - 1u) / slots;
    int rc = ensure(c, cs.perm, (size_t)perm_blocks * S * slots);
    if (rc) return rc;
    (void)hipEventRecord(cs.ev[0], st);
    if ((rc = launch_perm_kernels(c, cs, st, d))) return rc;
    (void)hipEventRecord(cs.ev[1], st);
    sa = SeedArgs{};
    sa.prefix = seed_prefix(103u /* TOURNAMENT_PLAYER */, d.root, (uint64_t)d.k);
    sa.coords = nullptr;
    sa.shuffle0 = d.sh0;
    sa.gps = gps;
    sa.k = d.k;
    sa.n_games = n_sh * gps;
    sa.perm_T = cs.perm.p;
    sa.perm_slots = slots;
    sa.S = d.S;
    sa.n_sh = n_sh;
    if (st_seed != st) {
        HIPCHK(c, hipStreamWaitEvent(st_seed, cs.ev[1], 0));     // the permutations
        HIPCHK(c, hipStreamWaitEvent(st_seed, c->main_idle, 0)); // the set's previous users (recorded by the caller)
    }
    rc = seed_stage(c, si, st_seed, sa, d.state_dw == STATE_DW, true);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(cs.ready, st_seed));
    cs.desc = d;
    cs.prepared = true;
    cs.side = (st_seed == c->prep_stream);
    return FK_OK;
}

// state store + result records of the chunk just played -> rows at `d_rows` (device), game-id order
int rows_pass(fk_ctx *c, const SeedArgs &sa, bool scheduled, uint32_t n_games, uint32_t gps, uint32_t n_sh, bool perm_mode, uint8_t *d_rows) {
    // `scheduled`: the caller has inverted the schedule into c->inv (fk_invert_sched_kernel)
    const uint32_t *inv = scheduled ? c->inv.p : nullptr;
    const uint32_t row_dw = 1u + 7u * sa.k;
    // rows of a block leave through an LDS tile as whole lines: the largest block whose tile fits 64 KiB
    uint32_t block = 256;
    while (block > 64 && (size_t)block * row_dw * 4 > 65536) block -= 64;
    const size_t tile = (size_t)block * row_dw * 4;
    if (tile <= 65536) {
        static int configured = -1;
        if (configured != c->device) {
            HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&fk_rows_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
            configured = c->device;
        }
        hipLaunchKernelGGL(fk_rows_kernel<true>, dim3((n_games + block - 1u) / block), dim3(block), tile, c->stream, CSET(c).state.p, c->recs.p, inv, n_games,
                           gps, n_sh, sa.k, perm_mode ? 1u : 0u, d_rows);
    } else { // tables of more than 36 seats: one thread stores its own row
        hipLaunchKernelGGL(fk_rows_kernel<false>, dim3((n_games + 255u) / 256u), dim3(256), 0, c->stream, CSET(c).state.p, c->recs.p, inv, n_games, gps, n_sh,
                           sa.k, perm_mode ? 1u : 0u, d_rows);
    }
    HIPCHK(c, hipGetLastError());
    return FK_OK;
}

// ---- RCCL, bound at run time ----
// The tally reduction is the path's only exchange: one ncclReduce(sum, int64) over xGMI.  librccl is
// dlopen'ed on first use, so the library loads (and every single-GPU entry point works) on hosts without RCCL.
struct Rccl {
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, fk_comm_id, int) = nullptr; // ncclUniqueId is a 128-byte struct passed by value
    // non-blocking initialisation (a rank that never joins must not park its peers inside RCCL): optional symbols
    int (*CommInitRankConfig)(void **, int, fk_comm_id, int, ncclConfig_t *) = nullptr;
    int (*CommGetAsyncError)(void *, int *) = nullptr;
    int (*CommAbort)(void *) = nullptr;
    int (*Reduce)(const void *, void *, size_t, int, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string why;
};

Rccl &rccl() {
    static Rccl r;
    if (r.lib || !r.why.empty()) return r;
    // The RCCL that belongs to the HIP runtime this process actually runs on: the one next to the loaded libamdhip64
    // (a process that imported PyTorch first runs on the runtime bundled with it, and so must the communicator), then
    // the system one.
    std::vector<std::string> names;
    Dl_info info{};
    if (dladdr(reinterpret_cast<const void *>(&hipGetDeviceCount), &info) && info.dli_fname) {
        std::string dir(info.dli_fname);
        const size_t slash = dir.rfind('/');
        if (slash != std::string::npos) {
            dir.resize(slash);
            names.push_back(dir + "/librccl.so.1");
            names.push_back(dir + "/librccl.so");
        }
    }
    for (const char *name : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"}) names.emplace_back(name);
    for (const auto &name : names) {
        r.lib = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (r.lib) break;
    }
    if (!r.lib) {
        r.why = std::string("librccl.so.1 could not be loaded: ") + (dlerror() ? dlerror() : "not found");
        return r;
    }
    r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
    r.Reduce = reinterpret_cast<decltype(r.Reduce)>(dlsym(r.lib, "ncclReduce"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
    r.CommInitRankConfig = reinterpret_cast<decltype(r.CommInitRankConfig)>(dlsym(r.lib, "ncclCommInitRankConfig"));
    r.CommGetAsyncError = reinterpret_cast<decltype(r.CommGetAsyncError)>(dlsym(r.lib, "ncclCommGetAsyncError"));
    r.CommAbort = reinterpret_cast<decltype(r.CommAbort)>(dlsym(r.lib, "ncclCommAbort"));
    if (!r.GetUniqueId || !r.CommInitRank || !r.Reduce || !r.CommDestroy) {
        r.why = "librccl.so.1 lacks ncclGetUniqueId / ncclCommInitRank / ncclReduce / ncclCommDestroy";
        dlclose(r.lib);
        r.lib = nullptr;
    }
    return r;
}

int rccl_fail(fk_ctx *c, const char *what, int code) {
    Rccl &r = rccl();
    return fail(c, FK_ERR_COMM, "%s failed: %s", what, r.GetErrorString ? r.GetErrorString(code) : "RCCL error");
}

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// Give the communicator up: abort it (ncclCommAbort ends a collective kernel that waits for a peer) and forget it.
void comm_abandon(fk_ctx *c) {
    Rccl &r = rccl();
    const bool dbg = getenv("FK_DEBUG_COMM") != nullptr;
    if (c->comm) {
        if (dbg) fprintf(stderr, "[fk comm] abandoning the communicator (%s)\n", r.CommAbort ? "ncclCommAbort" : "ncclCommDestroy");
        if (r.CommAbort) (void)r.CommAbort(c->comm);
        else (void)r.CommDestroy(c->comm);
        if (dbg) fprintf(stderr, "[fk comm] abandoned\n");
    }
    c->comm = nullptr;
    c->comm_world = 1;
    c->comm_rank = 0;
    c->comm_async = false;
    c->comm_lost = true; // (never silently fall back to a one-rank "reduction" of a multi-rank job)
}

// A non-blocking communicator reports ncclInProgress from every call until the operation has been issued: poll its state
// under the context's deadline ("comm_timeout_ms").  On expiry or error the communicator is aborted -> FK_ERR_COMM.
int comm_settle(fk_ctx *c, const char *what, int rc, double t0) {
    Rccl &r = rccl();
    if (rc != ncclSuccess && rc != ncclInProgress) {
        const int out = rccl_fail(c, what, rc);
        comm_abandon(c);
        return out;
    }
    if (!c->comm_async) return FK_OK;
    for (;;) {
        int st = ncclSuccess;
        const int q = r.CommGetAsyncError(c->comm, &st);
        if (q != ncclSuccess || (st != ncclSuccess && st != ncclInProgress)) {
            const int out = rccl_fail(c, what, q != ncclSuccess ? q : st);
            comm_abandon(c);
            return out;
        }
        if (st == ncclSuccess) return FK_OK;
        if (now_ms() - t0 > (double)c->comm_timeout_ms) {
            comm_abandon(c);
            return fail(c, FK_ERR_COMM, "%s did not complete within %d ms (comm_timeout_ms): a peer rank never joined; communicator aborted", what,
                        c->comm_timeout_ms);
        }
        usleep(500);
    }
}

// Wait for the context's stream behind a collective, under the same deadline: a peer that never enters the collective leaves
// the RCCL kernel spinning, and hipStreamSynchronize would wait with it.
int comm_wait_stream(fk_ctx *c, const char *what, double t0) {
    hipEvent_t ev = c->ev[SLOT_CALL + 1];
    HIPCHK(c, hipEventRecord(ev, c->stream));
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return FK_OK;
        if (q != hipErrorNotReady) return fail(c, FK_ERR_HIP, "%s: %s", what, hipGetErrorString(q));
        if (c->comm_timeout_ms > 0 && now_ms() - t0 > (double)c->comm_timeout_ms) {
            comm_abandon(c);
            (void)hipStreamSynchronize(c->stream); // the aborted collective returns
            return fail(c, FK_ERR_COMM, "%s did not complete within %d ms (comm_timeout_ms): a peer rank never entered the collective; communicator aborted",
                        what, c->comm_timeout_ms);
        }
        usleep(200);
    }
}

} // namespace

// Exactness of a cell's resampled int64 totals: every value of both [B][S] matrices in [0, 2^63 / B)
static bool boot_totals_exact(const int64_t *wins, const int64_t *exposures, uint64_t B, size_t S) {
    const uint64_t limit = ((uint64_t)1 << 63) / B;
    const size_t cells = (size_t)B * S;
    uint64_t seen = 0, top = 0; // OR of all values (a negative one sets the top bit); their maximum, looked for only when the OR is large
    for (const int64_t *m : {wins, exposures})
        for (size_t j = 0; j < cells; ++j) seen |= (uint64_t)m[j];
    if (seen >= limit)
        for (const int64_t *m : {wins, exposures})
            for (size_t j = 0; j < cells; ++j) top = std::max(top, (uint64_t)m[j]);
    return top < limit;
}

extern "C" {

void fk_destroy(fk_ctx *c);

int fk_init(int device_ordinal, fk_ctx **out) {
    if (!out) return FK_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FK_ERR_NO_DEVICE;
    if (device_ordinal < 0 || device_ordinal >= n) return FK_ERR_ARG;
    fk_ctx *c = new fk_ctx();
    c->device = device_ordinal;
    if (hipSetDevice(device_ordinal) != hipSuccess || hipGetDeviceProperties(&c->prop, device_ordinal) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        fk_destroy(c); // releases whatever was created
        return FK_ERR_HIP;
    }
    for (auto &e : c->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            fk_destroy(c);
            return FK_ERR_HIP;
        }
    {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        bool ok = hipStreamCreateWithPriority(&c->prep_stream, hipStreamNonBlocking, least) == hipSuccess;
        ok = ok && hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) == hipSuccess;
        for (int i = 0; i < 2; ++i) {
            ok = ok && hipEventCreateWithFlags(&c->ev_rows[i], hipEventDisableTiming) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&c->ev_copy[i], hipEventDisableTiming) == hipSuccess;
        }
        for (int i = 0; i < FK_ROWS_EVENTS; ++i) {
            ok = ok && hipEventCreateWithFlags(&c->ev_call_copy[i], hipEventDisableTiming) == hipSuccess;
        }
        ok = ok && hipEventCreateWithFlags(&c->main_idle, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipHostMalloc(reinterpret_cast<void **>(&c->err_host), 2 * sizeof(int32_t), hipHostMallocDefault) == hipSuccess;
        for (auto &cs : c->sets) {
            ok = ok && hipEventCreateWithFlags(&cs.ready, hipEventDisableTiming) == hipSuccess;
            for (auto &e : cs.ev) ok = ok && hipEventCreate(&e) == hipSuccess;
        }
        if (!ok) {
            fk_destroy(c);
            return FK_ERR_HIP;
        }
    }
    // score table (fk_device.h): 512 KiB, built by one small kernel, read by every roll of the game kernel
    if (ensure(c, c->score_lut, SCORE_LUT_KEYS) != FK_OK) {
        fk_destroy(c);
        return FK_ERR_HIP;
    }
    if (ensure(c, c->discard_lut, DISCARD_LUT_KEYS * (1 + sizeof(uint32_t))) != FK_OK) { // the byte table and, behind it, the wide one
        fk_destroy(c);
        return FK_ERR_HIP;
    }
    hipLaunchKernelGGL(fk_score_lut_kernel, dim3(SCORE_LUT_KEYS / 256), dim3(256), 0, c->stream, c->score_lut.p);
    hipLaunchKernelGGL(fk_discard_lut_kernel, dim3(DISCARD_LUT_KEYS / 256), dim3(256), 0, c->stream, c->discard_lut.p);
    {
        const std::vector<uint8_t> img = build_lds_tables();
        if (ensure(c, c->lds_tables, img.size()) != FK_OK ||
            hipMemcpyAsync(c->lds_tables.p, img.data(), img.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) {
            fk_destroy(c);
            return FK_ERR_HIP;
        }
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
        fk_destroy(c);
        return FK_ERR_HIP;
    }
    *out = c;
    return FK_OK;
}

void fk_destroy(fk_ctx *c) {
    if (!c) return;
    for (void *p : c->hog) (void)hipFree(p);
    c->hog.clear();
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) (void)rccl().CommDestroy(c->comm);
    c->comm = nullptr;
    if (c->prep_stream) (void)hipStreamSynchronize(c->prep_stream);
    for (auto &cs : c->sets) {
        if (cs.ready) (void)hipEventDestroy(cs.ready);
        for (auto &e : cs.ev)
            if (e) (void)hipEventDestroy(e);
    }
    if (c->copy_stream) {
        (void)hipStreamSynchronize(c->copy_stream);
        (void)hipStreamDestroy(c->copy_stream);
    }
    for (int i = 0; i < 2; ++i) {
        if (c->ev_rows[i]) (void)hipEventDestroy(c->ev_rows[i]);
        if (c->ev_copy[i]) (void)hipEventDestroy(c->ev_copy[i]);
    }
    for (auto &e : c->ev_call_copy)
        if (e) (void)hipEventDestroy(e);
    if (c->main_idle) (void)hipEventDestroy(c->main_idle);
    if (c->err_host) (void)hipHostFree(c->err_host);
    if (c->mail) (void)hipHostFree(c->mail);
    if (c->prep_stream) (void)hipStreamDestroy(c->prep_stream);
    for (auto &e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c; // (the device is still current) frees every device buffer: each Dev member releases its own
}

const char *fk_last_error(fk_ctx *c) { return c ? c->err.c_str() : "null context"; }

const char *fk_last_play_instance(fk_ctx *c) { return c ? c->play_instance.c_str() : ""; }

int fk_get_device_info(fk_ctx *c, fk_device_info *out) {
    if (!c || !out) return FK_ERR_ARG;
    memset(out, 0, sizeof(*out));
    snprintf(out->name, sizeof(out->name), "%s", c->prop.name);
    snprintf(out->arch, sizeof(out->arch), "%s", c->prop.gcnArchName);
    out->compute_units = c->prop.multiProcessorCount;
    out->clock_mhz = c->prop.clockRate / 1000;
    out->wavefront_size = c->prop.warpSize;
    out->lds_bytes_per_cu = (int32_t)c->prop.maxSharedMemoryPerMultiProcessor;
    out->hbm_bytes = c->prop.totalGlobalMem;
    return FK_OK;
}

// Page-locked host memory for the rows / column-image destinations.  Anonymous pages populated by the kernel (mmap MAP_POPULATE: outside
// the HIP runtime, so several buffers can be made at once and no launch waits meanwhile) and then registered with the runtime — measured on
// the MI355X host for 256 MB: 12 - 21 ms + 1 - 3 ms, against 41 - 55 ms for hipHostMalloc (two of those at once: 126 ms, and every HIP call
// of the process queues behind them); device-to-host copies into either run at the same 57 GB/s.  hipHostMalloc remains the fallback.
static std::mutex g_host_lock;
static std::unordered_map<void *, size_t> g_host_mapped; // registered mmap blocks -> their length

int fk_host_alloc(fk_ctx *c, size_t bytes, void **out) {
    if (!c || !out) return FK_ERR_ARG;
    *out = nullptr;
    const size_t page = (size_t)2 << 20, size = (std::max<size_t>(bytes, 1) + page - 1) & ~(page - 1);
    void *p = mmap(nullptr, size, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_POPULATE, -1, 0);
    if (p != MAP_FAILED) {
        if (hipSetDevice(c->device) == hipSuccess && hipHostRegister(p, size, hipHostRegisterDefault) == hipSuccess) {
            std::lock_guard<std::mutex> lk(g_host_lock);
            g_host_mapped[p] = size;
            *out = p;
            return FK_OK;
        }
        (void)hipGetLastError();
        munmap(p, size);
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipHostMalloc(out, std::max<size_t>(bytes, 1), hipHostMallocDefault));
    return FK_OK;
}

int fk_host_free(fk_ctx *c, void *p) {
    if (!c) return FK_ERR_ARG;
    if (!p) return FK_OK;
    size_t mapped = 0;
    {
        std::lock_guard<std::mutex> lk(g_host_lock);
        auto it = g_host_mapped.find(p);
        if (it != g_host_mapped.end()) {
            mapped = it->second;
            g_host_mapped.erase(it);
        }
    }
    if (mapped) {
        const hipError_t e = hipHostUnregister(p);
        munmap(p, mapped);
        HIPCHK(c, e);
        return FK_OK;
    }
    HIPCHK(c, hipHostFree(p));
    return FK_OK;
}

int fk_get_timing(fk_ctx *c, fk_timing *out) {
    if (!c || !out) return FK_ERR_ARG;
    *out = c->timing;
    return FK_OK;
}

// Tests of the memory budget: take device memory until about `leave_free` bytes are free (held by the context until the next call
// with leave_free < 0, or fk_destroy); free_now / total as hipMemGetInfo reports them afterwards.
int fk_debug_hold_memory(fk_ctx *c, int64_t leave_free, int64_t *free_now, int64_t *total) {
    if (!c) return FK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (leave_free < 0) {
        for (void *p : c->hog) (void)hipFree(p);
        c->hog.clear();
    }
    size_t free_b = 0, total_b = 0;
    for (;;) {
        HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
        if (leave_free < 0 || (int64_t)free_b - leave_free < ((int64_t)64 << 20)) break;
        void *p = nullptr;
        const size_t step = std::min<size_t>((size_t)((int64_t)free_b - leave_free), (size_t)32 << 30);
        if (hipMalloc(&p, step) != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
        c->hog.push_back(p);
    }
    if (free_now) *free_now = (int64_t)free_b;
    if (total) *total = (int64_t)total_b;
    return FK_OK;
}

static int32_t effective_comm_timeout_ms(const fk_ctx *c);

int fk_get_option(fk_ctx *c, const char *name, int64_t *value) {
    if (!c || !name || !value) return FK_ERR_ARG;
    const std::string n(name);
    if (n == "chunk_bytes") *value = c->chunk_bytes;
    else if (n == "workspace_percent") *value = c->workspace_percent;
    else if (n == "last_budget") *value = c->last_budget;
    else if (n == "device_bytes_held") *value = g_device_bytes_held.load();
    else if (n == "oom_replays") *value = c->oom_replays;
    else if (n == "comm_timeout_ms") *value = effective_comm_timeout_ms(c);
    else if (n == "rows_chunk_games") *value = c->rows_chunk_games;
    else if (n == "rows_async") *value = c->rows_async;
    else if (n == "rows_event") *value = c->last_rows_event;
    else if (n == "census_chunk_games") *value = c->census_chunk_games;
    else if (n == "rr_window_blocks") *value = c->rr_window_blocks;
    else if (n == "rr_keep_roots") *value = c->ri_keep_roots ? 1 : 0;
    else if (n == "agreement_grid") *value = c->agreement_grid;
    else if (n == "performance_grid") *value = c->performance_grid;
    else if (n == "root_windows_grid") *value = c->root_windows_grid;
    else return fail(c, FK_ERR_ARG, "fk_get_option: unknown option %s", name);
    return FK_OK;
}

int fk_set_option(fk_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return FK_ERR_ARG;
    std::string n(name);
    if (n == "chunk_bytes") c->chunk_bytes = std::max<int64_t>(value, 1 << 20);
    else if (n == "workspace_percent") c->workspace_percent = (int32_t)std::min<int64_t>(std::max<int64_t>(value, 1), 100000);
    else if (n == "comm_timeout_ms") {
        c->comm_timeout_ms = (int32_t)std::min<int64_t>(std::max<int64_t>(value, 0), 86400000);
        c->comm_timeout_set = true; // from now on the FK_COMM_TIMEOUT_MS environment default is not consulted
    }
    else if (n == "batch_threshold") c->batch_threshold = (int32_t)value;
    else if (n == "use_lds_tally") c->use_lds_tally = (int32_t)value;
    else if (n == "longest_first") c->longest_first = (int32_t)value;
    else if (n == "blocks_per_cu") c->blocks_per_cu = (int32_t)value;
    else if (n == "max_waves") c->max_waves = (int32_t)std::min<int64_t>(std::max<int64_t>(value, 1), 8);
    else if (n == "lean") c->lean = (int32_t)value;
    else if (n == "state_store") c->gs = (int32_t)value;
    else if (n == "rows_chunk_games") c->rows_chunk_games = std::max<int64_t>(value, 1);
    else if (n == "rows_async") c->rows_async = value != 0;
    else if (n == "resident_tally") {
        c->resident = value != 0;
        c->acc_n = 0; // the next tournament call starts a fresh accumulator
    } else if (n == "hot_cold") {
        if (value != -1 && value != 0) return fail(c, FK_ERR_ARG, "hot_cold is -1 (auto: four and more seats) or 0 (never)");
        c->hc = (int32_t)value;
    }
    else if (n == "clock_stamps") c->clock_stamps = value != 0;
    else if (n == "perm_split") c->perm_split = (int32_t)value;
    else if (n == "perm_draw_wave") c->perm_draw_wave = (int32_t)value;
    else if (n == "columns_by_seat") c->columns_by_seat = (int32_t)value;
    else if (n == "pipeline") c->pipeline = (int32_t)value;
    else if (n == "uniform_flags") c->uniform_flags_opt = (int32_t)value;
    else if (n == "flat_handover") c->flat_handover = value != 0 ? 1 : 0;
    else if (n == "matchup_sort_key_mask") c->matchup_sort_mask = (uint64_t)value;
    else if (n == "game_stats_window") c->game_stats_window = std::max<int64_t>(value, 0);
    else if (n == "bootstrap_block") c->bootstrap_block = std::max<int64_t>(value, 0);
    else if (n == "census_chunk_games") c->census_chunk_games = std::max<int64_t>(value, 0);
    else if (n == "agreement_grid") c->agreement_grid = std::max<int64_t>(value, 0);
    else if (n == "performance_grid") c->performance_grid = std::max<int64_t>(value, 0);
    else if (n == "root_windows_grid") c->root_windows_grid = std::max<int64_t>(value, 0);
    else if (n == "rr_window_blocks") {
        if (value < 2 || value > ((int64_t)1 << 22) || (value & 1))
            return fail(c, FK_ERR_ARG, "rr_window_blocks must be even and in [2, 2^22] (a pair's two blocks share a window)");
        c->rr_window_blocks = value;
    }
    else if (n == "rr_keep_roots") {
        if (value != 0 && value != 1) return fail(c, FK_ERR_ARG, "rr_keep_roots is 0 or 1");
        if (c->ri_valid) return fail(c, FK_ERR_ARG, "rr_keep_roots cannot change while counts are resident (fk_rr_counts_reset comes first)");
        c->ri_keep_roots = value != 0;
    }
    else if (n == "block") {
        if (value != 0 && value != 64 && value != 128 && value != 256 && value != 512 && value != 768 && value != 1024)
            return fail(c, FK_ERR_ARG, "block must be 0, 64, 128, 256, 512, 768 (lean records only) or 1024");
        c->block = (int32_t)value;
    } else return fail(c, FK_ERR_ARG, "unknown option %s", name);
    return FK_OK;
}

int fk_rows_wait(fk_ctx *c, int32_t slot) {
    if (!c || slot < 0 || slot >= FK_ROWS_EVENTS) return FK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(c->ev_call_copy[slot]));
    return FK_OK;
}

size_t fk_row_columns_bytes(int32_t k, int32_t games_per_shuffle) {
    return (k < 1 || games_per_shuffle < 1) ? 0 : fksw::shard_image_bytes(k, games_per_shuffle);
}

int fk_write_row_shards(const fk_shard_job *job, int64_t *byte_length, uint8_t *sha256, uint8_t *sidecar_sha256, char *error, size_t error_len) {
    auto say = [&](const std::string &m) {
        if (error && error_len) std::snprintf(error, error_len, "%s", m.c_str());
        return FK_ERR_ARG;
    };
    if (!job || !byte_length || !sha256) return say("job, byte_length and sha256 are required");
    if (!job->shuffle_index || !job->shuffle_seed || !job->batch_id || !job->game_seed || !job->columns || !job->directory || !job->footer_head ||
        !job->footer_kv || !job->footer_orders || !job->leaf_type || !job->leaf_paths)
        return say("a required field of the shard job is null");
    if ((job->side_body != nullptr) != (job->side_full != nullptr) || (job->side_body && (!job->side_directory || !sidecar_sha256)))
        return say("the sidecar template needs body, full, directory and a sidecar_sha256 output");
    fksw::Job j{};
    j.k = job->k; j.gps = job->games_per_shuffle; j.n_shuffles = job->n_shuffles; j.threads = job->threads; j.atomic = job->atomic;
    j.root_seed = job->root_seed; j.rng_purpose_namespace = job->rng_purpose_namespace;
    j.shuffle_index = job->shuffle_index; j.shuffle_seed = job->shuffle_seed; j.batch_id = job->batch_id; j.game_seed = job->game_seed;
    j.columns = static_cast<const uint8_t *>(job->columns); j.shard_stride = job->shard_stride; j.directory = job->directory;
    j.footer_head = job->footer_head; j.footer_head_len = job->footer_head_len; j.footer_kv = job->footer_kv; j.footer_kv_len = job->footer_kv_len;
    j.footer_orders = job->footer_orders; j.footer_orders_len = job->footer_orders_len; j.leaf_type = job->leaf_type; j.leaf_paths = job->leaf_paths;
    j.n_leaves = job->n_leaves; j.side_body = job->side_body; j.side_full = job->side_full; j.side_directory = job->side_directory;
    std::string err;
    if (fksw::write_shards(j, byte_length, sha256, sidecar_sha256, err) != 0) {
        if (error && error_len) std::snprintf(error, error_len, "%s", err.c_str());
        return FK_ERR_IO;
    }
    return FK_OK;
}

int fk_debug_sha256(const void *data, size_t n, uint8_t *out32, int32_t portable) {
    if ((!data && n) || !out32) return FK_ERR_ARG;
    if (portable == 2) { // the two-message form the shard writer uses: data = [first half | second half], out32 = 64 bytes
        const uint8_t *p = static_cast<const uint8_t *>(data);
        fksw::sha256_pair(p, n / 2, out32, p + n / 2, n - n / 2, out32 + 32);
        return FK_OK;
    }
    fksw::sha256(static_cast<const uint8_t *>(data), n, out32, portable != 0);
    return FK_OK;
}

// a lag list (fk_tournament_run_lags, fk_tournament_run_matchups, fk_matchup_reduce): strictly increasing, each in 1 .. 65535
static int check_lags(fk_ctx *c, const int32_t *lags, int32_t n_lags, const char *source) {
    for (int32_t i = 0; i < n_lags; ++i)
        if (lags[i] < 1 || lags[i] > 65535 || (i > 0 && lags[i] <= lags[i - 1]))
            return fail(c, FK_ERR_ARG, "lags must be strictly increasing positive integers%s", source);
    return FK_OK;
}

extern "C++" { // (this part of the file lies inside the C-ABI's extern "C" block)
template <int K>
static void launch_matchup_keys_k(fk_ctx *c, const uint32_t *recs, const uint16_t *perm, uint32_t slots, uint32_t S, uint32_t gps,
                                  uint32_t n_games, uint32_t max_players) {
    hipLaunchKernelGGL(fkm::fk_matchup_keys_kernel<K>, dim3((n_games + 255u) / 256u), dim3(256), 0, c->stream, recs, perm, slots, S, gps, n_games, c->m_ids.p,
                       max_players, c->m_dig.p, c->m_seat.p, c->m_rnd.p);
}
} // extern "C++"

// the key post-pass of one chunk: one instance per seat count (the sorting network is unrolled over K)
static int launch_matchup_keys(fk_ctx *c, uint32_t k, const uint32_t *recs, const uint16_t *perm, uint32_t slots, uint32_t S, uint32_t gps,
                               uint32_t n_games, uint32_t max_players) {
    switch (k) {
#define FKM_CASE(K) case K: launch_matchup_keys_k<K>(c, recs, perm, slots, S, gps, n_games, max_players); break;
        FKM_CASE(1) FKM_CASE(2) FKM_CASE(3) FKM_CASE(4) FKM_CASE(5) FKM_CASE(6) FKM_CASE(7) FKM_CASE(8)
        FKM_CASE(9) FKM_CASE(10) FKM_CASE(11) FKM_CASE(12) FKM_CASE(13) FKM_CASE(14) FKM_CASE(15) FKM_CASE(16)
#undef FKM_CASE
    default: return fail(c, FK_ERR_ARG, "matchup records: k = %u has no key-kernel instance", k);
    }
    HIPCHK(c, hipGetLastError());
    return FK_OK;
}

// hipcub device-wide primitives over the context's one scratch buffer (c->cub), in functions that return `rc` on failure.
// FK_CUB: size query, ensure, the call.  A loop that must not query sizes takes the two halves apart: FK_CUB_NEED raises `need` to what
// a call asks for, the caller ensures c->cub once, FK_CUB_SIZED is the call over the scratch as it stands.
#define FK_CUB_NEED(need, FN, ...)                \
    do {                                          \
        size_t tb_ = 0;                           \
        HIPCHK(c, FN(nullptr, tb_, __VA_ARGS__)); \
        need = std::max<size_t>(need, tb_);       \
    } while (0)
#define FK_CUB_SIZED(FN, ...)                         \
    do {                                              \
        size_t tb_ = c->cub.cap;                      \
        HIPCHK(c, FN(c->cub.p, tb_, __VA_ARGS__));    \
    } while (0)
#define FK_CUB(FN, ...)                                  \
    do {                                                 \
        size_t need_ = 1;                                \
        FK_CUB_NEED(need_, FN, __VA_ARGS__);             \
        if ((rc = ensure(c, c->cub, need_))) return rc;  \
        FK_CUB_SIZED(FN, __VA_ARGS__);                   \
    } while (0)

int fk_matchup_reduce(fk_ctx *c, int32_t k, int64_t n_obs, const uint64_t *digest, const uint16_t *seats, const uint16_t *rounds,
                      const int32_t *lags, int32_t n_lags, int64_t cap, int64_t out_capacity, int64_t *counts, uint64_t *histogram,
                      uint64_t *out_digest, uint16_t *out_seats, int64_t *out_count, int64_t *out_sums) {
    if (!c) return FK_ERR_ARG;
    if (!counts || !histogram || !lags || (n_obs > 0 && (!digest || !seats || !rounds)))
        return fail(c, FK_ERR_ARG, "counts, histogram, lags and (for n_obs > 0) the records are required");
    if (k < 1 || k > (int32_t)fkm::MAX_K) return fail(c, FK_ERR_ARG, "k must be in [1, %u]", fkm::MAX_K);
    if (n_obs < 0 || n_obs > (int64_t)0x7fffffff) return fail(c, FK_ERR_ARG, "n_obs must be in [0, 2^31)");
    if (n_lags < 1 || n_lags > FK_MAX_LAGS) return fail(c, FK_ERR_ARG, "1 <= n_lags <= %d", FK_MAX_LAGS);
    if (int rc_l = check_lags(c, lags, n_lags, "")) return rc_l;
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t n = (uint32_t)n_obs, K = (uint32_t)k, minimum = (uint32_t)lags[0] + 2u, H = minimum + 64u;
    for (int i = 0; i < 4; ++i) counts[i] = 0;
    std::fill(histogram, histogram + H, 0ull);
    counts[0] = n_obs;
    if (n == 0) return FK_OK;
    int rc = 0;
    MatchupReduceBufs &m = c->mr;
    const size_t nK = (size_t)n * K;
    if ((rc = ensure_all(c, m.digest, n, m.seats, nK, m.rounds, n, m.key, n, m.key_alt, n, m.idx, n, m.order, n, m.s_digest, n, m.s_seats, nK, m.s_rounds, n,
                         m.heads, n, m.run_id, n, m.tuple_break, n, m.run_mixed, n, m.mixed_flag, n, m.mixed_pos, n, m.mixed_key, n, m.mixed_key_alt, n,
                         m.mixed_a, n, m.mixed_b, n, m.order_before, n)))
        return rc;
    const hipStream_t st = c->stream;
    const dim3 bn((n + 255u) / 256u), b256(256);
    HIPCHK(c, hipMemcpyAsync(m.digest.p, digest, 8ul * n, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(m.seats.p, seats, 2ul * n * K, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(m.rounds.p, rounds, 2ul * n, hipMemcpyHostToDevice, st));
    // 1. stable radix sort by the (masked) digest: coordinate order is kept inside every run of equal keys
    hipLaunchKernelGGL(fkm::fkm_key_init, bn, b256, 0, st, m.digest.p, (ull)c->matchup_sort_mask, n, m.key.p, m.idx.p);
    HIPCHK(c, hipGetLastError());
    FK_CUB(hipcub::DeviceRadixSort::SortPairs, m.key.p, m.key_alt.p, m.idx.p, m.order.p, (int)n, 0, 64, st);
    hipLaunchKernelGGL(fkm::fkm_gather, bn, b256, 0, st, m.order.p, m.digest.p, m.seats.p, m.rounds.p, n, K, m.s_digest.p, m.s_seats.p, m.s_rounds.p);
    // 2. runs of equal sort key that hold more than one tuple (digest collisions): a stable LSD sort of only those elements by
    //    tuple column k-1 .. 0, then by run, puts every tuple of a run together, each still in coordinate order
    hipLaunchKernelGGL(fkm::fkm_run_heads, bn, b256, 0, st, m.key_alt.p, m.s_seats.p, n, K, m.heads.p, m.tuple_break.p);
    FK_CUB(hipcub::DeviceScan::InclusiveSum, m.heads.p, m.run_id.p, (int)n, st);
    HIPCHK(c, hipMemsetAsync(m.run_mixed.p, 0, 4ul * n, st));
    hipLaunchKernelGGL(fkm::fkm_mark_mixed, bn, b256, 0, st, m.run_id.p, m.tuple_break.p, n, m.run_mixed.p);
    hipLaunchKernelGGL(fkm::fkm_mixed_flags, bn, b256, 0, st, m.run_id.p, m.run_mixed.p, n, m.mixed_flag.p);
    HIPCHK(c, hipGetLastError());
    if ((rc = ensure(c, m.num, 4))) return rc;
    uint32_t *d_num = m.num.p;
    FK_CUB(hipcub::DeviceSelect::Flagged, hipcub::CountingInputIterator<uint32_t>(0u), static_cast<const uint8_t *>(m.mixed_flag.p), m.mixed_pos.p, d_num,
           (int)n, st);
    uint32_t n_mixed = 0;
    HIPCHK(c, hipMemcpyAsync(&n_mixed, d_num, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (n_mixed > 0) {
        const dim3 bm((n_mixed + 255u) / 256u);
        HIPCHK(c, hipMemcpyAsync(m.mixed_a.p, m.mixed_pos.p, 4ul * n_mixed, hipMemcpyDeviceToDevice, st)); // values: positions, ascending
        uint32_t *a = m.mixed_a.p, *b = m.mixed_b.p;
        for (int32_t col = k; col >= 0; --col) { // col = k - 1 .. 0, then the run (col == k is applied LAST: the primary key)
            const uint32_t key_col = col == 0 ? K : (uint32_t)(col - 1);
            hipLaunchKernelGGL(fkm::fkm_mixed_keys, bm, b256, 0, st, a, m.s_seats.p, m.run_id.p, n_mixed, K, key_col, m.mixed_key.p);
            HIPCHK(c, hipGetLastError());
            FK_CUB(hipcub::DeviceRadixSort::SortPairs, m.mixed_key.p, m.mixed_key_alt.p, a, b, (int)n_mixed, 0, key_col == K ? 32 : 16, st);
            std::swap(a, b);
        }
        HIPCHK(c, hipMemcpyAsync(m.order_before.p, m.order.p, 4ul * n, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(fkm::fkm_mixed_apply, bm, b256, 0, st, m.mixed_pos.p, a, m.order_before.p, n_mixed, m.order.p);
        hipLaunchKernelGGL(fkm::fkm_gather, bn, b256, 0, st, m.order.p, m.digest.p, m.seats.p, m.rounds.p, n, K, m.s_digest.p, m.s_seats.p, m.s_rounds.p);
        HIPCHK(c, hipGetLastError());
    }
    // 3. segments = groups (the tuple changes), their starts, counts, eligibility, priorities, histogram bins
    hipLaunchKernelGGL(fkm::fkm_seg_heads, bn, b256, 0, st, m.s_seats.p, n, K, m.heads.p);
    FK_CUB(hipcub::DeviceScan::InclusiveSum, m.heads.p, m.run_id.p, (int)n, st);
    uint32_t G = 0;
    HIPCHK(c, hipMemcpyAsync(&G, m.run_id.p + (n - 1), 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if ((rc = ensure_all(c, m.seg_start, (size_t)G + 1, m.eligible, G, m.prio, G, m.bin, G, m.hist, H, m.sel, G, m.sel_sorted, G, m.prio_sorted, G))) return rc;
    hipLaunchKernelGGL(fkm::fkm_seg_starts, bn, b256, 0, st, m.heads.p, m.run_id.p, n, m.seg_start.p);
    const dim3 bg((G + 255u) / 256u);
    hipLaunchKernelGGL(fkm::fkm_seg_info, bg, b256, 0, st, m.seg_start.p, m.s_digest.p, G, K, minimum, m.eligible.p, m.prio.p, m.bin.p);
    HIPCHK(c, hipGetLastError());
    FK_CUB(hipcub::DeviceHistogram::HistogramEven, static_cast<const int32_t *>(m.bin.p), m.hist.p, (int)(H + 1), 0, (int)H, (int)G, st);
    // 4. selection: the eligible groups by priority (radix sort); the first `cap` and every group tied with the last one kept
    FK_CUB(hipcub::DeviceSelect::Flagged, hipcub::CountingInputIterator<uint32_t>(0u), static_cast<const uint8_t *>(m.eligible.p), m.sel.p, d_num, (int)G, st);
    uint32_t E = 0;
    std::vector<uint32_t> hist32(H);
    HIPCHK(c, hipMemcpyAsync(&E, d_num, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hist32.data(), m.hist.p, 4ul * H, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (uint32_t i = 0; i < H; ++i) histogram[i] = hist32[i];
    counts[1] = G;
    counts[2] = E;
    uint64_t M = E;
    if (E > 0) {
        const dim3 be((E + 255u) / 256u);
        hipLaunchKernelGGL(fkm::fkm_gather_u64, be, b256, 0, st, m.sel.p, m.prio.p, E, m.key_alt.p);
        HIPCHK(c, hipGetLastError());
        FK_CUB(hipcub::DeviceRadixSort::SortPairs, m.key_alt.p, m.prio_sorted.p, m.sel.p, m.sel_sorted.p, (int)E, 0, 64, st);
        if (cap > 0 && (uint64_t)cap < E) {
            M = (uint64_t)cap;
            ull last = 0;
            HIPCHK(c, hipMemcpyAsync(&last, m.prio_sorted.p + (M - 1), 8, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            std::vector<ull> more(4096);
            while (M < E) { // ties on the 64-bit priority: the host breaks them by the rest of the tuple
                const uint64_t take = std::min<uint64_t>(more.size(), E - M);
                HIPCHK(c, hipMemcpy(more.data(), m.prio_sorted.p + M, 8 * take, hipMemcpyDeviceToHost));
                uint64_t j = 0;
                while (j < take && more[j] == last) ++j;
                M += j;
                if (j < take) break;
            }
        }
    }
    counts[3] = (int64_t)M;
    if ((int64_t)M > out_capacity) return fail(c, FK_ERR_ARG, "fk_matchup_reduce: %llu groups selected, out_capacity is %lld", (unsigned long long)M, (long long)out_capacity);
    if (M == 0) return FK_OK;
    if (!out_digest || !out_seats || !out_count || !out_sums) return fail(c, FK_ERR_ARG, "the output arrays are required");
    const size_t n_sums = (size_t)M * n_lags * fkm::SUM_COLS;
    if ((rc = ensure_all(c, m.out_digest, M, m.out_seats, (size_t)M * K, m.out_count, M, m.out_sums, n_sums, m.lags, (size_t)n_lags))) return rc;
    HIPCHK(c, hipMemcpyAsync(m.lags.p, lags, 4ul * n_lags, hipMemcpyHostToDevice, st));
    // 5. the lag sums of the selected groups: one wave per group
    hipLaunchKernelGGL(fkm::fkm_group_sums, dim3((unsigned)((M * 64 + 255) / 256)), b256, 0, st, m.sel_sorted.p, (uint32_t)M, m.seg_start.p, m.s_digest.p,
                       m.s_seats.p, m.s_rounds.p, K, m.lags.p, (uint32_t)n_lags, m.out_digest.p, m.out_seats.p, m.out_count.p, m.out_sums.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_digest, m.out_digest.p, 8ul * M, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out_seats, m.out_seats.p, 2ul * M * K, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out_count, m.out_count.p, 8ul * M, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out_sums, m.out_sums.p, 8 * n_sums, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FK_OK;
}
// The pair reduce of fk_tournament_run_seat_counts over the call's n mirror records (c->sa.key, c->sa.val), on the context's stream
// with no host round trip: pair_rank [capacity][2], pair_sums [capacity][6], pair_count.
static int mirror_reduce(fk_ctx *c, uint32_t n, uint64_t capacity) {
    int rc = 0;
    SeatBufs &s = c->sa;
    const size_t n1 = (size_t)n + 1, rows = std::max<size_t>((size_t)capacity, 1);
    if ((rc = ensure_all(c, s.fr, n1, s.e_fr, n1, s.sh, n1, s.e_sh, n1, s.ph, n1, s.e_ph, n1, s.seg_start, n1, s.pair_start, n1, s.seg_diff, n1,
                         s.pair_rank, rows * 2, s.pair_sums, rows * fksa::PAIR_COLS, s.pair_count, 1)))
        return rc;
    const hipStream_t st = c->stream;
    const dim3 bn((unsigned)((n1 + 255u) / 256u)), b256(256);
    FK_CUB(hipcub::DeviceRadixSort::SortPairs, s.key.p, s.key_sorted.p, s.val.p, s.val_sorted.p, (int)n, 0, 64, st);
    hipLaunchKernelGGL(fksa::fk_mirror_flags_kernel, bn, b256, 0, st, s.key_sorted.p, s.val_sorted.p, n, s.fr.p, s.sh.p, s.ph.p);
    HIPCHK(c, hipGetLastError());
    FK_CUB(hipcub::DeviceScan::ExclusiveSum, s.fr.p, s.e_fr.p, (int)n1, st);
    FK_CUB(hipcub::DeviceScan::ExclusiveSum, s.sh.p, s.e_sh.p, (int)n1, st);
    FK_CUB(hipcub::DeviceScan::ExclusiveSum, s.ph.p, s.e_ph.p, (int)n1, st);
    HIPCHK(c, hipMemsetAsync(s.seg_diff.p, 0, 4 * n1, st));
    hipLaunchKernelGGL(fksa::fk_mirror_starts_kernel, bn, b256, 0, st, s.sh.p, s.e_sh.p, s.ph.p, s.e_ph.p, n, s.seg_start.p, s.pair_start.p);
    hipLaunchKernelGGL(fksa::fk_mirror_segment_kernel, bn, b256, 0, st, s.key_sorted.p, s.val_sorted.p, n, s.e_fr.p, s.e_sh.p, s.seg_start.p, s.seg_diff.p);
    hipLaunchKernelGGL(fksa::fk_mirror_pair_sum_kernel, bn, b256, 0, st, s.key_sorted.p, s.e_fr.p, s.e_sh.p, s.e_ph.p, n, s.seg_start.p, s.pair_start.p,
                       s.seg_diff.p, (ull)capacity, s.pair_rank.p, s.pair_sums.p, s.pair_count.p);
    HIPCHK(c, hipGetLastError());
    return FK_OK;
}

// The tournament call path: an entry point checks its own arguments and fills a TournamentCall on its stack; tournament_call plays it
// through the driver below, once or again on one of its three replays.  Nothing that describes the call in progress is in the context.
static int tournament_run_impl(fk_ctx *c, const TournamentCall &call) {
    const fk_strategy *strategies = call.strategies;
    const int32_t S = call.S, k = call.k, target_score = call.target_score, max_rounds = call.max_rounds, n_ov = call.n_ov;
    const uint64_t root_seed = call.root_seed, shuffle_begin = call.shuffle_begin, shuffle_end = call.shuffle_end;
    const uint32_t shuffles_per_batch = call.shuffles_per_batch;
    const fk_override *ov = call.ov;
    const LagReq *lag = call.lag;
    int64_t *tally = call.tally, *seat_stats = call.seat_stats;
    void *rows = call.rows;
    int32_t *perms = call.perms;
    double *seat_ratios = call.seat_ratios;
    if (!strategies || !tally) return fail(c, FK_ERR_ARG, "strategies and tally are required");
    int rc = check_seating(c, S, k);
    if (rc) return rc;
    if (rows != nullptr && call.columns_ids != nullptr && k > 64)
        return fail(c, FK_ERR_ARG, "column images hold tables of at most 64 seats, got %d", (int)k);
    if ((rc = check_range(c, S, max_rounds, shuffle_begin, shuffle_end, shuffles_per_batch, ov, n_ov))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);

    const uint64_t n_sh_total = shuffle_end - shuffle_begin;
    const uint32_t gps = (uint32_t)(S / k);
    const uint64_t n_batches = (n_sh_total + shuffles_per_batch - 1) / shuffles_per_batch;
    const size_t tally_bytes = sizeof(int64_t) * (size_t)n_batches * (size_t)S * FK_TALLY_COLS;
    if (n_sh_total == 0) return FK_OK;
    const size_t row_bytes = sizeof(fk_row_hdr) + sizeof(fk_seat) * (size_t)k;
    const bool columns = rows != nullptr && call.columns_ids != nullptr; // fk_tournament_run_columns
    const size_t rows_per_shuffle = columns ? fksw::shard_image_bytes(k, (int)gps) : (size_t)gps * row_bytes;

    if ((rc = upload_strategies(c, strategies, S))) return rc;
    if (columns) {
        if ((rc = ensure(c, c->ids, (size_t)S))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->ids.p, call.columns_ids, sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = ensure(c, c->tally, tally_bytes / 8))) return rc;
    HIPCHK(c, hipMemsetAsync(c->tally.p, 0, tally_bytes, c->stream));

    LaunchPlan plan = plan_play(plan_knobs(c), PLAN_TOURNAMENT, k, S, n_batches == 1, target_score);
    if (plan.block == 0)
        return fail(c, FK_ERR_ARG, "target_score %d: no kernel instance (lean records hold totals up to %d points; %d full records do not fit LDS)",
                    target_score, 50 * LEAN_MAX_TARGET50, (int)k);
    if (plan.shape().hc) c->ran_hc = true;
    if (plan.shape().hc && !plan.shape().cl) { // cold seat records of every lane the grid can seat
        if ((rc = ensure(c, c->cold, (size_t)plan.grid * (size_t)plan.block * (size_t)k))) return rc;
    }
    const GameStatsReq *gst = call.gstats; // fk_tournament_run_game_stats (null otherwise)
    const RareReq *rare = gst ? call.rare : nullptr; // fk_tournament_run_rare_events
    const SeatReq *sq = call.seats; // fk_tournament_run_seat_counts
    const bool want_state = rows != nullptr || seat_stats != nullptr || gst != nullptr;
    const bool want_recs = !plan.lds_tally || want_state || lag != nullptr;
    const size_t stats_bytes = sizeof(int64_t) * (size_t)n_batches * (size_t)S * FK_SEAT_STAT_COLS;
    if (seat_stats) {
        if ((rc = ensure(c, c->stats, stats_bytes / 8))) return rc;
        HIPCHK(c, hipMemsetAsync(c->stats.p, 0, stats_bytes, c->stream));
    }
    const size_t sq_bytes = sizeof(int64_t) * (size_t)n_batches * (size_t)S * (size_t)k * fksa::COUNT_COLS;
    const uint32_t sq_n = sq && sq->id_rank ? (uint32_t)(n_sh_total * gps) : 0u; // mirror records of the call (the entry bounds the range)
    if (sq) {
        if ((rc = ensure(c, c->sa.counts, sq_bytes / 8))) return rc;
        HIPCHK(c, hipMemsetAsync(c->sa.counts.p, 0, sq_bytes, c->stream));
    }
    if (sq_n) { // id ranks, the call's mirror records: keys and payloads, two sort buffers each
        const size_t n = sq_n;
        if ((rc = ensure_all(c, c->sa.id_rank, (size_t)S, c->sa.key, n, c->sa.key_sorted, n, c->sa.val, n, c->sa.val_sorted, n))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->sa.id_rank.p, sq->id_rank, 2ul * (size_t)S, hipMemcpyHostToDevice, c->stream));
    }
    const size_t ratio_bytes = sizeof(double) * (size_t)n_batches * (size_t)S * FK_SEAT_RATIO_COLS;
    if (seat_ratios) { // running float64 sums, carried from chunk to chunk on the device (all-zero bits = 0.0)
        if ((rc = ensure(c, c->ratios, ratio_bytes / 8))) return rc;
        HIPCHK(c, hipMemsetAsync(c->ratios.p, 0, ratio_bytes, c->stream));
    }

    // chunk planning: whole shuffles per chunk inside the workspace budget
    const size_t bytes_per_shuffle = (size_t)S * 2 + (size_t)gps * (game_workspace_bytes(k, plan.shape().gs || want_state, want_recs, rows != nullptr) +
                                                                    (seat_stats ? (size_t)k * 32 : 0)) // + the exposure digests
                                     + (lag ? (size_t)S * 2 : 0)                                         // + the lag value matrix row
                                     + (lag && lag->m_digest ? (size_t)gps * (10 + 2 * (size_t)k) : 0)   // + the matchup records
                                     + (gst ? (size_t)gps * 16 : 0)                                       // + the game-stat records
                                     + (rare ? (size_t)gps * 4 + ((size_t)gps + 255) / 256 * 12 : 0);     // + second scores, workgroup counts / bases
    // (column images are larger than AoS rows: the workspace figure above counts 4 + 28 k bytes per game)
    uint64_t chunk_sh = std::max<uint64_t>(1, (uint64_t)workspace_budget(c) / bytes_per_shuffle);
    chunk_sh = std::min<uint64_t>(chunk_sh, (uint64_t)0x7fffffff / gps);
    if (rows) // rows mode: several chunks per call, so that the rows of chunk i cross PCIe while chunk i + 1 plays
        chunk_sh = std::min<uint64_t>(chunk_sh, std::max<uint64_t>(1, (uint64_t)c->rows_chunk_games / gps));
    chunk_sh = std::min<uint64_t>(chunk_sh, n_sh_total);

    const hipEvent_t t0 = c->ev[SLOT_CALL], t1 = c->ev[SLOT_CALL + 1];
    HIPCHK(c, hipEventRecord(t0, c->stream));

    // lag statistics (fk_tournament_run_lags): V = [max_lag carry rows][chunk rows] x S values, sums [S][n_lags][11]
    const uint32_t L = lag ? (uint32_t)lag->max_lag : 0u;
    const uint32_t edge_rows = lag ? (uint32_t)std::min<uint64_t>(L, n_sh_total) : 0u;
    const size_t lag_sum_bytes = lag ? sizeof(int64_t) * (size_t)S * (size_t)lag->n_lags * FK_LAG_COLS : 0;
    uint32_t head_filled = 0;
    if (lag) {
        if ((rc = ensure_all(c, c->lag_v, ((size_t)L + chunk_sh) * (size_t)S, c->lag_out, lag_sum_bytes / 8, c->lag_lags, (size_t)lag->n_lags, c->lag_edge,
                             2 * (size_t)std::max<uint32_t>(edge_rows, 1) * (size_t)S, c->lag_tmp, (size_t)std::max<uint32_t>(L, 1) * (size_t)S)))
            return rc;
        HIPCHK(c, hipMemsetAsync(c->lag_out.p, 0, lag_sum_bytes, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->lag_lags.p, lag->lags, sizeof(int32_t) * (size_t)lag->n_lags, hipMemcpyHostToDevice, c->stream));
    }
    if (lag && lag->m_digest) { // matchup records of one chunk (copied to the caller's arrays behind it)
        const size_t n = (size_t)chunk_sh * gps;
        if ((rc = ensure_all(c, c->m_ids, (size_t)S, c->m_dig, n, c->m_seat, n * (size_t)k, c->m_rnd, n))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->m_ids.p, lag->ids, sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, c->stream));
    }

    // game statistics (fk_tournament_run_game_stats): g_out in the layout `go`
    const uint32_t g_rb = gst ? gst->rounds_bins : 0u, g_mb = gst ? gst->margin_bins : 0u;
    const uint32_t g_wr = c->game_stats_window > 0 ? (uint32_t)std::min<int64_t>(g_rb, c->game_stats_window) : g_rb;
    const uint32_t g_wm = c->game_stats_window > 0 ? (uint32_t)std::min<int64_t>(g_mb, c->game_stats_window) : g_mb;
    const fkl::GameStatsOut go((size_t)S, g_rb, g_mb);
    fkg::Spill g_spill{};
    if (gst) {
        if ((rc = ensure_all(c, c->g_rec, (size_t)chunk_sh * gps, c->g_out, go.bytes(gst->spill_capacity)))) return rc;
        HIPCHK(c, hipMemsetAsync(c->g_out.p, 0, go.spill_at(), c->stream));
        g_spill.count = c->g_out.as<ull>() + go.spill_count;
        g_spill.entries = c->g_out.as<int32_t>(go.spill_at());
        g_spill.cap = (uint64_t)gst->spill_capacity;
    }

    // rare events (fk_tournament_run_rare_events): r_out in the layout `ro`
    const uint32_t r_sb = rare ? rare->second_bins : 0u;
    const uint32_t r_ws = c->game_stats_window > 0 ? (uint32_t)std::min<int64_t>(r_sb, c->game_stats_window) : r_sb;
    const fkl::RareOut ro((size_t)S, r_sb);
    if (rare) {
        const size_t max_blocks = ((size_t)chunk_sh * gps + fkre::COUNT_BLOCK - 1) / fkre::COUNT_BLOCK;
        if ((rc = ensure_all(c, c->r_sec, (size_t)chunk_sh * gps, c->r_out, ro.n_u64))) return rc;
        HIPCHK(c, hipMemsetAsync(c->r_out.p, 0, ro.n_u64 * 8, c->stream));
        if (rare->events) {
            const size_t room = (size_t)std::max<int64_t>(rare->event_capacity, 1);
            if ((rc = ensure_all(c, c->r_blk, max_blocks, c->r_base, max_blocks, c->r_head, room, c->r_seats, room * (size_t)k))) return rc;
        }
    }

    const uint32_t slots = perm_slots(S);
    const uint32_t state_dw = (plan.shape().gs || want_state) ? STATE_DW : 4u;
    auto describe = [&](uint64_t first_shuffle, uint32_t count, uint32_t dw) {
        return ChunkDesc{c->table_epoch, root_seed, first_shuffle, count, (uint32_t)S, (uint32_t)k, dw, c->longest_first ? 1u : 0u, slots};
    };
    // the hint (fk_tournament_hint_next) is for the call that FOLLOWS this one
    const bool hinted = c->hint_valid && c->hint_end > c->hint_begin;
    const uint64_t hint_begin = c->hint_begin, hint_end = c->hint_end;
    const uint32_t hint_dw = (plan.shape().gs || c->hint_state) ? STATE_DW : 4u;
    c->hint_valid = false;

    std::vector<uint16_t> perm_host;
    bool deferred = false;
    int64_t deferred_base = 0;
    for (uint64_t done = 0; done < n_sh_total; done += chunk_sh) {
        const uint32_t n_sh = (uint32_t)std::min<uint64_t>(chunk_sh, n_sh_total - done);
        const uint64_t sh0 = shuffle_begin + done;
        const uint32_t n_games = n_sh * gps;
        const uint32_t perm_blocks = (n_sh + slots - 1u) / slots;
        const uint32_t first_batch = (uint32_t)(done / shuffles_per_batch); // the batches the chunk touches
        const uint32_t nb = (uint32_t)((done + n_sh - 1) / shuffles_per_batch) - first_batch + 1u;

        // the chunk's preparation: already made on the side stream (by the previous chunk, or by the previous call after a
        // hint), or made now in front of the game kernel
        const ChunkDesc d = describe(sh0, n_sh, state_dw);
        int ready_set = -1;
        for (int si : {c->cur ^ 1, c->cur})
            if (c->sets[si].prepared && c->sets[si].desc == d) ready_set = si;
        // A chunk prepared on the side stream: its seat seeding may still be running in the previous game kernel's drain tail.
        // The main stream waits for it only in front of THIS chunk's game kernel (below) — what is enqueued before that point,
        // the next chunk's permutation kernels above all, runs beside the seeding's tail instead of behind it.
        bool wait_ready = false;
        if (ready_set >= 0) {
            c->cur = ready_set;
            wait_ready = true;
        } else {
            if (c->sets[c->cur].prepared) c->cur ^= 1; // keep a prepared (hinted) chunk for its own call if there is room
            if ((rc = prep_tournament_chunk(c, c->cur, c->stream, d, CSET(c).sa))) return rc;
        }
        CSET(c).prepared = false; // consumed
        const SeedArgs sa = CSET(c).sa;
        if (perms) {
            if (wait_ready) HIPCHK(c, hipStreamWaitEvent(c->stream, CSET(c).ready, 0));
            wait_ready = false;
            perm_host.resize((size_t)perm_blocks * S * slots);
            HIPCHK(c, hipMemcpyAsync(perm_host.data(), CSET(c).perm.p, perm_host.size() * 2, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (uint32_t s = 0; s < n_sh; ++s)
                for (int32_t i = 0; i < S; ++i)
                    perms[(size_t)(done + s) * S + i] = perm_host[((size_t)(s / slots) * S + i) * slots + s % slots];
        }

        // overrides that fall into this chunk -> chunk-local game ids
        uint32_t n_dov = 0;
        if ((rc = map_tournament_overrides(c, ov, n_ov, root_seed, k, sh0, n_sh, gps, n_dov))) return rc;
        // the device row buffers alternate over chunks — and, in async mode, over calls: a one-chunk call's row kernel then has not to wait for the previous call's copy
        const int rb = (int)((done / chunk_sh + (c->rows_async ? c->rows_calls : 0u)) & 1u);
        Dev<uint8_t> &row_buf = rb ? c->rows_alt : c->rows;
        if (rows) {
            if ((size_t)n_sh * rows_per_shuffle > row_buf.cap) HIPCHK(c, hipStreamSynchronize(c->copy_stream)); // growing: no copy may be reading it
            if ((rc = ensure(c, row_buf, (size_t)n_sh * rows_per_shuffle))) return rc;
        }

        PlayArgs pa = table_args(c, target_score, max_rounds);
        pa.perm_T = CSET(c).perm.p;
        pa.perm_slots = slots;
        pa.seat_strategy = nullptr;
        pa.tally = c->tally.p;
        pa.ov = c->ov.p;
        pa.n_ov = n_dov;
        pa.mode = MODE_PERM;
        pa.n_games = n_games;
        pa.gps = gps;
        pa.n_sh = n_sh;
        pa.k = (uint32_t)k;
        pa.S = (uint32_t)S;
        pa.cold = c->cold.p;

        // The next chunk (or the hinted next call) is prepared into the other chunk set around this game kernel: its permutations
        // in front of it on the main stream, its schedule + seat seeding on the low-priority stream while it runs.
        HIPCHK(c, hipEventRecord(c->main_idle, c->stream)); // everything that used the other chunk set is in front of this point
        if (c->pipeline) {
            ChunkDesc next{};
            bool have_next = false;
            if (done + chunk_sh < n_sh_total) {
                next = describe(sh0 + n_sh, (uint32_t)std::min<uint64_t>(chunk_sh, n_sh_total - done - chunk_sh), state_dw);
                have_next = true;
            } else if (hinted) {
                next = describe(hint_begin, (uint32_t)std::min<uint64_t>(chunk_sh, hint_end - hint_begin), hint_dw);
                have_next = true;
            }
            if (have_next) {
                if ((rc = prep_tournament_chunk(c, c->cur ^ 1, c->prep_stream, next, c->sets[c->cur ^ 1].sa))) return rc;
            }
        }
        if (wait_ready) HIPCHK(c, hipStreamWaitEvent(c->stream, c->sets[c->cur].ready, 0));
        if ((rc = launch_play_stage(c, sa, pa, plan, want_state, want_recs || sq != nullptr, want_recs))) return rc;
        // The last chunk of a call without rows: its error record travels with the tally, behind the post-passes — one host
        // round trip per call instead of two (the post-passes only read; on an error their output is discarded).
        const bool defer_check = done + chunk_sh >= n_sh_total && !rows && c->err_host && !pa.hcount; // (measuring builds read their counts in finish_play)
        if (defer_check) {
            HIPCHK(c, hipMemcpyAsync(c->err_host, pa.err, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            deferred = true;
            deferred_base = (int64_t)done * gps;
        } else {
            if ((rc = finish_play(c, pa, (int64_t)done * gps, "tournament"))) return rc;
        }
        const bool scheduled = c->longest_first != 0;
        const uint32_t *inv = nullptr; // game id -> slot of its state records
        if (want_state && scheduled) {
            if ((rc = ensure(c, c->inv, (size_t)n_games))) return rc;
            hipLaunchKernelGGL(fk_invert_sched_kernel, dim3((n_games + 255u) / 256u), dim3(256), 0, c->stream, CSET(c).order.p, n_games, c->inv.p);
            inv = c->inv.p;
        }
        const uint16_t *inv_perm = nullptr;
        if (seat_stats || gst || sq) { // the draws buffer is free again: inverse permutations
            if ((rc = ensure(c, CSET(c).draws, (size_t)perm_blocks * S * slots * 2))) return rc;
            const uint32_t cells = perm_blocks * (uint32_t)S * slots;
            hipLaunchKernelGGL(fk_invert_perm_kernel, dim3((cells + 255u) / 256u), dim3(256), 0, c->stream, CSET(c).perm.p, (uint32_t)S, slots, n_sh,
                               CSET(c).draws16());
            inv_perm = CSET(c).draws16();
        }
        if (gst) {
            // phase 1, game-major: one 16-byte record per game + the game-level histograms; phase 2 gathers them per strategy
            ull *o = c->g_out.as<ull>();
            const uint32_t rec_grid = std::max<uint32_t>(1u, std::min<uint32_t>((n_games + 255u) / 256u, 2048u));
            hipLaunchKernelGGL(fkg::fk_game_record_kernel, dim3(rec_grid), dim3(256), (size_t)(g_wr + g_wm + fkg::N_COUNTS) * 4, c->stream,
                               CSET(c).state.p, c->recs.p, inv, n_games, gps, n_sh, (uint32_t)k, gst->rare_target, g_wr, g_wm, c->g_rec.p,
                               o + go.g_counts, o + go.g_rounds, o + go.g_runner, g_spill);
            // (strategy, segment) workgroups: enough of them to fill the chip, at least 256 shuffles (one per lane) per segment
            const uint32_t want_seg = std::max<uint32_t>(1u, (2048u + (uint32_t)S - 1u) / (uint32_t)S);
            const uint32_t rows_per_seg = std::max<uint32_t>(256u, (n_sh + want_seg - 1u) / want_seg);
            const uint32_t n_seg = (n_sh + rows_per_seg - 1u) / rows_per_seg;
            hipLaunchKernelGGL(fkg::fk_game_stats_gather_kernel, dim3((uint32_t)S, n_seg), dim3(256), (size_t)(g_wr + 2 * g_wm + fkg::N_COUNTS) * 4,
                               c->stream, c->g_rec.p, inv_perm, slots, (uint32_t)S, (uint32_t)k, gps, n_sh, rows_per_seg, g_wr, g_wm, g_rb, g_mb,
                               o + go.s_counts, o + go.s_rounds, o + go.s_runner, o + go.s_spread, g_spill);
            HIPCHK(c, hipGetLastError());
            if (rare) {
                ull *r = c->r_out.p;
                if (k >= 2) { // one seat has no second score: it contributes nothing
                    hipLaunchKernelGGL(fkre::fk_second_score_kernel, dim3(rec_grid), dim3(256), (size_t)r_ws * 4, c->stream, CSET(c).state.p, inv,
                                       n_games, gps, n_sh, (uint32_t)k, r_ws, c->r_sec.p, r + ro.g_second, g_spill);
                    hipLaunchKernelGGL(fkre::fk_second_gather_kernel, dim3((uint32_t)S, n_seg), dim3(256), (size_t)r_ws * 4, c->stream, c->r_sec.p,
                                       inv_perm, slots, (uint32_t)S, (uint32_t)k, gps, n_sh, rows_per_seg, r_ws, r_sb, r + ro.s_second, g_spill);
                }
                if (rare->events) { // ordered compaction of the flagged games: count per workgroup, scan from the running total, scatter
                    const uint32_t n_blk = (n_games + fkre::COUNT_BLOCK - 1u) / fkre::COUNT_BLOCK;
                    hipLaunchKernelGGL(fkre::fk_event_count_kernel, dim3(n_blk), dim3(fkre::COUNT_BLOCK), 0, c->stream, c->g_rec.p, n_games,
                                       rare->thr, c->r_blk.p);
                    hipLaunchKernelGGL(fkre::fk_event_scan_kernel, dim3(1), dim3(fkre::SCAN_BLOCK), 0, c->stream, c->r_blk.p, n_blk, r + ro.total, c->r_base.p);
                    hipLaunchKernelGGL(fkre::fk_event_scatter_kernel, dim3(n_blk), dim3(fkre::COUNT_BLOCK), 0, c->stream, c->g_rec.p, CSET(c).perm.p,
                                       slots, (uint32_t)S, (uint32_t)k, gps, n_games, (uint32_t)done, rare->thr, c->r_base.p,
                                       (ull)rare->event_capacity, c->r_head.p, c->r_seats.p);
                }
                HIPCHK(c, hipGetLastError());
            }
        }
        if (sq) { // seat counts from rec0 through the inverse permutation; at k = 2 the chunk's mirror records
            const uint32_t s_blocks = ((uint32_t)S + fksa::COUNT_BLOCK - 1u) / fksa::COUNT_BLOCK;
            const uint32_t ppb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(shuffles_per_batch, n_sh) / 8, (4096u + nb * s_blocks - 1u) / (nb * s_blocks)));
            hipLaunchKernelGGL(fksa::fk_seat_counts_kernel, dim3(s_blocks, nb * ppb), dim3(fksa::COUNT_BLOCK),
                               (size_t)k * fksa::COUNT_COLS * fksa::COUNT_BLOCK * 4, c->stream, c->rec0.p, inv_perm, slots, (uint32_t)S, (uint32_t)k, gps,
                               n_sh, (uint32_t)done, shuffles_per_batch, ppb, first_batch, c->sa.counts.p);
            if (sq_n)
                hipLaunchKernelGGL(fksa::fk_mirror_record_kernel, dim3((n_games + 255u) / 256u), dim3(256), 0, c->stream, c->rec0.p, CSET(c).perm.p,
                                   slots, (uint32_t)S, gps, n_games, (uint32_t)done, shuffles_per_batch, c->sa.id_rank.p, (uint32_t)(done * gps),
                                   c->sa.key.p, c->sa.val.p);
            HIPCHK(c, hipGetLastError());
        }
        if (seat_stats) {
            const uint32_t s_blocks = ((uint32_t)S + 255u) / 256u;
            // enough (strategy block, batch, part) workgroups to fill the chip; a part is at least 8 shuffles
            const uint32_t ppb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(shuffles_per_batch, n_sh) / 8, (4096u + nb * s_blocks - 1u) / (nb * s_blocks)));
            // phase 1, game-major: one 32-byte digest per exposure; phase 2 gathers them per strategy
            if ((rc = ensure(c, c->digest, (size_t)n_games * k * 2))) return rc;
            const size_t pairs = (size_t)n_games * k;
            hipLaunchKernelGGL(fk_seat_digest_kernel, dim3((unsigned)((pairs + 255u) / 256u)), dim3(256), 0, c->stream, CSET(c).state.p, c->recs.p, inv,
                               n_games, gps, n_sh, (uint32_t)k, c->digest.p);
            hipLaunchKernelGGL(fk_seat_stats_kernel, dim3(s_blocks, nb * ppb), dim3(256), 0, c->stream, c->digest.p, inv_perm, slots, (uint32_t)S,
                               (uint32_t)k, gps, n_sh, (uint32_t)done, shuffles_per_batch, ppb, first_batch, c->stats.p);
            if (seat_ratios) // the four float64 sums: one thread per (strategy, batch), the batch's shuffles of this chunk in order
                hipLaunchKernelGGL(fk_seat_ratio_kernel, dim3(s_blocks, nb), dim3(256), 0, c->stream, c->digest.p, inv_perm, slots, (uint32_t)S,
                                   (uint32_t)k, gps, n_sh, (uint32_t)done, shuffles_per_batch, first_batch, c->ratios.p);
            HIPCHK(c, hipGetLastError());
        }
        if (lag) {
            uint16_t *V = c->lag_v.p;
            const size_t row = (size_t)S; // values per row
            const uint32_t carry = (uint32_t)std::min<uint64_t>(done, L);
            hipLaunchKernelGGL(fk_lag_values_kernel, dim3((unsigned)(((size_t)n_games * k + 255u) / 256u)), dim3(256), 0, c->stream, c->recs.p,
                               CSET(c).perm.p, slots, (uint32_t)S, (uint32_t)k, gps, n_games, V + (size_t)L * row);
            const uint32_t s_blocks = ((uint32_t)S + 255u) / 256u;
            // enough (strategy block, segment) workgroups to fill the chip, at least 64 rows per segment
            const uint32_t want_seg = std::max<uint32_t>(1u, (2048u + s_blocks - 1u) / s_blocks);
            const uint32_t rows_per_seg = std::max<uint32_t>(64u, (n_sh + want_seg - 1u) / want_seg);
            const uint32_t n_seg = (n_sh + rows_per_seg - 1u) / rows_per_seg;
            hipLaunchKernelGGL(fk_lag_sums_kernel, dim3(s_blocks, n_seg), dim3(256), 0, c->stream, V, (uint32_t)S, L - carry, L, L + n_sh,
                               rows_per_seg, c->lag_lags.p, (uint32_t)lag->n_lags, c->lag_out.p);
            HIPCHK(c, hipGetLastError());
            if (lag->m_digest) {
                rc = launch_matchup_keys(c, (uint32_t)k, c->recs.p, CSET(c).perm.p, slots, (uint32_t)S, gps, n_games, (uint32_t)lag->max_players);
                if (rc) return rc;
                const size_t g0 = (size_t)done * gps;
                HIPCHK(c, hipMemcpyAsync(lag->m_digest + g0, c->m_dig.p, (size_t)n_games * 8, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipMemcpyAsync(lag->m_seats + g0 * k, c->m_seat.p, (size_t)n_games * 2 * k, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipMemcpyAsync(lag->m_rounds + g0, c->m_rnd.p, (size_t)n_games * 2, hipMemcpyDeviceToHost, c->stream));
            }
            uint16_t *edge = c->lag_edge.p;
            if (head_filled < edge_rows) { // the first rows of the call's range (they may span chunks shorter than the largest lag)
                const uint32_t take = std::min<uint32_t>(edge_rows - head_filled, n_sh);
                HIPCHK(c, hipMemcpyAsync(edge + (size_t)head_filled * row, V + (size_t)L * row, (size_t)take * row * 2, hipMemcpyDeviceToDevice, c->stream));
                head_filled += take;
            }
            if (done + chunk_sh >= n_sh_total) { // last chunk: the last rows of the range (carry rows + this chunk's)
                HIPCHK(c, hipMemcpyAsync(edge + (size_t)edge_rows * row, V + ((size_t)L + n_sh - edge_rows) * row, (size_t)edge_rows * row * 2,
                                         hipMemcpyDeviceToDevice, c->stream));
            } else { // the next chunk's carry = the last L rows of [carry | chunk] (through a scratch copy: the ranges may overlap)
                HIPCHK(c, hipMemcpyAsync(c->lag_tmp.p, V + (size_t)n_sh * row, (size_t)L * row * 2, hipMemcpyDeviceToDevice, c->stream));
                HIPCHK(c, hipMemcpyAsync(V, c->lag_tmp.p, (size_t)L * row * 2, hipMemcpyDeviceToDevice, c->stream));
            }
        }
        if (!plan.lds_tally) { // result records -> per-batch tallies
            const uint64_t games_per_batch = (uint64_t)shuffles_per_batch * gps;
            if (games_per_batch >= 4096) {
                // 896 x 22 x 8 B = 154 KiB of LDS: one 1024-thread workgroup per CU, half as many passes over rec0 as two
                // smaller ones would need
                const uint32_t slice = (uint32_t)std::min<int64_t>(S, 896);
                const uint32_t n_slices = ((uint32_t)S + slice - 1u) / slice;
                // enough parts to fill the chip, at least ~16 K games each
                uint32_t ppb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(games_per_batch / 16384, (2048u + nb * n_slices - 1u) / (nb * n_slices)));
                static int reduce_configured = -1;
                if (reduce_configured != c->device) {
                    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&fk_tally_reduce_kernel),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT));
                    reduce_configured = c->device;
                }
                hipLaunchKernelGGL(fk_tally_reduce_kernel, dim3(ppb * nb, n_slices), dim3(REDUCE_BLOCK), (size_t)slice * RT_COLS * 8, c->stream,
                                   c->rec0.p, c->recs.p, n_games, gps, (uint32_t)k, (uint32_t)S, CSET(c).perm.p, slots, (uint32_t)done,
                                   shuffles_per_batch, n_sh, ppb, slice, first_batch, c->tally.p);
            } else {
                hipLaunchKernelGGL(fk_tally_direct_kernel, dim3((n_games + 255u) / 256u), dim3(256), 0, c->stream, c->recs.p, n_games, gps,
                                   (uint32_t)k, (uint32_t)S, CSET(c).perm.p, slots, (uint32_t)done, shuffles_per_batch, c->tally.p);
            }
            HIPCHK(c, hipGetLastError());
        }
        if (rows) {
            // rows kernel on the main stream (behind this buffer's previous copy), the copy to the host on the copy stream: it
            // runs beside the next chunk's game kernel.  With a pinned destination (fk_host_alloc) it is one DMA at PCIe rate.
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_copy[rb], 0));
            if (columns && k <= 16 && c->columns_by_seat != 0) {
                hipLaunchKernelGGL(fk_row_columns_seats_kernel, dim3((n_games + 63u) / 64u), dim3(64u * (uint32_t)k), 0, c->stream, CSET(c).state.p,
                                   c->recs.p, inv, n_games, gps, n_sh, (uint32_t)k, 1u, c->ids.p, row_buf.p, rows_per_shuffle);
                HIPCHK(c, hipGetLastError());
            } else if (columns) {
                hipLaunchKernelGGL(fk_row_columns_kernel, dim3((n_games + 255u) / 256u), dim3(256), 0, c->stream, CSET(c).state.p, c->recs.p, inv,
                                   n_games, gps, n_sh, (uint32_t)k, 1u, c->ids.p, row_buf.p, rows_per_shuffle);
                HIPCHK(c, hipGetLastError());
            } else {
                if ((rc = rows_pass(c, sa, scheduled, n_games, gps, n_sh, true, row_buf.p))) return rc;
            }
            HIPCHK(c, hipEventRecord(c->ev_rows[rb], c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_rows[rb], 0));
            HIPCHK(c, hipMemcpyAsync(static_cast<uint8_t *>(rows) + (size_t)done * rows_per_shuffle, row_buf.p,
                                     (size_t)n_sh * rows_per_shuffle, hipMemcpyDeviceToHost, c->copy_stream));
            HIPCHK(c, hipEventRecord(c->ev_copy[rb], c->copy_stream));
        }
    }
    if (rows && c->rows_async) { // the caller waits (fk_rows_wait): the next call's game kernel may run beside this call's last copy
        c->last_rows_event = (int32_t)(c->rows_calls % FK_ROWS_EVENTS);
        HIPCHK(c, hipEventRecord(c->ev_call_copy[c->last_rows_event], c->copy_stream));
        ++c->rows_calls;
    } else if (rows) {
        HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    }
    if (sq_n) {
        if ((rc = mirror_reduce(c, sq_n, (uint64_t)std::max<int64_t>(sq->pair_capacity, 0)))) return rc;
    }
    const uint32_t n_rows = (uint32_t)(n_batches * (uint64_t)S);
    hipLaunchKernelGGL(fk_finalize_tally, dim3((n_rows + 255u) / 256u), dim3(256), 0, c->stream, c->tally.p, n_rows, (uint32_t)S, shuffles_per_batch,
                       n_sh_total, 1u);
    HIPCHK(c, hipGetLastError());
    c->last_tally_bytes = tally_bytes; // (fk_tournament_run_stats adds it to the resident accumulator once the call has succeeded)
    HIPCHK(c, hipEventRecord(t1, c->stream));
    const size_t game_seed_bytes = call.game_seeds ? (size_t)n_sh_total * gps * 4 : 0, shuffle_seed_bytes = call.shuffle_seeds ? (size_t)n_sh_total * 4 : 0;
    reserve_mail(c, tally_bytes + game_seed_bytes + shuffle_seed_bytes + 256);
    if ((rc = post_d2h(c, tally, c->tally.p, tally_bytes))) return rc;
    if (game_seed_bytes + shuffle_seed_bytes) {
        // the fingerprints the row shards carry (game_seed column: ns 102, run_tournament.py:340-350) and their manifest names
        // (shuffle_seed: ns 100 = the same coordinate with game_index 0): with the tally, one host round trip for the launch group
        const fkl::Fingerprints fp(game_seed_bytes, shuffle_seed_bytes);
        if ((rc = ensure(c, c->seeds, fp.bytes))) return rc;
        if (game_seed_bytes) {
            const size_t n = (size_t)n_sh_total * gps;
            hipLaunchKernelGGL(fk_game_seed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, seed_prefix(102u /* TOURNAMENT_GAME */, root_seed, (uint64_t)k),
                               shuffle_begin, (uint32_t)n_sh_total, gps, c->seeds.as<uint32_t>(fp.game_at));
            HIPCHK(c, hipGetLastError());
            if ((rc = post_d2h(c, call.game_seeds, c->seeds.p + fp.game_at, game_seed_bytes))) return rc;
        }
        if (shuffle_seed_bytes) {
            hipLaunchKernelGGL(fk_game_seed_kernel, dim3((unsigned)((n_sh_total + 255) / 256)), dim3(256), 0, c->stream, seed_prefix(100u /* TOURNAMENT_SHUFFLE */, root_seed, (uint64_t)k),
                               shuffle_begin, (uint32_t)n_sh_total, 1u, c->seeds.as<uint32_t>(fp.shuffle_at));
            HIPCHK(c, hipGetLastError());
            if ((rc = post_d2h(c, call.shuffle_seeds, c->seeds.p + fp.shuffle_at, shuffle_seed_bytes))) return rc;
        }
    }
    if (seat_stats) HIPCHK(c, hipMemcpyAsync(seat_stats, c->stats.p, stats_bytes, hipMemcpyDeviceToHost, c->stream));
    if (seat_ratios) HIPCHK(c, hipMemcpyAsync(seat_ratios, c->ratios.p, ratio_bytes, hipMemcpyDeviceToHost, c->stream));
    int64_t sq_pairs = 0;
    if (sq) HIPCHK(c, hipMemcpyAsync(sq->counts, c->sa.counts.p, sq_bytes, hipMemcpyDeviceToHost, c->stream));
    if (sq_n) HIPCHK(c, hipMemcpyAsync(&sq_pairs, c->sa.pair_count.p, 8, hipMemcpyDeviceToHost, c->stream));
    int64_t g_spilled = 0;
    if (gst) {
        const ull *o = c->g_out.as<ull>();
        const std::pair<int64_t *, std::pair<size_t, size_t>> parts[] = { // every part ends where the next begins
            {gst->s_counts, {go.s_counts, go.s_rounds}}, {gst->s_rounds, {go.s_rounds, go.s_runner}}, {gst->s_runner, {go.s_runner, go.s_spread}},
            {gst->s_spread, {go.s_spread, go.g_counts}}, {gst->g_counts, {go.g_counts, go.g_rounds}}, {gst->g_rounds, {go.g_rounds, go.g_runner}},
            {gst->g_runner, {go.g_runner, go.spill_count}}, {&g_spilled, {go.spill_count, go.n_u64}}};
        for (const auto &pt : parts)
            HIPCHK(c, hipMemcpyAsync(pt.first, o + pt.second.first, (pt.second.second - pt.second.first) * 8, hipMemcpyDeviceToHost, c->stream));
    }
    int64_t r_events = 0;
    if (rare) {
        const ull *o = c->r_out.p;
        HIPCHK(c, hipMemcpyAsync(rare->s_second, o + ro.s_second, ro.g_second * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(rare->g_second, o + ro.g_second, (size_t)r_sb * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&r_events, o + ro.total, 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (lag) {
        const size_t edge_cells = (size_t)edge_rows * (size_t)S, edge_bytes = edge_cells * 2;
        HIPCHK(c, hipMemcpyAsync(lag->sums, c->lag_out.p, lag_sum_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(lag->head, c->lag_edge.p, edge_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(lag->tail, c->lag_edge.p + edge_cells, edge_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    deliver_mail(c);
    if (deferred) {
        rc = report_device_error(c, c->err_host, deferred_base, "tournament");
        const int rc_t = finish_timers(c);
        if (rc) return rc;
        if (rc_t) return rc_t;
    }
    if (rare) *rare->event_count = r_events; // (reported beside the spill count when both lists are too small)
    if (gst) { // the exact values outside the histogram windows
        *gst->spill_count = g_spilled;
        if (rare && r_events > rare->event_capacity && g_spilled > gst->spill_capacity)
            return fail(c, FK_ERR_ARG, "rare events: the event list needs %lld entries, event_capacity is %lld; the spill list needs %lld, spill_capacity is %lld",
                        (long long)r_events, (long long)rare->event_capacity, (long long)g_spilled, (long long)gst->spill_capacity);
        if (g_spilled > gst->spill_capacity)
            return fail(c, FK_ERR_ARG, "game statistics: the spill list needs %lld entries, spill_capacity is %lld", (long long)g_spilled,
                        (long long)gst->spill_capacity);
        if (g_spilled)
            HIPCHK(c, hipMemcpy(gst->spill, c->g_out.p + go.spill_at(), (size_t)g_spilled * 12, hipMemcpyDeviceToHost));
    }
    if (rare) { // the flagged games, in (shuffle, game) order
        if (r_events > rare->event_capacity)
            return fail(c, FK_ERR_ARG, "rare events: the event list needs %lld entries, event_capacity is %lld", (long long)r_events,
                        (long long)rare->event_capacity);
        if (r_events) {
            HIPCHK(c, hipMemcpy(rare->event_head, c->r_head.p, (size_t)r_events * 16, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(rare->event_seats, c->r_seats.p, (size_t)r_events * (size_t)k * 2, hipMemcpyDeviceToHost));
        }
    }
    if (sq_n) { // the pair rows, in ascending (rank a, rank b); ranks -> table indices
        *sq->pair_count = sq_pairs;
        if (sq_pairs > sq->pair_capacity)
            return fail(c, FK_ERR_ARG, "mirrored pairs: the pair list needs %lld rows, pair_capacity is %lld", (long long)sq_pairs,
                        (long long)sq->pair_capacity);
        if (sq_pairs) {
            HIPCHK(c, hipMemcpy(sq->pair_index, c->sa.pair_rank.p, (size_t)sq_pairs * 4, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(sq->pair_sums, c->sa.pair_sums.p, (size_t)sq_pairs * fksa::PAIR_COLS * 8, hipMemcpyDeviceToHost));
            std::vector<uint16_t> index_of((size_t)S);
            for (int32_t i = 0; i < S; ++i) index_of[sq->id_rank[i]] = (uint16_t)i;
            for (int64_t i = 0; i < 2 * sq_pairs; ++i) sq->pair_index[i] = index_of[sq->pair_index[i]];
        }
    }
    HIPCHK(c, hipEventElapsedTime(&c->timing.total_ms, t0, t1));
    return FK_OK;
}

static int tournament_call(fk_ctx *c, const TournamentCall &call) {
    if (!c) return FK_ERR_ARG;
    c->ran_hc = false;
    c->last_tally_bytes = 0;
    int rc = replay_on_oom(c, [&] { return tournament_run_impl(c, call); }); // from its first shuffle: every output is overwritten
    if (rc == FK_ERR_COUNTER_OVERFLOW && c->ran_hc) {
        // the hot / cold kernel's narrower counter fields (fk_play_hc.h) left their guard bands: the call is replayed on
        // fk_play_kernel, whose 16-bit fields are the ABI's stated limits
        if (getenv("FK_DEBUG_REPLAY")) fprintf(stderr, "hot / cold kernel replayed: %s\n", c->err.c_str());
        const int32_t saved = c->hc;
        c->hc = 0;
        for (auto &cs : c->sets) cs.prepared = false;
        rc = tournament_run_impl(c, call);
        c->hc = saved;
    }
    if (rc == 0 && c->resident && c->last_tally_bytes) {
        // the call's tally (still in c->tally) joins the resident accumulator — only now: a call that raised a device error,
        // the overflow that is replayed above included, must not have added anything (shape changes start a new accumulator)
        const size_t tally_bytes = c->last_tally_bytes, n_el = tally_bytes / sizeof(int64_t);
        if (c->acc_n != n_el) {
            rc = ensure(c, c->acc, n_el);
            if (rc) return rc;
            HIPCHK(c, hipMemsetAsync(c->acc.p, 0, tally_bytes, c->stream));
            c->acc_n = n_el;
        }
        hipLaunchKernelGGL(fk_add_i64_kernel, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, c->stream, c->acc.p, c->tally.p, n_el);
        HIPCHK(c, hipGetLastError());
    }
    return rc;
}

// ---- the entry points: each checks its own arguments and fills the request
int fk_tournament_run(fk_ctx *c, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                      uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score,
                      int32_t max_rounds, const fk_override *ov, int32_t n_ov, int64_t *tally, void *rows, int32_t *perms) {
    TournamentCall call{strategies, S, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch, target_score, max_rounds, ov, n_ov, tally, rows, perms};
    return tournament_call(c, call);
}

int fk_tournament_run_columns(fk_ctx *c, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed, uint64_t shuffle_begin,
                              uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score, int32_t max_rounds,
                              const fk_override *ov, int32_t n_ov, int64_t *tally, const int32_t *strategy_ids, void *columns) {
    if (!c) return FK_ERR_ARG;
    if (!strategy_ids || !columns) return fail(c, FK_ERR_ARG, "strategy_ids and columns are required");
    TournamentCall call{strategies, S, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch, target_score, max_rounds, ov, n_ov, tally, columns};
    call.columns_ids = strategy_ids;
    return tournament_call(c, call);
}

int fk_tournament_run_columns_seeds(fk_ctx *c, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed, uint64_t shuffle_begin,
                                    uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score, int32_t max_rounds,
                                    const fk_override *ov, int32_t n_ov, int64_t *tally, const int32_t *strategy_ids, void *columns,
                                    uint32_t *shuffle_seeds, uint32_t *game_seeds) {
    if (!c) return FK_ERR_ARG;
    if (!strategy_ids || !columns) return fail(c, FK_ERR_ARG, "strategy_ids and columns are required");
    TournamentCall call{strategies, S, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch, target_score, max_rounds, ov, n_ov, tally, columns};
    call.columns_ids = strategy_ids;
    call.shuffle_seeds = shuffle_seeds;
    call.game_seeds = game_seeds;
    return tournament_call(c, call);
}

int fk_tournament_run_stats(fk_ctx *c, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                            uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score,
                            int32_t max_rounds, const fk_override *ov, int32_t n_ov, int64_t *tally, void *rows, int32_t *perms,
                            int64_t *seat_stats) {
    TournamentCall call{strategies, S, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch, target_score, max_rounds, ov, n_ov, tally, rows, perms, seat_stats};
    return tournament_call(c, call);
}

int fk_tournament_run_all_player(fk_ctx *c, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                                 uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score,
                                 int32_t max_rounds, const fk_override *ov, int32_t n_ov, int64_t *tally, void *rows, int32_t *perms,
                                 int64_t *seat_stats, double *seat_ratio_sums) {
    if (!c) return FK_ERR_ARG;
    if (!seat_stats || !seat_ratio_sums) return fail(c, FK_ERR_ARG, "seat_stats and seat_ratio_sums are required");
    TournamentCall call{strategies, S, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch, target_score, max_rounds, ov, n_ov, tally, rows, perms, seat_stats, seat_ratio_sums};
    return tournament_call(c, call);
}

// the game-stat part of a request (fk_tournament_run_game_stats, fk_tournament_run_rare_events): checked, its count cleared
static int check_game_stats(fk_ctx *c, const TournamentCall &call) {
    const GameStatsReq &r = *call.gstats;
    if (!r.s_counts || !r.s_rounds || !r.s_runner || !r.s_spread || !r.g_counts || !r.g_rounds || !r.g_runner || !r.spill_count)
        return fail(c, FK_ERR_ARG, "the game-stat outputs and spill_count are required");
    if (call.seat_ratios && !call.seat_stats) return fail(c, FK_ERR_ARG, "seat_ratio_sums needs seat_stats");
    if (r.rounds_bins < 1 || r.rounds_bins > fkg::MAX_ROUNDS_BINS || r.margin_bins < 1 || r.margin_bins > fkg::MAX_MARGIN_BINS) // (negative: far above)
        return fail(c, FK_ERR_ARG, "rounds_bins must be in [1, %u] and margin_bins in [1, %u]", fkg::MAX_ROUNDS_BINS, fkg::MAX_MARGIN_BINS);
    if (r.spill_capacity < 0 || (r.spill_capacity > 0 && !r.spill)) return fail(c, FK_ERR_ARG, "spill_capacity must be >= 0, with a spill buffer when > 0");
    *r.spill_count = 0;
    return FK_OK;
}

int fk_tournament_run_game_stats(fk_ctx *c, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                                 uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score,
                                 int32_t max_rounds, const fk_override *ov, int32_t n_ov, int64_t *tally, void *rows, int32_t *perms,
                                 int64_t *seat_stats, double *seat_ratio_sums, int32_t rare_target_score, int32_t rounds_bins,
                                 int32_t margin_bins, int64_t *strategy_counts, int64_t *strategy_rounds, int64_t *strategy_runner,
                                 int64_t *strategy_spread, int64_t *game_counts, int64_t *game_rounds, int64_t *game_runner,
                                 int64_t spill_capacity, int64_t *spill_count, int32_t *spill) {
    if (!c) return FK_ERR_ARG;
    const GameStatsReq req{rare_target_score, (uint32_t)rounds_bins, (uint32_t)margin_bins, strategy_counts, strategy_rounds, strategy_runner,
                           strategy_spread, game_counts, game_rounds, game_runner, spill_capacity, spill_count, spill};
    TournamentCall call{strategies, S, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch, target_score, max_rounds, ov, n_ov, tally, rows, perms, seat_stats, seat_ratio_sums};
    call.gstats = &req;
    const int rc = check_game_stats(c, call);
    return rc ? rc : tournament_call(c, call);
}

int fk_tournament_run_rare_events(fk_ctx *c, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                                  uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score,
                                  int32_t max_rounds, const fk_override *ov, int32_t n_ov, int64_t *tally, void *rows, int32_t *perms,
                                  int64_t *seat_stats, double *seat_ratio_sums, int32_t rare_target_score, int32_t rounds_bins,
                                  int32_t margin_bins, int64_t *strategy_counts, int64_t *strategy_rounds, int64_t *strategy_runner,
                                  int64_t *strategy_spread, int64_t *game_counts, int64_t *game_rounds, int64_t *game_runner,
                                  int64_t spill_capacity, int64_t *spill_count, int32_t *spill, int32_t second_bins,
                                  int64_t *strategy_second, int64_t *game_second, int32_t n_thresholds, const int32_t *margin_thresholds,
                                  int64_t event_capacity, int64_t *event_count, uint32_t *event_head, uint16_t *event_seats) {
    if (!c) return FK_ERR_ARG;
    if (!strategy_second || !game_second || !event_count) return fail(c, FK_ERR_ARG, "strategy_second, game_second and event_count are required");
    if (second_bins < 1 || second_bins > (int32_t)fkre::MAX_SECOND_BINS) return fail(c, FK_ERR_ARG, "second_bins must be in [1, %u]", fkre::MAX_SECOND_BINS);
    if (n_thresholds < 0 || n_thresholds > (int32_t)fkre::MAX_THRESHOLDS || (n_thresholds > 0 && !margin_thresholds))
        return fail(c, FK_ERR_ARG, "n_thresholds must be in [0, %u], with margin_thresholds when > 0", fkre::MAX_THRESHOLDS);
    if (event_capacity < 0 || (event_capacity > 0 && (!event_head || !event_seats)))
        return fail(c, FK_ERR_ARG, "event_capacity must be >= 0, with event_head and event_seats when > 0");
    if (shuffle_end > shuffle_begin && shuffle_end - shuffle_begin > 0xffffffffull)
        return fail(c, FK_ERR_ARG, "rare events: an event names its shuffle in 32 bits; split the range");
    if (k > 0 && S / k > 65536) return fail(c, FK_ERR_ARG, "rare events: an event names its game in 16 bits (S / k <= 65536)");
    *event_count = 0;
    RareReq rr{};
    rr.second_bins = (uint32_t)second_bins;
    rr.s_second = strategy_second;
    rr.g_second = game_second;
    rr.thr.n = n_thresholds;
    for (int32_t i = 0; i < n_thresholds; ++i) rr.thr.v[i] = margin_thresholds[i];
    rr.events = !(event_capacity == 0 && n_thresholds == 0 && !event_head && !event_seats); // that form: the histograms only
    rr.event_capacity = event_capacity;
    rr.event_count = event_count;
    rr.event_head = event_head;
    rr.event_seats = event_seats;
    const GameStatsReq req{rare_target_score, (uint32_t)rounds_bins, (uint32_t)margin_bins, strategy_counts, strategy_rounds, strategy_runner,
                           strategy_spread, game_counts, game_rounds, game_runner, spill_capacity, spill_count, spill};
    TournamentCall call{strategies, S, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch, target_score, max_rounds, ov, n_ov, tally, rows, perms, seat_stats, seat_ratio_sums};
    call.gstats = &req;
    call.rare = &rr;
    const int rc = check_game_stats(c, call);
    return rc ? rc : tournament_call(c, call);
}

int fk_tournament_run_seat_counts(fk_ctx *c, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed,
                                  uint64_t shuffle_begin, uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score,
                                  int32_t max_rounds, const fk_override *ov, int32_t n_ov, int64_t *tally, int64_t *seat_counts,
                                  const uint16_t *id_rank, int64_t pair_capacity, int64_t *pair_count, uint16_t *pair_index,
                                  int64_t *pair_sums) {
    if (!c) return FK_ERR_ARG;
    if (!seat_counts) return fail(c, FK_ERR_ARG, "seat_counts is required");
    if (k < 1 || k > (int32_t)fksa::MAX_K) return fail(c, FK_ERR_ARG, "seat counts are made for 1 .. %u seats, got %d", fksa::MAX_K, (int)k);
    const bool mirrored = id_rank || pair_count || pair_index || pair_sums || pair_capacity != 0;
    if (mirrored) {
        if (k != 2) return fail(c, FK_ERR_ARG, "mirrored pairs exist at k = 2 only: the pair arguments must be null / 0 at k = %d", (int)k);
        if (!id_rank || !pair_count) return fail(c, FK_ERR_ARG, "mirrored pairs need id_rank and pair_count");
        if (pair_capacity < 0 || (pair_capacity > 0 && (!pair_index || !pair_sums)))
            return fail(c, FK_ERR_ARG, "pair_capacity must be >= 0, with pair_index and pair_sums when > 0");
        if (shuffles_per_batch == 0 || shuffle_begin % shuffles_per_batch != 0)
            return fail(c, FK_ERR_ARG, "mirrored pairs: shuffle_begin must be a multiple of shuffles_per_batch (a call never starts inside a batch)");
        if (S >= 2 && shuffle_end > shuffle_begin && (shuffle_end - shuffle_begin) > (uint64_t)0x7ffffffe / (uint64_t)(S / 2))
            return fail(c, FK_ERR_ARG, "mirrored pairs: the range may hold at most 2^31 - 2 games (one sort, 32-bit positions, one end entry); split it at a batch boundary");
        std::vector<uint8_t> seen((size_t)std::max(S, 0), 0);
        for (int32_t i = 0; i < S; ++i) {
            if (id_rank[i] >= (uint32_t)S || seen[id_rank[i]]) return fail(c, FK_ERR_ARG, "id_rank must be a permutation of 0 .. S - 1 (strategy IDs are unique)");
            seen[id_rank[i]] = 1;
        }
        *pair_count = 0;
    }
    const SeatReq req{seat_counts, mirrored ? id_rank : nullptr, pair_capacity, pair_count, pair_index, pair_sums};
    TournamentCall call{strategies, S, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch, target_score, max_rounds, ov, n_ov, tally};
    call.seats = &req;
    return tournament_call(c, call);
}

// the lag part of a request (fk_tournament_run_lags, fk_tournament_run_matchups): checked, then gathered
static int lag_request(fk_ctx *c, const TournamentCall &call, const int32_t *lags, int32_t n_lags, int64_t *lag_sums, uint16_t *edge_head,
                       uint16_t *edge_tail, LagReq &req) {
    if (!lags || !lag_sums || !edge_head || !edge_tail || n_lags < 1 || n_lags > FK_MAX_LAGS)
        return fail(c, FK_ERR_ARG, "lags, lag_sums, edge_head, edge_tail are required; 1 <= n_lags <= %d", FK_MAX_LAGS);
    const int rc = check_lags(c, lags, n_lags, " (rng_diagnostic_lags, config.py:1933-1939)");
    if (rc) return rc;
    if (call.max_rounds > 32767) return fail(c, FK_ERR_ARG, "lag statistics carry n_rounds in 15 bits: max_rounds must be <= 32767");
    for (int32_t i = 0; i < call.n_ov; ++i)
        if (call.ov && call.ov[i].max_rounds > 32767u) return fail(c, FK_ERR_ARG, "lag statistics carry n_rounds in 15 bits: override max_rounds must be <= 32767");
    req = LagReq{lags, n_lags, lags[n_lags - 1], lag_sums, edge_head, edge_tail};
    return FK_OK;
}

int fk_tournament_run_lags(fk_ctx *c, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed, uint64_t shuffle_begin,
                           uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score, int32_t max_rounds,
                           const fk_override *ov, int32_t n_ov, int64_t *tally, const int32_t *lags, int32_t n_lags, int64_t *lag_sums,
                           uint16_t *edge_head, uint16_t *edge_tail) {
    if (!c) return FK_ERR_ARG;
    TournamentCall call{strategies, S, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch, target_score, max_rounds, ov, n_ov, tally};
    LagReq req{};
    const int rc = lag_request(c, call, lags, n_lags, lag_sums, edge_head, edge_tail, req);
    if (rc) return rc;
    call.lag = &req;
    return tournament_call(c, call);
}

int fk_tournament_run_matchups(fk_ctx *c, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed, uint64_t shuffle_begin,
                               uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score, int32_t max_rounds,
                               const fk_override *ov, int32_t n_ov, int64_t *tally, const int32_t *lags, int32_t n_lags, int64_t *lag_sums,
                               uint16_t *edge_head, uint16_t *edge_tail, const int32_t *strategy_ids, int32_t max_players,
                               uint64_t *m_digest, uint16_t *m_seats, uint16_t *m_rounds) {
    if (!c) return FK_ERR_ARG;
    if (!strategy_ids || !m_digest || !m_seats || !m_rounds) return fail(c, FK_ERR_ARG, "strategy_ids, m_digest, m_seats, m_rounds are required");
    if (k < 1 || k > (int32_t)fkm::MAX_K) return fail(c, FK_ERR_ARG, "matchup records are made for 1 .. %u seats, got %d", fkm::MAX_K, (int)k);
    if (max_players < k || max_players > (int32_t)fkm::MAX_PLAYERS)
        return fail(c, FK_ERR_ARG, "max_players must be in [k, %u] (one BLAKE2b block), got %d", fkm::MAX_PLAYERS, (int)max_players);
    TournamentCall call{strategies, S, k, root_seed, shuffle_begin, shuffle_end, shuffles_per_batch, target_score, max_rounds, ov, n_ov, tally};
    LagReq req{};
    const int rc = lag_request(c, call, lags, n_lags, lag_sums, edge_head, edge_tail, req);
    if (rc) return rc;
    req.ids = strategy_ids;
    req.max_players = max_players;
    req.m_digest = m_digest;
    req.m_seats = m_seats;
    req.m_rounds = m_rounds;
    call.lag = &req;
    return tournament_call(c, call);
}

int fk_play_games(fk_ctx *c, const fk_coord *coords, int64_t n_games, const fk_strategy *table, int32_t S,
                  const int32_t *seat_strategy, int32_t k, int32_t target_score, int32_t max_rounds, void *rows) {
    if (!c) return FK_ERR_ARG;
    if (!coords || !table || !seat_strategy || !rows) return fail(c, FK_ERR_ARG, "coords, table, seat_strategy, rows are required");
    int rc = check_list_shape(c, n_games, S, k, max_rounds, 0x7fffffff);
    if (!rc) rc = check_list_games(c, coords, n_games, seat_strategy, S, k);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);
    if (n_games == 0) return FK_OK;
    if ((rc = upload_strategies(c, table, S))) return rc;
    const size_t row_bytes = sizeof(fk_row_hdr) + sizeof(fk_seat) * (size_t)k;
    if ((rc = ensure_all(c, c->coords, (size_t)n_games, c->seatlist, (size_t)n_games * k, c->rows, (size_t)n_games * row_bytes))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->coords.p, coords, sizeof(fk_coord) * (size_t)n_games, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->seatlist.p, seat_strategy, sizeof(int32_t) * (size_t)n_games * k, hipMemcpyHostToDevice, c->stream));

    LaunchPlan plan = plan_play(plan_knobs(c), PLAN_LIST, k, S, false, target_score);
    if (plan.block == 0)
        return fail(c, FK_ERR_ARG, "target_score %d: no kernel instance (lean records hold totals up to %d points; %d full records do not fit LDS)",
                    target_score, 50 * LEAN_MAX_TARGET50, (int)k);

    SeedArgs sa{};
    sa.coords = c->coords.p;
    sa.seat_strategy = c->seatlist.p;
    sa.k = (uint32_t)k;
    sa.n_games = (uint32_t)n_games;

    PlayArgs pa = table_args(c, target_score, max_rounds);
    pa.seat_strategy = c->seatlist.p;
    pa.mode = MODE_LIST;
    pa.n_games = (uint32_t)n_games;
    pa.gps = 1;
    pa.n_sh = 1;
    pa.k = (uint32_t)k;
    pa.S = (uint32_t)S;
    rc = run_chunk(c, sa, pa, plan, true, true, true, 0, "list");
    if (rc) return rc;
    rc = rows_pass(c, sa, false, (uint32_t)n_games, 1, 1, false, c->rows.p);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(rows, c->rows.p, (size_t)n_games * row_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->timing.total_ms = c->timing.seed_ms + c->timing.play_ms;
    return FK_OK;
}

// Roll-level trace of an explicit game list (fk_trace.h).  Counting pass (events per game + rows) -> exclusive scan -> the host
// reads the total and checks the capacity -> writing pass.  Nothing of the call stays in the context but device buffers.
int fk_trace_games(fk_ctx *c, const fk_coord *coords, int64_t n_games, const fk_strategy *table, int32_t S, const int32_t *seat_strategy,
                   int32_t k, int32_t target_score, int32_t max_rounds, void *rows, int64_t *event_begin, fk_roll_event *events,
                   int64_t event_capacity) {
    if (!c) return FK_ERR_ARG;
    if (!coords || !table || !seat_strategy || !rows || !event_begin)
        return fail(c, FK_ERR_ARG, "coords, table, seat_strategy, rows, event_begin are required");
    int rc = check_list_shape(c, n_games, S, k, max_rounds, 0x7ffffffe);
    if (rc) return rc;
    if (events && event_capacity < 0) return fail(c, FK_ERR_ARG, "event_capacity must not be negative");
    if ((rc = check_list_games(c, coords, n_games, seat_strategy, S, k))) return rc;
    if ((rc = validate_strategies(c, table, S))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);
    event_begin[0] = 0;
    if (n_games == 0) return FK_OK;
    const std::vector<int2> packed = strategies_in_points(table, S);
    const uint32_t n = (uint32_t)n_games, n_pad = (n + fktr::TR_BLOCK - 1u) / fktr::TR_BLOCK * fktr::TR_BLOCK;
    const size_t row_bytes = sizeof(fk_row_hdr) + sizeof(fk_seat) * (size_t)k;
    TraceBufs &t = c->tr;
    const size_t n1 = (size_t)n + 1;
    if ((rc = ensure_all(c, t.strat, (size_t)S, t.ws, (size_t)k * fktr::TR_FIELDS * n_pad, t.counts, n1, t.begin, n1, t.rows, (size_t)n * row_bytes, t.err, 1,
                         c->coords, (size_t)n, c->seatlist, (size_t)n * k)))
        return rc;
    const hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->coords.p, coords, sizeof(fk_coord) * (size_t)n, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->seatlist.p, seat_strategy, sizeof(int32_t) * (size_t)n * k, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(t.strat.p, packed.data(), sizeof(int2) * (size_t)S, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(t.counts.p, 0, 8 * n1, st)); // (the scan's last input, behind the games' counts)
    HIPCHK(c, hipMemsetAsync(t.err.p, 0xff, 8, st));      // TR_NO_ERROR
    fktr::TraceArgs a{};
    a.coords = c->coords.p;
    a.strat = t.strat.p;
    a.seat_strategy = c->seatlist.p;
    a.n_games = n;
    a.n_pad = n_pad;
    a.k = (uint32_t)k;
    a.target_score = target_score;
    a.max_rounds = (uint32_t)max_rounds;
    a.ws = t.ws.p;
    a.rows = t.rows.p;
    a.counts = t.counts.p;
    a.begin = t.begin.p;
    a.err = t.err.p;
    const dim3 grid(n_pad / fktr::TR_BLOCK), block(fktr::TR_BLOCK);
    {
        Timer tm(c, &c->timing.play_ms, SLOT_PLAY);
        hipLaunchKernelGGL(fktr::fk_trace_kernel<false>, grid, block, 0, st, a);
        HIPCHK(c, hipGetLastError());
        tm.stop();
    }
    FK_CUB(hipcub::DeviceScan::ExclusiveSum, a.counts, t.begin.p, (int)(n + 1u), st);
    unsigned long long err = fktr::TR_NO_ERROR;
    HIPCHK(c, hipMemcpyAsync(&err, t.err.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(event_begin, t.begin.p, 8 * n1, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(rows, t.rows.p, (size_t)n * row_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, collect_timers(c));
    c->timing.play_launches = 1;
    c->timing.play_block = (int32_t)fktr::TR_BLOCK;
    c->timing.play_grid = (int32_t)grid.x;
    c->timing.games = n_games;
    c->timing.total_ms = c->timing.play_ms;
    if ((rc = report_plain_error(c, err, "trace"))) return rc;
    const int64_t total = event_begin[n];
    if (!events) return FK_OK;
    if (event_capacity < total)
        return fail(c, FK_ERR_ARG, "event_capacity %lld is too small: the games roll %lld times (call again with that capacity)",
                    (long long)event_capacity, (long long)total);
    if (total == 0) return FK_OK;
    static_assert(sizeof(fk_roll_event) == sizeof(uint4), "the trace kernel stores an event as one uint4");
    if ((rc = ensure(c, t.events, (size_t)total))) return rc;
    a.events = t.events.p;
    {
        Timer tm(c, &c->timing.play_ms, SLOT_PLAY);
        hipLaunchKernelGGL(fktr::fk_trace_kernel<true>, grid, block, 0, st, a);
        HIPCHK(c, hipGetLastError());
        tm.stop();
    }
    HIPCHK(c, hipMemcpyAsync(events, t.events.p, sizeof(fk_roll_event) * (size_t)total, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, collect_timers(c));
    c->timing.play_launches = 2;
    c->timing.total_ms = c->timing.play_ms;
    return FK_OK;
}

// ---- roll census (fk_census.h).  One call = the tables zeroed on the device, the games played in chunks that fit the workspace
// budget (the per-seat workspace is [k][CN_FIELDS][chunk games]), one error word for the whole call, the tables copied out after the
// last chunk.  Nothing of the call stays in the context but device buffers; a failed call stores nothing in the caller's tables.
struct CensusCall {
    size_t n_u64[4]; // elements of roll_cells, strategy_dice, strategy_turns, turn_hist
    size_t off[5];   // their offsets in cn.tables (u64 units, the layout of fkcn::CensusArgs::tables); [4] = the error word
};

static int census_check_out(fk_ctx *c, const fk_census *out) {
    if (!out || !out->roll_cells || !out->strategy_dice || !out->strategy_turns || !out->turn_hist)
        return fail(c, FK_ERR_ARG, "the census and its four tables are required");
    if (out->turn_bins < 2 || out->turn_bins > 4096) return fail(c, FK_ERR_ARG, "turn_bins must be in [2, 4096], got %d", (int)out->turn_bins);
    return FK_OK;
}

// strategies in points, zeroed tables, error word; fills the table pointers of `a`
static int census_begin(fk_ctx *c, const fk_strategy *table, int32_t S, int32_t k, int32_t target_score, int32_t max_rounds, const fk_census *out,
                        CensusCall &cc, fkcn::CensusArgs &a) {
    int rc;
    begin_call(c);
    const std::vector<int2> packed = strategies_in_points(table, S);
    cc.n_u64[0] = fkcn::CN_CELLS;
    cc.n_u64[1] = (size_t)S * fkcn::CN_N * fkcn::CN_DICE_COLS;
    cc.n_u64[2] = (size_t)S * fkcn::CN_TURN_COLS;
    cc.n_u64[3] = (size_t)S * (size_t)out->turn_bins;
    cc.off[0] = 0;
    cc.off[1] = fkcn::dice_offset((uint32_t)S);
    cc.off[2] = fkcn::turns_offset((uint32_t)S);
    cc.off[3] = fkcn::hist_offset((uint32_t)S);
    cc.off[4] = fkcn::err_offset((uint32_t)S, (uint32_t)out->turn_bins);
    if ((rc = ensure_all(c, c->cn.strat, (size_t)S, c->cn.tables, cc.off[4] + 1))) return rc;
    const hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->cn.strat.p, packed.data(), sizeof(int2) * (size_t)S, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(c->cn.tables.p, 0, 8 * cc.off[4], st));
    HIPCHK(c, hipMemsetAsync(c->cn.tables.p + cc.off[4], 0xff, 8, st)); // TR_NO_ERROR
    HIPCHK(c, hipStreamSynchronize(st)); // `packed` goes out of scope
    a = fkcn::CensusArgs{};
    a.strat = c->cn.strat.p;
    a.k = (uint32_t)k;
    a.S = (uint32_t)S;
    a.target_score = target_score;
    a.max_rounds = (uint32_t)max_rounds;
    a.turn_bins = (uint32_t)out->turn_bins;
    a.tables = c->cn.tables.p;
    return FK_OK;
}

// games one chunk may hold: the workspace budget over the per-game seat workspace, whole workgroups; option "census_chunk_games" caps it
static uint64_t census_chunk_games(fk_ctx *c, int32_t k) {
    const uint64_t per_game = (uint64_t)k * fkcn::CN_FIELDS * 4;
    uint64_t n = (uint64_t)workspace_budget(c) / per_game / fkcn::CN_BLOCK * fkcn::CN_BLOCK;
    n = std::min<uint64_t>(std::max<uint64_t>(n, fkcn::CN_BLOCK), (uint64_t)1 << 30);
    if (c->census_chunk_games > 0) n = std::min<uint64_t>(n, (uint64_t)c->census_chunk_games);
    return n;
}

// one chunk: a.n_games games from a.game_base; waits for it and reads the error word
static int census_chunk(fk_ctx *c, fkcn::CensusArgs &a, bool list, const char *what) {
    int rc;
    a.n_pad = (a.n_games + fkcn::CN_BLOCK - 1u) / fkcn::CN_BLOCK * fkcn::CN_BLOCK;
    if ((rc = ensure(c, c->cn.ws, (size_t)a.k * fkcn::CN_FIELDS * a.n_pad))) return rc;
    a.ws = c->cn.ws.p;
    const dim3 grid(a.n_pad / fkcn::CN_BLOCK), block(fkcn::CN_BLOCK);
    {
        Timer t(c, &c->timing.play_ms, SLOT_PLAY);
        if (list) hipLaunchKernelGGL(fkcn::fk_census_kernel<true>, grid, block, 0, c->stream, a);
        else hipLaunchKernelGGL(fkcn::fk_census_kernel<false>, grid, block, 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        t.stop();
    }
    unsigned long long err = fktr::TR_NO_ERROR;
    HIPCHK(c, hipMemcpyAsync(&err, a.tables + fkcn::err_offset(a.S, a.turn_bins), 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, collect_timers(c));
    c->timing.play_launches += 1;
    c->timing.play_block = (int32_t)fkcn::CN_BLOCK;
    c->timing.play_grid = (int32_t)grid.x;
    c->timing.play_lds_bytes = (int32_t)(fkcn::CN_CELLS * 4);
    c->timing.games += a.n_games;
    c->timing.total_ms = c->timing.play_ms;
    return report_plain_error(c, err, what);
}

static int census_end(fk_ctx *c, const CensusCall &cc, const fk_census *out) {
    const ull *t = c->cn.tables.p;
    uint64_t *dst[4] = {out->roll_cells, out->strategy_dice, out->strategy_turns, out->turn_hist};
    for (int i = 0; i < 4; ++i) HIPCHK(c, hipMemcpyAsync(dst[i], t + cc.off[i], 8 * cc.n_u64[i], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FK_OK;
}

int fk_census_games(fk_ctx *c, const fk_coord *coords, int64_t n_games, const fk_strategy *table, int32_t S, const int32_t *seat_strategy,
                    int32_t k, int32_t target_score, int32_t max_rounds, fk_census *out) {
    if (!c) return FK_ERR_ARG;
    if (!coords || !table || !seat_strategy) return fail(c, FK_ERR_ARG, "coords, table, seat_strategy are required");
    int rc = check_list_shape(c, n_games, S, k, max_rounds, 0x7ffffffe);
    if (!rc) rc = census_check_out(c, out);
    if (!rc) rc = check_list_games(c, coords, n_games, seat_strategy, S, k);
    if (rc) return rc;
    if ((rc = validate_strategies(c, table, S))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    CensusCall cc{};
    fkcn::CensusArgs a{};
    if ((rc = census_begin(c, table, S, k, target_score, max_rounds, out, cc, a))) return rc;
    const uint64_t chunk = census_chunk_games(c, k);
    for (uint64_t done = 0; done < (uint64_t)n_games; done += chunk) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, (uint64_t)n_games - done);
        if ((rc = ensure_all(c, c->coords, (size_t)n, c->seatlist, (size_t)n * k))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->coords.p, coords + done, sizeof(fk_coord) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->seatlist.p, seat_strategy + done * (uint64_t)k, sizeof(int32_t) * (size_t)n * k, hipMemcpyHostToDevice, c->stream));
        a.coords = c->coords.p;
        a.seat_strategy = c->seatlist.p;
        a.n_games = n;
        a.game_base = done;
        if ((rc = census_chunk(c, a, true, "census"))) return rc;
    }
    return census_end(c, cc, out);
}

int fk_tournament_run_census(fk_ctx *c, const fk_strategy *strategies, int32_t S, int32_t k, uint64_t root_seed, uint64_t shuffle_begin,
                             uint64_t shuffle_end, uint32_t shuffles_per_batch, int32_t target_score, int32_t max_rounds, const fk_override *ov,
                             int32_t n_ov, fk_census *out) {
    if (!c) return FK_ERR_ARG;
    if (!strategies) return fail(c, FK_ERR_ARG, "strategies are required");
    int rc = check_seating(c, S, k);
    if (!rc) rc = check_range(c, S, max_rounds, shuffle_begin, shuffle_end, shuffles_per_batch, ov, n_ov);
    if (!rc) rc = census_check_out(c, out);
    if (rc) return rc;
    if ((rc = validate_strategies(c, strategies, S))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    CensusCall cc{};
    fkcn::CensusArgs a{};
    if ((rc = census_begin(c, strategies, S, k, target_score, max_rounds, out, cc, a))) return rc;
    const uint64_t n_sh_total = shuffle_end - shuffle_begin;
    const uint32_t gps = (uint32_t)(S / k);
    const uint32_t slots = perm_slots(S);
    uint64_t chunk_sh = std::max<uint64_t>(1, census_chunk_games(c, k) / gps);
    chunk_sh = std::min<uint64_t>(chunk_sh, (uint64_t)0x7fffffff / gps);
    // the chunk set no prepared (hinted) tournament chunk sits in; whatever it held is void afterwards
    const int si = c->sets[c->cur].prepared ? c->cur ^ 1 : c->cur;
    ChunkSet &cs = c->sets[si];
    for (uint64_t done = 0; done < n_sh_total; done += chunk_sh) {
        const uint32_t n_sh = (uint32_t)std::min<uint64_t>(chunk_sh, n_sh_total - done);
        const uint64_t sh0 = shuffle_begin + done;
        // overrides that fall into this chunk -> chunk-local game ids
        if ((rc = map_tournament_overrides(c, ov, n_ov, root_seed, k, sh0, n_sh, gps, a.n_ov))) return rc;
        cs.prepared = false;
        HIPCHK(c, hipStreamWaitEvent(c->stream, cs.ready, 0)); // an unused side-stream preparation may still own the set
        const ChunkDesc d{c->table_epoch, root_seed, sh0, n_sh, (uint32_t)S, (uint32_t)k, 0u, 0u, slots};
        const uint32_t perm_blocks = (n_sh + slots - 1u) / slots;
        if ((rc = ensure(c, cs.perm, (size_t)perm_blocks * S * slots))) return rc;
        if ((rc = launch_perm_kernels(c, cs, c->stream, d))) return rc;
        a.coords = nullptr;
        a.seat_strategy = nullptr;
        a.perm_T = cs.perm.p;
        a.perm_slots = slots;
        a.gps = gps;
        a.root_seed = root_seed;
        a.shuffle0 = sh0;
        a.ov = c->ov.p;
        a.n_games = n_sh * gps;
        a.game_base = done * gps;
        if ((rc = census_chunk(c, a, false, "census"))) return rc;
    }
    return census_end(c, cc, out);
}

// Many H2H blocks advanced together.  Each pass plays, for every block that still needs games, exactly
// min(target - completed, stop - attempted) attempts in attempt order: a pass can never overshoot the prefix rule (the
// first attempt index at which `target` games have completed, h2h_schedule.py:1165-1235), because it reaches the target
// only if every one of its attempts completes, i.e. at its last attempt.  Blocks with safety-limit games need further
// (geometrically smaller) passes; all blocks share each pass's launch.
static int h2h_run_blocks_impl(fk_ctx *c, fk_h2h_block *blocks, int64_t n_blocks, uint64_t root_seed, uint64_t chunk_games,
                               int32_t target_score, int32_t max_rounds, const fk_override *ov, int32_t n_ov);

int fk_h2h_run_blocks(fk_ctx *c, fk_h2h_block *blocks, int64_t n_blocks, uint64_t root_seed, uint64_t chunk_games,
                      int32_t target_score, int32_t max_rounds, const fk_override *ov, int32_t n_ov) {
    if (!c) return FK_ERR_ARG;
    // the blocks are advanced in place: a replay after an out-of-memory failure starts from the states the caller handed in
    std::vector<fk_h2h_block> saved;
    if (blocks && n_blocks > 0 && n_blocks <= (1 << 22)) saved.assign(blocks, blocks + n_blocks);
    return replay_on_oom(c, [&] {
        if (c->oom_replays) std::copy(saved.begin(), saved.end(), blocks);
        return h2h_run_blocks_impl(c, blocks, n_blocks, root_seed, chunk_games, target_score, max_rounds, ov, n_ov);
    });
}

static int h2h_run_blocks_impl(fk_ctx *c, fk_h2h_block *blocks, int64_t n_blocks, uint64_t root_seed, uint64_t chunk_games,
                               int32_t target_score, int32_t max_rounds, const fk_override *ov, int32_t n_ov) {
    if (!blocks || n_blocks < 0 || n_blocks > (1 << 22)) return fail(c, FK_ERR_ARG, "blocks are required (at most 2^22 per call)");
    int rc = check_max_rounds(c, max_rounds);
    if (!rc) rc = check_override_list(c, ov, n_ov);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);
    if (n_blocks == 0) return FK_OK;
    std::vector<fk_strategy> table((size_t)n_blocks * 2);
    std::vector<uint64_t> stop((size_t)n_blocks);
    for (int64_t b = 0; b < n_blocks; ++b) {
        const fk_h2h_block &blk = blocks[b];
        if (blk.order > 1u) return fail(c, FK_ERR_ARG, "block %lld: order must be 0 or 1", (long long)b);
        const uint64_t attempted = blk.state[0], completed = blk.state[1], safety = blk.state[2], w1 = blk.state[3], w2 = blk.state[4];
        if (!(completed <= blk.target) || !(attempted <= blk.max_attempts) || completed + safety != attempted || w1 + w2 != completed)
            return fail(c, FK_ERR_ARG, "block %lld: inconsistent block state", (long long)b); // h2h_schedule.py:1366, 1422-1468
        uint64_t st = attempted + chunk_games; // :1172
        if (st > blk.max_attempts || st < attempted) st = blk.max_attempts;
        stop[(size_t)b] = st;
        table[(size_t)b * 2] = blk.seats[0];
        table[(size_t)b * 2 + 1] = blk.seats[1];
    }
    if ((rc = upload_strategies(c, table.data(), n_blocks * 2))) return rc;
    const LaunchPlan plan = plan_play(plan_knobs(c), PLAN_H2H, 2, n_blocks * 2, false, target_score);
    if (plan.block == 0)
        return fail(c, FK_ERR_ARG, "target_score %d: batched head-to-head plays with lean records (totals up to %d points)", target_score,
                    50 * LEAN_MAX_TARGET50);
    const uint64_t max_launch = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)workspace_budget(c) / (game_workspace_bytes(2, plan.shape().gs, false, false) + 8), 1u << 30));
    rc = ensure(c, c->block_out, (size_t)n_blocks * 4);
    if (rc) return rc;

    // A GENERATION plays, for every block that still needs games, exactly min(stop - attempted, target - completed) attempts —
    // all of them planned up front from the blocks' current states and cut into passes (launches) of at most max_launch games,
    // which play_block_passes plays.  The strategy table (two rows per block of the CALL) and the per-block counts are per call.
    // Blocks with safety-limit games need further (geometrically smaller) generations.
    struct Pass {
        std::vector<DevBlock> blocks;
        uint32_t n_games = 0;
    };
    constexpr size_t MAX_PASS_BLOCKS = (size_t)1 << 22;
    std::vector<unsigned long long> out((size_t)n_blocks * 4);
    std::vector<uint64_t> planned((size_t)n_blocks);
    const bool pipelined = c->pipeline != 0 && n_ov == 0; // per-pass override lists live in one device buffer
    while (true) {
        std::vector<Pass> passes;
        std::fill(planned.begin(), planned.end(), 0);
        for (int64_t b = 0; b < n_blocks; ++b) {
            const fk_h2h_block &blk = blocks[b];
            if (blk.state[0] >= stop[(size_t)b] || blk.state[1] >= blk.target) continue;
            uint64_t n = std::min<uint64_t>(stop[(size_t)b] - blk.state[0], blk.target - blk.state[1]);
            planned[(size_t)b] = n;
            uint64_t attempt0 = blk.state[0];
            while (n) { // a block may straddle passes
                if (passes.empty() || passes.back().n_games >= max_launch || passes.back().blocks.size() >= MAX_PASS_BLOCKS) passes.emplace_back();
                Pass &p = passes.back();
                const uint64_t take = std::min<uint64_t>(n, max_launch - p.n_games);
                p.blocks.push_back(DevBlock{blk.pair_id, attempt0, blk.order, p.n_games, (uint32_t)b, 0u});
                p.n_games += (uint32_t)take;
                attempt0 += take;
                n -= take;
            }
        }
        if (passes.empty()) break;
        HIPCHK(c, hipMemsetAsync(c->block_out.p, 0, (size_t)n_blocks * 4 * 8, c->stream));

        const PassBlocks pass_blocks = [&](size_t i, DevBlock *dst, hipStream_t st, uint32_t &nb, uint32_t &games) -> int {
            const Pass &p = passes[i];
            nb = (uint32_t)p.blocks.size();
            games = p.n_games;
            if (dst) HIPCHK(c, hipMemcpyAsync(dst, p.blocks.data(), (size_t)nb * sizeof(DevBlock), hipMemcpyHostToDevice, st));
            return FK_OK;
        };
        // overrides -> pass-local game ids (not pipelined: one device list)
        const PassOverrides pass_overrides = [&](size_t i, uint32_t &n_dev) -> int {
            const Pass &p = passes[i];
            return map_overrides(c, ov, n_ov, n_dev, [&](const fk_override &o, std::vector<uint32_t> &games) {
                if (o.root_seed != root_seed) return false;
                for (size_t q = 0; q < p.blocks.size(); ++q) {
                    const DevBlock &db = p.blocks[q];
                    const uint32_t n_q = (q + 1 < p.blocks.size() ? p.blocks[q + 1].start : p.n_games) - db.start;
                    if (o.a != db.pair || o.k_or_order != db.order) continue;
                    if (o.b < db.attempt0 || o.b >= db.attempt0 + n_q) continue;
                    games.push_back(db.start + (uint32_t)(o.b - db.attempt0));
                }
                return true;
            });
        };
        rc = play_block_passes(c, passes.size(), plan, root_seed, (uint32_t)n_blocks * 2u, target_score, max_rounds, pipelined, pass_blocks, pass_overrides);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(out.data(), c->block_out.p, (size_t)n_blocks * 4 * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int64_t b = 0; b < n_blocks; ++b) {
            const uint64_t n_b = planned[(size_t)b];
            if (!n_b) continue;
            const uint64_t comp = out[(size_t)b * 4], saf = out[(size_t)b * 4 + 1], a1 = out[(size_t)b * 4 + 2], a2 = out[(size_t)b * 4 + 3];
            if (comp + saf != n_b || a1 + a2 != comp)
                return fail(c, FK_ERR_HIP, "h2h block conservation failed (block %lld: %llu + %llu != %llu)", (long long)b,
                            (unsigned long long)comp, (unsigned long long)saf, (unsigned long long)n_b);
            fk_h2h_block &blk = blocks[b];
            blk.state[0] += n_b;
            blk.state[1] += comp;
            blk.state[2] += saf;
            blk.state[3] += a1;
            blk.state[4] += a2;
        }
    }
    c->timing.total_ms = c->timing.seed_ms + c->timing.play_ms;
    return FK_OK;
}

int fk_h2h_run(fk_ctx *c, const fk_strategy seats[2], uint64_t root_seed, uint64_t pair_id, uint32_t order, uint64_t target,
               uint64_t max_attempts, uint64_t chunk_games, int32_t target_score, int32_t max_rounds, const fk_override *ov,
               int32_t n_ov, uint64_t state[5]) {
    if (!c) return FK_ERR_ARG;
    if (!seats || !state) return fail(c, FK_ERR_ARG, "seats and state are required");
    if (order > 1u) return fail(c, FK_ERR_ARG, "order must be 0 or 1");
    fk_h2h_block blk{};
    blk.seats[0] = seats[0];
    blk.seats[1] = seats[1];
    blk.pair_id = pair_id;
    blk.order = order;
    blk.target = target;
    blk.max_attempts = max_attempts;
    memcpy(blk.state, state, sizeof(blk.state));
    const int rc = fk_h2h_run_blocks(c, &blk, 1, root_seed, chunk_games, target_score, max_rounds, ov, n_ov);
    if (rc == FK_OK) memcpy(state, blk.state, sizeof(blk.state));
    return rc;
}

// ---- head-to-head round robin: every pair of a table in one call (device side: fk_round_robin.h) ----
// The window / generation structure is h2h_run_blocks_impl's with the host's per-block work moved to the device: the host reads the
// generation's total, the number of playing blocks and the call's error record, then two words per pass; play_block_passes plays them.
static int h2h_round_robin_impl(fk_ctx *c, const fk_strategy *table, int32_t n, uint64_t root_seed, uint64_t pair_begin, uint64_t pair_end,
                                uint64_t target, uint64_t max_attempts, int32_t target_score, int32_t max_rounds, const LaunchPlan &plan,
                                uint32_t *block_state, int64_t *summary, uint32_t *d_staged = nullptr, uint32_t *d_root_slot = nullptr) {
    using namespace fkrr; // d_staged: the call's states stay on the device, [pair_end - pair_begin][2][RR_STATE] (block_state is null then);
                          // d_root_slot, nullable: they are also kept there (option "rr_keep_roots")
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);
    // the n-row table, packed, and its patience classes: uploaded once per call
    std::vector<uint2> packed((size_t)n);
    std::vector<uint8_t> patience((size_t)n);
    uint32_t f_and = 0xff00u, f_or = 0u;
    for (int32_t i = 0; i < n; ++i) {
        packed[(size_t)i] = pack_strategy(table[i]);
        patience[(size_t)i] = patience_of(table[i]);
        f_and &= packed[(size_t)i].y;
        f_or |= packed[(size_t)i].y & 0xff00u;
    }
    // the resident table of the other entries is replaced by window rows: whatever was prepared for it is void
    c->strat_host.clear();
    c->table_epoch += 1;
    for (auto &cs : c->sets) cs.prepared = false;
    c->hint_valid = false;
    if (c->prep_stream) HIPCHK(c, hipStreamSynchronize(c->prep_stream));
    c->table_mixed_flags = f_or & ~f_and; // every window's rows are rows of this table
    c->table_flags = f_and;

    const uint64_t n_pairs_call = pair_end - pair_begin;
    const uint64_t window_pairs = std::min<uint64_t>((uint64_t)c->rr_window_blocks / 2u, n_pairs_call);
    const uint32_t max_rows = (uint32_t)(window_pairs * 2u);
    const uint64_t max_launch = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)workspace_budget(c) / (game_workspace_bytes(2, plan.shape().gs, false, false) + 8), 1u << 30));
    RoundRobinBufs &r = c->rr;
    const size_t rows1 = (size_t)max_rows + 1;
    int rc = FK_OK;
    if ((rc = ensure_all(c, r.table, (size_t)n, r.patience, (size_t)n, r.state, d_staged ? 0 : (size_t)max_rows * RR_STATE, r.need, rows1, r.off, rows1, r.flag, rows1,
                         r.aidx, rows1, r.act, (size_t)max_rows, r.err, 1)))
        return rc;
    if (summary && (rc = ensure(c, r.summary, (size_t)n * RR_COLS))) return rc;
    if ((rc = ensure_all(c, c->strat, 2 * (size_t)max_rows, c->slow, 2 * (size_t)max_rows, c->block_out, (size_t)max_rows * 4))) return rc;
    uint32_t *d_flag = r.flag.p, *d_aidx = r.aidx.p, *d_act = r.act.p;
    ull *d_need = r.need.p, *d_off = r.off.p;
    RrError *d_err = r.err.p;
    { // the scratch of both scans of a generation, sized once for the largest window: no size query inside the window loop
        size_t need = 1;
        FK_CUB_NEED(need, hipcub::DeviceScan::ExclusiveSum, d_need, d_off, (int)(max_rows + 1u), c->stream);
        FK_CUB_NEED(need, hipcub::DeviceScan::ExclusiveSum, d_flag, d_aidx, (int)(max_rows + 1u), c->stream);
        if ((rc = ensure(c, c->cub, need))) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(r.table.p, packed.data(), sizeof(uint2) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(r.patience.p, patience.data(), (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_err, 0, sizeof(RrError), c->stream));
    if (summary) HIPCHK(c, hipMemsetAsync(r.summary.p, 0, (size_t)n * RR_COLS * 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the host vectors are pageable)

    const bool pipelined = c->pipeline != 0;
    std::vector<uint32_t> bounds;
    for (uint64_t pair0 = pair_begin; pair0 < pair_end; pair0 += window_pairs) {
        const uint32_t n_pairs = (uint32_t)std::min<uint64_t>(window_pairs, pair_end - pair0), n_rows = 2u * n_pairs;
        const dim3 rows_grid((n_rows + 1u + 255u) / 256u), b256(256);
        uint32_t *d_state = d_staged ? d_staged + (size_t)(pair0 - pair_begin) * 2 * RR_STATE : r.state.p;
        hipLaunchKernelGGL(fk_rr_window_kernel, rows_grid, b256, 0, c->stream, r.table.p, r.patience.p, (uint32_t)n, pair0, n_rows, c->strat.p, c->slow.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemsetAsync(d_state, 0, (size_t)n_rows * RR_STATE * 4, c->stream)); // every block starts fresh
        while (true) { // generations
            hipLaunchKernelGGL(fk_rr_need_kernel, rows_grid, b256, 0, c->stream, d_state, n_rows, (uint32_t)target, (uint32_t)max_attempts, d_need, d_flag);
            HIPCHK(c, hipGetLastError());
            FK_CUB_SIZED(hipcub::DeviceScan::ExclusiveSum, d_need, d_off, (int)(n_rows + 1u), c->stream);
            FK_CUB_SIZED(hipcub::DeviceScan::ExclusiveSum, d_flag, d_aidx, (int)(n_rows + 1u), c->stream);
            hipLaunchKernelGGL(fk_rr_compact_kernel, rows_grid, b256, 0, c->stream, d_flag, d_aidx, n_rows, d_act);
            HIPCHK(c, hipGetLastError());
            unsigned long long total = 0;
            uint32_t n_act = 0;
            RrError err{0u, 0u};
            HIPCHK(c, hipMemcpyAsync(&total, d_off + n_rows, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&n_act, d_aidx + n_rows, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, c->stream)); // of the generation before
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (err.raised)
                return fail(c, FK_ERR_HIP, "h2h block conservation failed (pair %llu, order %u)", (unsigned long long)(pair0 + (err.row >> 1)), err.row & 1u);
            if (total == 0) break;
            const uint64_t n_passes64 = (total + max_launch - 1) / max_launch;
            if (n_passes64 > ((uint64_t)1 << 20))
                return fail(c, FK_ERR_ARG, "a generation of %llu games needs more than 2^20 launches of %llu games: raise chunk_bytes or lower rr_window_blocks",
                            total, (unsigned long long)max_launch);
            const uint32_t n_passes = (uint32_t)n_passes64;
            if ((rc = ensure(c, r.bounds, (size_t)n_passes * 2))) return rc;
            hipLaunchKernelGGL(fk_rr_pass_bounds_kernel, dim3((n_passes + 255u) / 256u), b256, 0, c->stream, d_off, d_need, d_act, n_act, total,
                               (unsigned long long)max_launch, n_passes, r.bounds.p);
            HIPCHK(c, hipGetLastError());
            bounds.resize((size_t)n_passes * 2);
            HIPCHK(c, hipMemcpyAsync(bounds.data(), r.bounds.p, (size_t)n_passes * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemsetAsync(c->block_out.p, 0, (size_t)n_rows * 4 * 8, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            auto pass_games = [&](size_t i) { return (uint32_t)(std::min<uint64_t>(total, (uint64_t)(i + 1) * max_launch) - (uint64_t)i * max_launch); };

            // a pass's DevBlocks are written on the device
            const PassBlocks pass_blocks = [&](size_t i, DevBlock *dst, hipStream_t st, uint32_t &nb, uint32_t &games) -> int {
                const uint32_t first = bounds[2 * i];
                if (bounds[2 * i + 1] <= first || bounds[2 * i + 1] > n_act) return fail(c, FK_ERR_HIP, "round-robin pass %zu has no blocks", i);
                nb = bounds[2 * i + 1] - first;
                games = pass_games(i);
                if (!dst) return FK_OK;
                hipLaunchKernelGGL(fk_rr_pass_blocks_kernel, dim3((nb + 255u) / 256u), dim3(256), 0, st, d_off, d_act, d_state, first, nb,
                                   (unsigned long long)((uint64_t)i * max_launch), pair0, dst);
                HIPCHK(c, hipGetLastError());
                return FK_OK;
            };
            if ((rc = play_block_passes(c, n_passes, plan, root_seed, n_rows * 2u, target_score, max_rounds, pipelined, pass_blocks, nullptr))) return rc;
            hipLaunchKernelGGL(fk_rr_apply_kernel, rows_grid, b256, 0, c->stream, d_state, d_need, c->block_out.p, n_rows, d_err);
            HIPCHK(c, hipGetLastError());
        }
        if (summary) {
            hipLaunchKernelGGL(fk_rr_summary_kernel, dim3((n_pairs + 255u) / 256u), b256, 0, c->stream, d_state, (uint32_t)n, pair0, n_pairs,
                               (uint32_t)target, r.summary.p);
            HIPCHK(c, hipGetLastError());
        }
        if (!d_staged)
            HIPCHK(c, hipMemcpyAsync(block_state + (size_t)(pair0 - pair_begin) * 2 * RR_STATE, d_state, (size_t)n_rows * RR_STATE * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); // the next window reuses the device buffers
    }
    if (d_staged) { // the whole call has succeeded: its states join the resident accumulator (a failed or replayed call has added nothing)
        const uint64_t n_rows_call = 2u * n_pairs_call;
        hipLaunchKernelGGL(fkri::fk_ri_add_kernel, dim3((uint32_t)((n_rows_call + 255u) / 256u)), dim3(256), 0, c->stream, d_staged, n_rows_call,
                           (uint32_t)target, (uint32_t)max_attempts, c->ri.counts.p);
        HIPCHK(c, hipGetLastError());
        if (d_root_slot) HIPCHK(c, hipMemcpyAsync(d_root_slot, d_staged, (size_t)n_rows_call * RR_STATE * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (summary) { // added to the caller's buffer only when the whole call has succeeded
        std::vector<int64_t> add((size_t)n * RR_COLS);
        HIPCHK(c, hipMemcpy(add.data(), r.summary.p, add.size() * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < add.size(); ++i) summary[i] += add[i];
    }
    c->timing.total_ms = c->timing.seed_ms + c->timing.play_ms;
    return FK_OK;
}

// what fk_h2h_round_robin and fk_h2h_round_robin_resident refuse alike, before any device work; `plan` is the call's launch plan
static int round_robin_check(fk_ctx *c, const fk_strategy *table, int32_t n, uint64_t pair_begin, uint64_t pair_end, uint64_t target,
                             uint64_t max_attempts, int32_t target_score, int32_t max_rounds, LaunchPlan &plan) {
    if (!table) return fail(c, FK_ERR_ARG, "the strategy table is required");
    if (n < 2) return fail(c, FK_ERR_ARG, "a round robin needs at least two strategies, got %d", (int)n);
    const uint64_t all_pairs = (uint64_t)n * (uint64_t)(n - 1) / 2u;
    if (pair_begin > pair_end || pair_end > all_pairs)
        return fail(c, FK_ERR_ARG, "pair range [%llu, %llu) is not inside the %llu pairs of %d strategies", (unsigned long long)pair_begin,
                    (unsigned long long)pair_end, (unsigned long long)all_pairs, (int)n);
    if (target == 0 || target > max_attempts || max_attempts > 0x7fffffffull)
        return fail(c, FK_ERR_ARG, "target must be in [1, max_attempts] and max_attempts at most 2^31 - 1");
    int rc = check_max_rounds(c, max_rounds);
    if (rc) return rc;
    plan = plan_play(plan_knobs(c), PLAN_H2H, 2, 4, false, target_score);
    if (plan.block == 0)
        return fail(c, FK_ERR_ARG, "target_score %d: batched head-to-head plays with lean records (totals up to %d points)", target_score,
                    50 * LEAN_MAX_TARGET50);
    return validate_strategies(c, table, n);
}

int fk_h2h_round_robin(fk_ctx *c, const fk_strategy *table, int32_t n, uint64_t root_seed, uint64_t pair_begin, uint64_t pair_end, uint64_t target,
                       uint64_t max_attempts, int32_t target_score, int32_t max_rounds, uint32_t *block_state, int64_t *summary) {
    if (!c) return FK_ERR_ARG;
    LaunchPlan plan{};
    if (const int rc = round_robin_check(c, table, n, pair_begin, pair_end, target, max_attempts, target_score, max_rounds, plan)) return rc;
    if (pair_begin == pair_end) return FK_OK; // an empty range touches nothing
    if (!block_state) return fail(c, FK_ERR_ARG, "block_state is required");
    // no in/out state: the replay after an out-of-memory failure is the call again with half the budget
    return replay_on_oom(c, [&] {
        return h2h_round_robin_impl(c, table, n, root_seed, pair_begin, pair_end, target, max_attempts, target_score, max_rounds, plan, block_state, summary);
    });
}

// ---- round-robin inference: resident pair counts and the inference over them (device side: fk_rr_inference.h) ----
static uint64_t rr_table_hash(const fk_strategy *table, int32_t n) { // FNV-1a over the table's bytes (fk_strategy has no padding)
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char *b = reinterpret_cast<const unsigned char *>(table);
    for (size_t i = 0; i < (size_t)n * sizeof(fk_strategy); ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

// The first adding call fixes (n, range, table, family); every later one repeats them.  `fresh`: this call is the first.
static int rr_counts_match(fk_ctx *c, const fk_strategy *table, int32_t n, uint64_t pair_begin, uint64_t pair_end, uint64_t family_pair_count,
                           uint64_t &hash, bool &fresh) {
    if (pair_begin == pair_end) return fail(c, FK_ERR_ARG, "resident counts need a pair range that is not empty");
    if (pair_end - pair_begin > 0x7fffffffull) return fail(c, FK_ERR_ARG, "resident counts hold at most 2^31 - 1 pairs");
    if (family_pair_count < pair_end - pair_begin)
        return fail(c, FK_ERR_ARG, "family_pair_count %llu is smaller than the %llu pairs of the range", (unsigned long long)family_pair_count,
                    (unsigned long long)(pair_end - pair_begin));
    hash = rr_table_hash(table, n);
    fresh = !c->ri_valid;
    if (!fresh && (n != c->ri_n || pair_begin != c->ri_begin || pair_end != c->ri_end || hash != c->ri_hash || family_pair_count != c->ri_family))
        return fail(c, FK_ERR_ARG,
                    "the resident counts were begun for pairs [%llu, %llu) of a table of %d strategies and a family of %llu pairs: this call's "
                    "table, range or family differs (fk_rr_counts_reset starts over)",
                    (unsigned long long)c->ri_begin, (unsigned long long)c->ri_end, (int)c->ri_n, (unsigned long long)c->ri_family);
    return FK_OK;
}

// Option "rr_keep_roots": the root slot this adding call's states go to, -1 for none (option off, or the root set is untracked already).
// Refuses, before any device work, a seed that is kept already and a root beyond the slots.
static int rr_root_slot(fk_ctx *c, uint64_t root_seed, int &slot) {
    slot = -1;
    if (!c->ri_keep_roots || c->ri_untracked) return FK_OK;
    for (int32_t r = 0; r < c->ri_roots; ++r)
        if (c->ri_root_seed[r] == root_seed)
            return fail(c, FK_ERR_ARG, "root_seed %llu is kept already: the kept roots are distinct", (unsigned long long)root_seed);
    if (c->ri_roots >= FK_RR_MAX_ROOTS)
        return fail(c, FK_ERR_ARG, "%d roots are kept already: fk_rr_root_diagnostics admits one or two roots", (int)c->ri_roots);
    slot = c->ri_roots;
    return FK_OK;
}

static void rr_root_keep(fk_ctx *c, int slot, uint64_t root_seed, uint64_t target, uint64_t max_attempts) { // the call has succeeded
    if (slot < 0) return;
    c->ri_root_seed[slot] = root_seed, c->ri_root_target[slot] = target, c->ri_root_cap[slot] = max_attempts;
    c->ri_roots = slot + 1;
}

// room for the call's states (and the root slot they are kept in) and, on a first call, a zeroed accumulator (it counts as resident only
// once the call has succeeded)
static int rr_counts_prepare(fk_ctx *c, uint64_t n_pairs, bool fresh, int slot = -1) {
    HIPCHK(c, hipSetDevice(c->device));
    if (const int rc = ensure_all(c, c->ri.counts, (size_t)n_pairs * 2 * fkri::RI_COLS, c->ri.staged, (size_t)n_pairs * 2 * fkrr::RR_STATE)) return rc;
    if (slot >= 0)
        if (const int rc = ensure(c, c->ri.root_states[slot], (size_t)n_pairs * 2 * fkrr::RR_STATE)) return rc;
    if (fresh) HIPCHK(c, hipMemsetAsync(c->ri.counts.p, 0, (size_t)n_pairs * 2 * fkri::RI_COLS * 8, c->stream));
    return FK_OK;
}

static void rr_counts_fix(fk_ctx *c, int32_t n, uint64_t pair_begin, uint64_t pair_end, uint64_t hash, uint64_t family_pair_count) {
    c->ri_valid = true;
    c->ri_n = n, c->ri_begin = pair_begin, c->ri_end = pair_end, c->ri_hash = hash, c->ri_family = family_pair_count;
}

int fk_h2h_round_robin_resident(fk_ctx *c, const fk_strategy *table, int32_t n, uint64_t root_seed, uint64_t pair_begin, uint64_t pair_end,
                                uint64_t target, uint64_t max_attempts, int32_t target_score, int32_t max_rounds, int64_t *summary,
                                uint64_t family_pair_count) {
    if (!c) return FK_ERR_ARG;
    LaunchPlan plan{};
    int rc = round_robin_check(c, table, n, pair_begin, pair_end, target, max_attempts, target_score, max_rounds, plan);
    if (rc) return rc;
    uint64_t hash = 0;
    bool fresh = false;
    if ((rc = rr_counts_match(c, table, n, pair_begin, pair_end, family_pair_count, hash, fresh))) return rc;
    int slot = -1;
    if ((rc = rr_root_slot(c, root_seed, slot))) return rc;
    rc = replay_on_oom(c, [&] {
        if (const int r = rr_counts_prepare(c, pair_end - pair_begin, fresh, slot)) return r;
        return h2h_round_robin_impl(c, table, n, root_seed, pair_begin, pair_end, target, max_attempts, target_score, max_rounds, plan, nullptr, summary,
                                    c->ri.staged.p, slot >= 0 ? c->ri.root_states[slot].p : nullptr);
    });
    if (rc == FK_OK) {
        rr_counts_fix(c, n, pair_begin, pair_end, hash, family_pair_count);
        rr_root_keep(c, slot, root_seed, target, max_attempts);
    }
    return rc;
}

// fk_rr_counts_add (root_seed null) and fk_rr_counts_add_root
static int rr_counts_add_impl(fk_ctx *c, const fk_strategy *table, int32_t n, uint64_t pair_begin, uint64_t pair_end, uint64_t target,
                              uint64_t max_attempts, const uint32_t *block_state, uint64_t family_pair_count, const uint64_t *root_seed) {
    if (!c) return FK_ERR_ARG;
    if (!table || !block_state) return fail(c, FK_ERR_ARG, "the strategy table and block_state are required");
    if (n < 2) return fail(c, FK_ERR_ARG, "a round robin needs at least two strategies, got %d", (int)n);
    const uint64_t all_pairs = (uint64_t)n * (uint64_t)(n - 1) / 2u;
    if (pair_begin > pair_end || pair_end > all_pairs)
        return fail(c, FK_ERR_ARG, "pair range [%llu, %llu) is not inside the %llu pairs of %d strategies", (unsigned long long)pair_begin,
                    (unsigned long long)pair_end, (unsigned long long)all_pairs, (int)n);
    if (target == 0 || target > max_attempts || max_attempts > 0x7fffffffull)
        return fail(c, FK_ERR_ARG, "target must be in [1, max_attempts] and max_attempts at most 2^31 - 1");
    uint64_t hash = 0;
    bool fresh = false;
    int rc = rr_counts_match(c, table, n, pair_begin, pair_end, family_pair_count, hash, fresh);
    if (rc) return rc;
    const uint64_t n_rows = 2u * (pair_end - pair_begin);
    for (uint64_t row = 0; row < n_rows; ++row) { // a state no block can end in would poison the sums
        const uint32_t *s = block_state + row * fkrr::RR_STATE;
        if (s[0] > max_attempts || s[1] > target || (uint64_t)s[1] + s[2] != s[0] || (uint64_t)s[3] + s[4] != s[1])
            return fail(c, FK_ERR_ARG, "block_state of pair %llu, order %u is not a state of a block with target %llu and max_attempts %llu",
                        (unsigned long long)(pair_begin + row / 2u), (unsigned)(row & 1u), (unsigned long long)target, (unsigned long long)max_attempts);
    }
    int slot = -1;
    if (root_seed && (rc = rr_root_slot(c, *root_seed, slot))) return rc;
    if ((rc = rr_counts_prepare(c, pair_end - pair_begin, fresh, slot))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->ri.staged.p, block_state, (size_t)n_rows * fkrr::RR_STATE * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(fkri::fk_ri_add_kernel, dim3((uint32_t)((n_rows + 255u) / 256u)), dim3(256), 0, c->stream, c->ri.staged.p, n_rows, (uint32_t)target,
                       (uint32_t)max_attempts, c->ri.counts.p);
    HIPCHK(c, hipGetLastError());
    if (slot >= 0)
        HIPCHK(c, hipMemcpyAsync(c->ri.root_states[slot].p, c->ri.staged.p, (size_t)n_rows * fkrr::RR_STATE * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rr_counts_fix(c, n, pair_begin, pair_end, hash, family_pair_count);
    if (root_seed) rr_root_keep(c, slot, *root_seed, target, max_attempts);
    else if (c->ri_keep_roots) c->ri_untracked = true; // the accumulator now holds cells that no slot holds
    return FK_OK;
}

int fk_rr_counts_add(fk_ctx *c, const fk_strategy *table, int32_t n, uint64_t pair_begin, uint64_t pair_end, uint64_t target, uint64_t max_attempts,
                     const uint32_t *block_state, uint64_t family_pair_count) {
    return rr_counts_add_impl(c, table, n, pair_begin, pair_end, target, max_attempts, block_state, family_pair_count, nullptr);
}

int fk_rr_counts_add_root(fk_ctx *c, const fk_strategy *table, int32_t n, uint64_t pair_begin, uint64_t pair_end, uint64_t target,
                          uint64_t max_attempts, const uint32_t *block_state, uint64_t family_pair_count, uint64_t root_seed) {
    return rr_counts_add_impl(c, table, n, pair_begin, pair_end, target, max_attempts, block_state, family_pair_count, &root_seed);
}

int fk_rr_counts_reset(fk_ctx *c) {
    if (!c) return FK_ERR_ARG;
    c->ri_valid = false;
    c->ri_roots = 0, c->ri_untracked = false; // the root slots are forgotten with the accumulator
    return FK_OK;
}

// fk_rr_inference's refusals; fk_rr_dominance makes them too
static int rr_inference_check(fk_ctx *c, const fk_rr_inference_params *par, bool rows, uint64_t row_begin, uint64_t row_end,
                              const int64_t *class_counts) {
    if (!par || !class_counts) return fail(c, FK_ERR_ARG, "params and class_counts are required");
    if (!c->ri_valid) return fail(c, FK_ERR_ARG, "no resident counts: fk_h2h_round_robin_resident or fk_rr_counts_add comes first");
    if (rows && (row_begin > row_end || row_begin < c->ri_begin || row_end > c->ri_end))
        return fail(c, FK_ERR_ARG, "row range [%llu, %llu) is not inside the resident pair range [%llu, %llu)", (unsigned long long)row_begin,
                    (unsigned long long)row_end, (unsigned long long)c->ri_begin, (unsigned long long)c->ri_end);
    if (!(par->family_alpha > 0.0 && par->family_alpha < 1.0)) return fail(c, FK_ERR_ARG, "family_alpha must be in (0, 1), got %g", par->family_alpha);
    if (!(par->practical_delta > 0.0)) return fail(c, FK_ERR_ARG, "practical_delta must be positive, got %g", par->practical_delta);
    if (!std::isnan(par->delta_equivalence) && !(par->delta_equivalence > 0.0 && par->delta_equivalence < 1.0))
        return fail(c, FK_ERR_ARG, "delta_equivalence must be in (0, 1) or NaN (off), got %g", par->delta_equivalence);
    if (!(par->min_candidate_completion_rate >= 0.0 && par->min_candidate_completion_rate <= 1.0))
        return fail(c, FK_ERR_ARG, "min_candidate_completion_rate must be in [0, 1], got %g", par->min_candidate_completion_rate);
    const uint64_t n_pairs64 = c->ri_end - c->ri_begin;
    if (par->family_pair_count < n_pairs64)
        return fail(c, FK_ERR_ARG, "family_pair_count %llu is smaller than the %llu pairs of the resident range", (unsigned long long)par->family_pair_count,
                    (unsigned long long)n_pairs64);
    if (par->family_pair_count != c->ri_family)
        return fail(c, FK_ERR_ARG, "family_pair_count %llu is not the %llu fixed with the resident counts", (unsigned long long)par->family_pair_count,
                    (unsigned long long)c->ri_family);
    if (!(par->critical_ordinary > 0.0 && std::isfinite(par->critical_ordinary) && par->critical_simultaneous > 0.0 && std::isfinite(par->critical_simultaneous)))
        return fail(c, FK_ERR_ARG, "the critical values must be positive and finite, got %g and %g", par->critical_ordinary, par->critical_simultaneous);
    return FK_OK;
}

// The chain of fk_rr_inference on the context's stream, after begin_call: its device work and the copies home, not yet awaited.
// `cls_out`, nullable: [pairs] on the device, every pair's class (fk_rr_dominance).
static int rr_inference_enqueue(fk_ctx *c, const fk_rr_inference_params *par, fk_rr_pair_row *rows, uint64_t row_begin, uint64_t row_end,
                                int64_t *class_counts, int64_t *strategy_classes, uint8_t *cls_out) {
    using namespace fkri;
    const uint64_t n_pairs64 = c->ri_end - c->ri_begin;
    RrInferenceBufs &b = c->ri;
    const uint32_t P = (uint32_t)n_pairs64, n = (uint32_t)c->ri_n;
    const size_t n_rows_out = rows ? (size_t)(row_end - row_begin) : 0;
    int rc = FK_OK;
    if ((rc = ensure_all(c, b.sums, (size_t)n * RI_SUMS, b.strat_flags, (size_t)n, b.key, (size_t)P, b.key_sorted, (size_t)P, b.val, (size_t)P, b.val_sorted,
                         (size_t)P, b.sim, (size_t)P, b.scaled, (size_t)P, b.running, (size_t)P, b.adjusted, (size_t)P, b.position, (size_t)P, b.class_counts, (size_t)RI_CLASSES,
                         b.strat_out, (size_t)n * RI_STRAT_COLS, b.rows, n_rows_out)))
        return rc;
    Timer device_work(c, &c->timing.play_ms, SLOT_PLAY); // fk_timing: play_ms = total_ms = the entry's device work, copies back excluded
    HIPCHK(c, hipMemsetAsync(b.sums.p, 0, (size_t)n * RI_SUMS * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(b.class_counts.p, 0, RI_CLASSES * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(b.strat_out.p, 0, (size_t)n * RI_STRAT_COLS * 8, c->stream));
    const dim3 pair_grid((P + 255u) / 256u), b256(256);
    hipLaunchKernelGGL(fk_ri_pair_kernel<true>, pair_grid, b256, 0, c->stream, b.counts.p, n, c->ri_begin, P, par->critical_simultaneous, b.sums.p, b.key.p,
                       b.val.p, b.sim.p, (uint8_t *)nullptr);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(fk_ri_strategy_kernel, dim3((n + 255u) / 256u), b256, 0, c->stream, b.sums.p, n, par->min_candidate_completion_rate, b.strat_flags.p,
                       b.strat_out.p);
    HIPCHK(c, hipGetLastError());
    // Holm: a stable sort of the p-values' bit patterns (ties keep pair order, as argsort(kind="mergesort")), scale, running maximum, scatter
    FK_CUB(hipcub::DeviceRadixSort::SortPairs, b.key.p, b.key_sorted.p, b.val.p, b.val_sorted.p, (int)P, 0, 64, c->stream);
    hipLaunchKernelGGL(fk_ri_holm_scale_kernel, pair_grid, b256, 0, c->stream, b.key_sorted.p, P, b.scaled.p);
    HIPCHK(c, hipGetLastError());
    FK_CUB(hipcub::DeviceScan::InclusiveScan, b.scaled.p, b.running.p, hipcub::Max(), (int)P, c->stream);
    hipLaunchKernelGGL(fk_ri_holm_scatter_kernel, pair_grid, b256, 0, c->stream, b.running.p, b.val_sorted.p, P, b.adjusted.p, b.position.p);
    HIPCHK(c, hipGetLastError());
    const DecideParams dp{par->family_alpha, par->practical_delta, par->delta_equivalence, par->critical_ordinary};
    const uint32_t row_first = rows ? (uint32_t)(row_begin - c->ri_begin) : 0u, row_last = rows ? (uint32_t)(row_end - c->ri_begin) : 0u;
    hipLaunchKernelGGL(fk_ri_decide_kernel, pair_grid, b256, 0, c->stream, b.counts.p, n, c->ri_begin, P, dp, b.strat_flags.p, b.sim.p, b.adjusted.p, b.position.p,
                       b.class_counts.p, b.strat_out.p, row_first, row_last, n_rows_out ? b.rows.p : nullptr, cls_out);
    HIPCHK(c, hipGetLastError());
    device_work.stop();
    HIPCHK(c, hipMemcpyAsync(class_counts, b.class_counts.p, RI_CLASSES * 8, hipMemcpyDeviceToHost, c->stream));
    if (strategy_classes) HIPCHK(c, hipMemcpyAsync(strategy_classes, b.strat_out.p, (size_t)n * RI_STRAT_COLS * 8, hipMemcpyDeviceToHost, c->stream));
    if (n_rows_out) HIPCHK(c, hipMemcpyAsync(rows, b.rows.p, n_rows_out * sizeof(fk_rr_pair_row), hipMemcpyDeviceToHost, c->stream));
    return FK_OK;
}

int fk_rr_inference(fk_ctx *c, const fk_rr_inference_params *par, fk_rr_pair_row *rows, uint64_t row_begin, uint64_t row_end, int64_t *class_counts,
                    int64_t *strategy_classes) {
    if (!c) return FK_ERR_ARG;
    if (const int rc = rr_inference_check(c, par, rows != nullptr, row_begin, row_end, class_counts)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);
    if (const int rc = rr_inference_enqueue(c, par, rows, row_begin, row_end, class_counts, strategy_classes, nullptr)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, collect_timers(c));
    c->timing.total_ms = c->timing.play_ms;
    return FK_OK;
}

// ---- the inference per kept root and the cross-root agreement (device side: fk_rr_root_diagnostics.h) ----
int fk_rr_root_diagnostics(fk_ctx *c, const fk_rr_inference_params *par, uint64_t *root_seeds, int32_t *n_roots, fk_rr_root_row *rows, uint64_t row_begin,
                           uint64_t row_end, fk_rr_agreement_row *agreement, int64_t *summary, double *max_abs_discrepancy) {
    using namespace fkri;
    if (!c) return FK_ERR_ARG;
    if (!par || !root_seeds || !n_roots || !summary) return fail(c, FK_ERR_ARG, "params, root_seeds, n_roots and summary are required");
    if (const int rc = rr_inference_check(c, par, rows || agreement, row_begin, row_end, summary)) return rc;
    if (c->ri_untracked)
        return fail(c, FK_ERR_ARG, "the root set is untracked: fk_rr_counts_add added counts that no root slot holds (fk_rr_counts_add_root keeps them)");
    if (c->ri_roots == 0) return fail(c, FK_ERR_ARG, "no kept roots: option rr_keep_roots comes before the adding calls");
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);
    RrInferenceBufs &b = c->ri;
    const uint32_t P = (uint32_t)(c->ri_end - c->ri_begin), n = (uint32_t)c->ri_n, R = (uint32_t)c->ri_roots;
    uint32_t slot_of[FK_RR_MAX_ROOTS] = {0u, 1u}; // ascending seed, unsigned
    if (R == 2u && c->ri_root_seed[1] < c->ri_root_seed[0]) slot_of[0] = 1u, slot_of[1] = 0u;
    const bool sliced = rows || agreement;
    const size_t n_rows_out = sliced ? (size_t)(row_end - row_begin) : 0;
    int rc = FK_OK;
    if ((rc = ensure_all(c, b.sums, (size_t)n * RI_SUMS, b.strat_flags, (size_t)n, b.strat_out, (size_t)n * RI_STRAT_COLS, b.viable, (size_t)P, b.key, (size_t)P,
                         b.key_sorted, (size_t)P, b.val, (size_t)P, b.val_sorted, (size_t)P, b.scaled, (size_t)P, b.running, (size_t)P, b.adjusted, (size_t)P,
                         b.position, (size_t)P, b.root_effect, (size_t)R * P, b.root_decision, (size_t)R * P, b.agree_summary, (size_t)RD_COLS + 1,
                         b.root_rows, rows ? (size_t)R * n_rows_out : 0, b.agree_rows, agreement ? n_rows_out : 0)))
        return rc;
    Timer device_work(c, &c->timing.play_ms, SLOT_PLAY); // fk_timing: play_ms = total_ms = the entry's device work, copies back excluded
    HIPCHK(c, hipMemsetAsync(b.sums.p, 0, (size_t)n * RI_SUMS * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(b.agree_summary.p, 0, ((size_t)RD_COLS + 1) * 8, c->stream));
    const dim3 pair_grid((P + 255u) / 256u), b256(256);
    // 1. the combined viability and the strategies' flags, without the interval
    hipLaunchKernelGGL(fk_ri_pair_kernel<false>, pair_grid, b256, 0, c->stream, b.counts.p, n, c->ri_begin, P, 0.0, b.sums.p, (unsigned long long *)nullptr,
                       (uint32_t *)nullptr, (double2 *)nullptr, b.viable.p);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(fk_ri_strategy_kernel, dim3((n + 255u) / 256u), b256, 0, c->stream, b.sums.p, n, par->min_candidate_completion_rate, b.strat_flags.p,
                       b.strat_out.p);
    HIPCHK(c, hipGetLastError());
    const uint32_t row_first = sliced ? (uint32_t)(row_begin - c->ri_begin) : 0u, row_last = sliced ? (uint32_t)(row_end - c->ri_begin) : 0u;
    // 2. per kept root: the score test, Holm as the combined chain does it, the decisions and the rows
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t *state = b.root_states[slot_of[r]].p;
        double *effect = b.root_effect.p + (size_t)r * P;
        hipLaunchKernelGGL(fk_rd_test_kernel, pair_grid, b256, 0, c->stream, state, b.viable.p, P, b.key.p, b.val.p, effect);
        HIPCHK(c, hipGetLastError());
        FK_CUB(hipcub::DeviceRadixSort::SortPairs, b.key.p, b.key_sorted.p, b.val.p, b.val_sorted.p, (int)P, 0, 64, c->stream);
        hipLaunchKernelGGL(fk_ri_holm_scale_kernel, pair_grid, b256, 0, c->stream, b.key_sorted.p, P, b.scaled.p);
        HIPCHK(c, hipGetLastError());
        FK_CUB(hipcub::DeviceScan::InclusiveScan, b.scaled.p, b.running.p, hipcub::Max(), (int)P, c->stream);
        hipLaunchKernelGGL(fk_ri_holm_scatter_kernel, pair_grid, b256, 0, c->stream, b.running.p, b.val_sorted.p, P, b.adjusted.p, b.position.p);
        HIPCHK(c, hipGetLastError());
        fk_rr_root_row *d_rows = rows && n_rows_out ? b.root_rows.p + (size_t)r * n_rows_out : nullptr;
        hipLaunchKernelGGL(d_rows ? fk_rd_decide_kernel<true> : fk_rd_decide_kernel<false>, pair_grid, b256, 0, c->stream, state, b.viable.p, n, c->ri_begin, P,
                           par->family_alpha, par->critical_ordinary, b.strat_flags.p, effect, b.adjusted.p, b.position.p,
                           b.agree_summary.p + RD_ROOT0 + (size_t)r * RD_ROOT_COLS, b.root_decision.p + (size_t)r * P, row_first, row_last, d_rows);
        HIPCHK(c, hipGetLastError());
    }
    // 3. the agreement
    hipLaunchKernelGGL(fk_rd_agree_kernel, pair_grid, b256, 0, c->stream, n, c->ri_begin, P, R, b.root_effect.p, b.root_decision.p, b.agree_summary.p, row_first,
                       row_last, agreement && n_rows_out ? b.agree_rows.p : nullptr);
    HIPCHK(c, hipGetLastError());
    device_work.stop();
    unsigned long long out[RD_COLS + 1];
    HIPCHK(c, hipMemcpyAsync(out, b.agree_summary.p, sizeof(out), hipMemcpyDeviceToHost, c->stream));
    if (rows && n_rows_out) HIPCHK(c, hipMemcpyAsync(rows, b.root_rows.p, (size_t)R * n_rows_out * sizeof(fk_rr_root_row), hipMemcpyDeviceToHost, c->stream));
    if (agreement && n_rows_out)
        HIPCHK(c, hipMemcpyAsync(agreement, b.agree_rows.p, n_rows_out * sizeof(fk_rr_agreement_row), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, collect_timers(c));
    c->timing.total_ms = c->timing.play_ms;
    for (uint32_t k = 0; k < RD_COLS; ++k) summary[k] = (int64_t)out[k];
    if (max_abs_discrepancy) {
        double largest = NAN;
        if (out[RD_AVAILABLE]) memcpy(&largest, &out[RD_COLS], sizeof(largest));
        *max_abs_discrepancy = largest;
    }
    for (uint32_t r = 0; r < FK_RR_MAX_ROOTS; ++r) root_seeds[r] = r < R ? c->ri_root_seed[slot_of[r]] : 0u;
    *n_roots = (int32_t)R;
    return FK_OK;
}

// ---- dominance graphs of a round robin (device side: fk_dominance.h) ----
static int dominance_check_shape(fk_ctx *c, int64_t n, const uint32_t *rank, const void *nodes, const void *extremes) {
    if (!nodes || !extremes) return fail(c, FK_ERR_ARG, "nodes and extremes are required");
    if (n < 2) return fail(c, FK_ERR_ARG, "a dominance graph needs at least two strategies, got %lld", (long long)n);
    if (n > FK_DOM_MAX_N)
        return fail(c, FK_ERR_ARG, "a dominance graph holds at most %d strategies (the fronts' in-degrees live in one workgroup's LDS), got %lld", FK_DOM_MAX_N,
                    (long long)n);
    if (rank) {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int64_t i = 0; i < n; ++i) {
            if (rank[i] >= (uint64_t)n || seen[rank[i]]) return fail(c, FK_ERR_ARG, "rank is not a permutation of 0 .. %lld (entry %lld)", (long long)n - 1, (long long)i);
            seen[rank[i]] = 1;
        }
    }
    return FK_OK;
}

// The graph stage on the context's stream, classes / bounds / rates on the device; awaits it and copies home.
static int dominance_run(fk_ctx *c, uint32_t n, const uint8_t *d_cls, const double2 *d_sim, const double *d_rate, double delta, const uint32_t *rank,
                         fk_dom_node *nodes, fk_dom_extreme *extremes, uint64_t *adjacency) {
    using namespace fkdm;
    DominanceBufs &b = c->dm;
    const uint32_t P = (uint32_t)((uint64_t)n * (n - 1u) / 2u);
    const fkl::DominanceMats lay(n);
    const fkl::DominanceKeys keys(n);
    int rc = FK_OK;
    if ((rc = ensure_all(c, b.mats, lay.n_u64, b.keys, keys.n_u64, b.comp, (size_t)2 * n, b.comp_deg, (size_t)2 * n, b.rank, (size_t)n, b.unrank, (size_t)n, b.nodes,
                         (size_t)n, b.extremes, (size_t)2 * n)))
        return rc;
    if (rank) {
        std::vector<uint32_t> inverse(n);
        for (uint32_t i = 0; i < n; ++i) inverse[rank[i]] = i;
        HIPCHK(c, hipMemcpyAsync(b.rank.p, rank, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.unrank.p, inverse.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); // (`inverse` leaves scope)
    }
    const uint32_t W = (uint32_t)lay.W;
    const Mats m{b.mats.p + lay.adj, b.mats.p + lay.adj_t, b.mats.p + lay.reach, n, W};
    const ExtremeBufs e{b.keys.p + keys.max_bits, b.keys.p + keys.min_bits, b.keys.p + keys.strong_key, b.keys.p + keys.weak_key};
    const dim3 pair_grid((P + 255u) / 256u), b256(256);
    Timer device_work(c, &c->timing.play_ms, SLOT_CALL);
    Timer edges(c, &c->timing.perm_ms, SLOT_PERM);
    HIPCHK(c, hipMemsetAsync(b.mats.p, 0, 4 * lay.plane * 8, c->stream)); // adj, adj_t
    hipLaunchKernelGGL(fk_dm_edges_kernel, pair_grid, b256, 0, c->stream, d_cls, n, P, m);
    HIPCHK(c, hipGetLastError());
    edges.stop();
    Timer closure(c, &c->timing.seed_ms, SLOT_SEED);
    HIPCHK(c, hipMemcpyAsync(m.reach, m.adj, 4 * lay.plane * 8, hipMemcpyDeviceToDevice, c->stream)); // adj[0], adj[1], adj_t[0], adj_t[1]
    for (uint32_t kb = 0; kb < W; ++kb) {
        hipLaunchKernelGGL(fk_dm_panel_kernel, dim3(4), b256, 0, c->stream, m.reach, n, W, kb, b.mats.p + lay.panel, b.mats.p + lay.dstar);
        hipLaunchKernelGGL(fk_dm_close_kernel, dim3((n + 3u) / 4u, 4), b256, 0, c->stream, m.reach, n, W, kb, b.mats.p + lay.panel, b.mats.p + lay.dstar);
    }
    HIPCHK(c, hipGetLastError());
    closure.stop();
    HIPCHK(c, hipMemsetAsync(b.comp_deg.p, 0, (size_t)2 * n * 4, c->stream));
    hipLaunchKernelGGL(fk_dm_component_kernel, dim3((n + 3u) / 4u, 2), b256, 0, c->stream, m, b.nodes.p, b.comp.p, b.comp_deg.p);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(fk_dm_front_kernel, dim3(2), dim3(1024), 0, c->stream, m, b.nodes.p, b.comp.p, b.comp_deg.p);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(fk_dm_mean_kernel, dim3((n + 255u) / 256u), b256, 0, c->stream, d_rate, n, b.nodes.p);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(fk_dm_cycle_kernel, dim3(n, 2), dim3(128), 0, c->stream, m, b.nodes.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemsetAsync(e.max_bits, 0, (size_t)2 * n * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(e.min_bits, 0xff, (size_t)6 * n * 8, c->stream)); // min_bits, strong_key, weak_key
    for (const bool second : {false, true}) {
        hipLaunchKernelGGL(fk_dm_extreme_kernel, pair_grid, b256, 0, c->stream, d_cls, d_sim, delta, n, P, b.comp.p, rank ? b.rank.p : nullptr, e, second);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(fk_dm_extreme_out_kernel, dim3((2u * n + 255u) / 256u), b256, 0, c->stream, n, rank ? b.unrank.p : nullptr, e, b.extremes.p);
    HIPCHK(c, hipGetLastError());
    device_work.stop();
    HIPCHK(c, hipMemcpyAsync(nodes, b.nodes.p, (size_t)n * sizeof(fk_dom_node), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(extremes, b.extremes.p, (size_t)2 * n * sizeof(fk_dom_extreme), hipMemcpyDeviceToHost, c->stream));
    if (adjacency) HIPCHK(c, hipMemcpyAsync(adjacency, m.adj, 2 * lay.plane * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, collect_timers(c));
    c->timing.total_ms = c->timing.play_ms;
    return FK_OK;
}

int fk_dominance_graph(fk_ctx *c, int32_t n, const uint8_t *decision_class, const double *sim_d_low, const double *sim_d_high, const double *balanced_rate,
                       double practical_delta, const uint32_t *rank, fk_dom_node *nodes, fk_dom_extreme *extremes, uint64_t *adjacency) {
    if (!c) return FK_ERR_ARG;
    if (const int rc = dominance_check_shape(c, n, rank, nodes, extremes)) return rc;
    if (!decision_class || !sim_d_low || !sim_d_high || !balanced_rate) return fail(c, FK_ERR_ARG, "the class, bound and rate arrays are required");
    if (!(practical_delta > 0.0)) return fail(c, FK_ERR_ARG, "practical_delta must be positive, got %g", practical_delta);
    const size_t P = (size_t)n * (size_t)(n - 1) / 2u;
    std::vector<double2> sim(P);
    for (size_t p = 0; p < P; ++p) {
        const uint8_t cls = decision_class[p];
        if (cls >= fkri::RI_CLASSES) return fail(c, FK_ERR_ARG, "decision class %u of pair %zu is not one of the %u classes", (unsigned)cls, p, fkri::RI_CLASSES);
        if (cls < 2u && !std::isfinite(cls == 0u ? sim_d_low[p] : sim_d_high[p]))
            return fail(c, FK_ERR_ARG, "pair %zu is a practical dominance whose simultaneous bound is not finite", p);
        sim[p] = make_double2(sim_d_low[p], sim_d_high[p]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);
    DominanceBufs &b = c->dm;
    if (const int rc = ensure_all(c, b.cls, P, b.sim, P, b.rate, P)) return rc;
    HIPCHK(c, hipMemcpyAsync(b.cls.p, decision_class, P, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.sim.p, sim.data(), P * sizeof(double2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.rate.p, balanced_rate, P * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (`sim` is pageable memory of this frame)
    return dominance_run(c, (uint32_t)n, b.cls.p, b.sim.p, b.rate.p, practical_delta, rank, nodes, extremes, adjacency);
}

int fk_rr_dominance(fk_ctx *c, const fk_rr_inference_params *par, const uint32_t *rank, fk_dom_node *nodes, fk_dom_extreme *extremes, uint64_t *adjacency,
                    int64_t *class_counts) {
    if (!c) return FK_ERR_ARG;
    if (const int rc = rr_inference_check(c, par, false, 0, 0, class_counts)) return rc;
    const uint64_t all_pairs = (uint64_t)c->ri_n * (uint64_t)(c->ri_n - 1) / 2u;
    if (c->ri_begin != 0 || c->ri_end != all_pairs)
        return fail(c, FK_ERR_ARG, "the resident counts hold pairs [%llu, %llu) of the table's %llu: a dominance graph needs the whole family",
                    (unsigned long long)c->ri_begin, (unsigned long long)c->ri_end, (unsigned long long)all_pairs);
    if (const int rc = dominance_check_shape(c, c->ri_n, rank, nodes, extremes)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);
    DominanceBufs &b = c->dm;
    const uint32_t P = (uint32_t)all_pairs;
    if (const int rc = ensure_all(c, b.cls, (size_t)P, b.rate, (size_t)P)) return rc;
    if (const int rc = rr_inference_enqueue(c, par, nullptr, 0, 0, class_counts, nullptr, b.cls.p)) return rc;
    hipLaunchKernelGGL(fkdm::fk_dm_rate_kernel, dim3((P + 255u) / 256u), dim3(256), 0, c->stream, c->ri.counts.p, P, b.rate.p);
    HIPCHK(c, hipGetLastError());
    return dominance_run(c, (uint32_t)c->ri_n, b.cls.p, c->ri.sim.p, b.rate.p, par->practical_delta, rank, nodes, extremes, adjacency);
}

// ---- method agreement of a round robin (device side: fk_agreement.h) ----
static int agreement_check_ranks(fk_ctx *c, int64_t n, const int32_t *win_rate_rank, const int32_t *trueskill_rank, const void *counts) {
    if (!win_rate_rank || !trueskill_rank || !counts) return fail(c, FK_ERR_ARG, "win_rate_rank, trueskill_rank and counts are required");
    for (int64_t i = 0; i < n; ++i)
        if (win_rate_rank[i] < 0 || trueskill_rank[i] < 0)
            return fail(c, FK_ERR_ARG, "row %lld has a negative rank (%d, %d): a rank is at least 1, FK_AGREE_NO_RANK = 0 is null", (long long)i,
                        (int)win_rate_rank[i], (int)trueskill_rank[i]);
    return FK_OK;
}

// the rank pairs of the table's rows to the device, awaited: nothing else is on the stream yet
static int agreement_put_ranks(fk_ctx *c, uint32_t n, const int32_t *win_rate_rank, const int32_t *trueskill_rank) {
    if (const int rc = ensure(c, c->ag.ranks, (size_t)n)) return rc;
    std::vector<int2> ranks(n);
    for (uint32_t i = 0; i < n; ++i) ranks[i] = make_int2(win_rate_rank[i], trueskill_rank[i]);
    HIPCHK(c, hipMemcpyAsync(c->ag.ranks.p, ranks.data(), (size_t)n * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (`ranks` leaves scope)
    return FK_OK;
}

// The pair pass on the context's stream, classes and ranks on the device; awaits it and copies home.
static int agreement_run(fk_ctx *c, uint32_t n, const uint8_t *d_cls, uint8_t *codes, int64_t *counts) {
    using namespace fkag;
    AgreementBufs &b = c->ag;
    const uint32_t P = (uint32_t)((uint64_t)n * (n - 1u) / 2u);
    if (const int rc = ensure_all(c, b.counts, (size_t)AG_COUNTS, b.codes, codes ? (size_t)P : 0)) return rc;
    const uint32_t cap = c->agreement_grid > 0 ? (uint32_t)std::min<int64_t>(c->agreement_grid, AG_MAX_GRID) : AG_MAX_GRID;
    const uint32_t grid = std::min<uint32_t>((P + AG_BLOCK - 1u) / AG_BLOCK, cap);
    Timer device_work(c, &c->timing.play_ms, SLOT_CALL);
    Timer pairs(c, &c->timing.perm_ms, SLOT_PERM);
    HIPCHK(c, hipMemsetAsync(b.counts.p, 0, AG_COUNTS * 8, c->stream));
    hipLaunchKernelGGL(fk_ag_pairs_kernel, dim3(grid), dim3(AG_BLOCK), 0, c->stream, d_cls, b.ranks.p, n, P, codes ? b.codes.p : nullptr, b.counts.p);
    HIPCHK(c, hipGetLastError());
    pairs.stop();
    device_work.stop();
    unsigned long long out[AG_COUNTS];
    HIPCHK(c, hipMemcpyAsync(out, b.counts.p, sizeof(out), hipMemcpyDeviceToHost, c->stream));
    if (codes) HIPCHK(c, hipMemcpyAsync(codes, b.codes.p, (size_t)P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, collect_timers(c));
    c->timing.total_ms = c->timing.play_ms;
    for (uint32_t k = 0; k < AG_COUNTS; ++k) counts[k] = (int64_t)out[k];
    return FK_OK;
}

int fk_agreement_pairs(fk_ctx *c, int32_t n, const uint8_t *decision_class, const int32_t *win_rate_rank, const int32_t *trueskill_rank, uint8_t *codes,
                       int64_t *counts) {
    if (!c) return FK_ERR_ARG;
    if (n < 2) return fail(c, FK_ERR_ARG, "pair agreement needs at least two strategies, got %d", (int)n);
    const uint64_t all_pairs = (uint64_t)n * (uint64_t)(n - 1) / 2u;
    if (all_pairs > 0x7fffffffull) return fail(c, FK_ERR_ARG, "pair agreement holds at most 2^31 - 1 pairs, %d strategies have %llu", (int)n, (unsigned long long)all_pairs);
    if (!decision_class) return fail(c, FK_ERR_ARG, "decision_class is required");
    if (const int rc = agreement_check_ranks(c, n, win_rate_rank, trueskill_rank, counts)) return rc;
    const size_t P = (size_t)all_pairs;
    for (size_t p = 0; p < P; ++p)
        if (decision_class[p] >= fkri::RI_CLASSES)
            return fail(c, FK_ERR_ARG, "decision class %u of pair %zu is not one of the %u classes", (unsigned)decision_class[p], p, fkri::RI_CLASSES);
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);
    if (const int rc = ensure(c, c->ag.cls, P)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->ag.cls.p, decision_class, P, hipMemcpyHostToDevice, c->stream));
    if (const int rc = agreement_put_ranks(c, (uint32_t)n, win_rate_rank, trueskill_rank)) return rc;
    return agreement_run(c, (uint32_t)n, c->ag.cls.p, codes, counts);
}

int fk_rr_agreement(fk_ctx *c, const fk_rr_inference_params *par, const int32_t *win_rate_rank, const int32_t *trueskill_rank, uint8_t *codes, int64_t *counts,
                    int64_t *class_counts) {
    if (!c) return FK_ERR_ARG;
    if (const int rc = rr_inference_check(c, par, false, 0, 0, class_counts)) return rc;
    const uint64_t all_pairs = (uint64_t)c->ri_n * (uint64_t)(c->ri_n - 1) / 2u;
    if (c->ri_begin != 0 || c->ri_end != all_pairs)
        return fail(c, FK_ERR_ARG, "the resident counts hold pairs [%llu, %llu) of the table's %llu: pair agreement needs the whole family",
                    (unsigned long long)c->ri_begin, (unsigned long long)c->ri_end, (unsigned long long)all_pairs);
    if (const int rc = agreement_check_ranks(c, c->ri_n, win_rate_rank, trueskill_rank, counts)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);
    if (const int rc = ensure(c, c->ag.cls, (size_t)all_pairs)) return rc;
    if (const int rc = agreement_put_ranks(c, (uint32_t)c->ri_n, win_rate_rank, trueskill_rank)) return rc;
    if (const int rc = rr_inference_enqueue(c, par, nullptr, 0, 0, class_counts, nullptr, c->ag.cls.p)) return rc;
    return agreement_run(c, (uint32_t)c->ri_n, c->ag.cls.p, codes, counts);
}

int fk_rank_concordance(fk_ctx *c, int32_t m, const int32_t *x, const int32_t *y, int64_t *counts) {
    using namespace fkag;
    if (!c) return FK_ERR_ARG;
    if (m < 2 || m > FK_CONCORDANCE_MAX_M)
        return fail(c, FK_ERR_ARG, "rank concordance takes 2 to %d items (one workgroup per tile of the comparison), got %d", FK_CONCORDANCE_MAX_M, (int)m);
    if (!x || !y || !counts) return fail(c, FK_ERR_ARG, "x, y and counts are required");
    for (int32_t i = 0; i < m; ++i)
        if (x[i] < 1 || y[i] < 1) return fail(c, FK_ERR_ARG, "item %d has the keys (%d, %d): a key is at least 1", (int)i, (int)x[i], (int)y[i]);
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);
    AgreementBufs &b = c->ag;
    if (const int rc = ensure_all(c, b.x, (size_t)m, b.y, (size_t)m, b.concordance, (size_t)CC_COUNTS)) return rc;
    HIPCHK(c, hipMemcpyAsync(b.x.p, x, (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.y.p, y, (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
    const uint32_t tiles = ((uint32_t)m + CC_TILE - 1u) / CC_TILE;
    Timer device_work(c, &c->timing.play_ms, SLOT_CALL);
    HIPCHK(c, hipMemsetAsync(b.concordance.p, 0, CC_COUNTS * 8, c->stream));
    hipLaunchKernelGGL(fk_ag_concordance_kernel, dim3(tiles * (tiles + 1u) / 2u), dim3(CC_TILE), 0, c->stream, b.x.p, b.y.p, (uint32_t)m, tiles, b.concordance.p);
    HIPCHK(c, hipGetLastError());
    device_work.stop();
    unsigned long long out[CC_COUNTS];
    HIPCHK(c, hipMemcpyAsync(out, b.concordance.p, sizeof(out), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, collect_timers(c));
    c->timing.total_ms = c->timing.play_ms;
    unsigned long long sum = 0;
    for (uint32_t k = 0; k < CC_COUNTS; ++k) sum += out[k];
    const unsigned long long all = (unsigned long long)m * (unsigned long long)(m - 1) / 2u;
    if (sum != all) // every pair i < j falls into exactly one count
        return fail(c, FK_ERR_HIP, "rank concordance lost pairs: the five counts sum to %llu, %d items have %llu pairs", sum, (int)m, all);
    for (uint32_t k = 0; k < CC_COUNTS; ++k) counts[k] = (int64_t)out[k];
    return FK_OK;
}

// ---- exact power of the score test per (sample size, scenario) cell (device side: fk_power_plan.h) ----
// The context's log-factorial table holds lf[0 .. n_max]: filled on the host, the whole table again when it grows.  An entry is libm's
// long-double lgamma rounded to fp64, which h2h_power.log_factorials states with the same libm call: a table off by two units in the last place at n = 20 001 (the fp64 lgamma) moves every mass by 5e-11 of itself.
static int power_plan_table(fk_ctx *c, int32_t n_max) {
    PowerPlanBufs &b = c->pp;
    const size_t want = (size_t)n_max + 1u;
    if (want <= b.lf_n) return FK_OK;
    const size_t entries = std::max<size_t>(want, std::min<size_t>(2u * b.lf_n, (size_t)FK_POWER_MAX_N + 1u)); // (grown on demand, not cell by cell)
    b.lf_n = 0;
    if (const int rc = ensure(c, b.lf, entries)) return rc;
    std::vector<double> lf(entries);
    int sign = 0;
    for (size_t k = 0; k < entries; ++k) lf[k] = k < 2u ? 0.0 : (double)lgammal_r((long double)k + 1.0L, &sign);
    HIPCHK(c, hipMemcpyAsync(b.lf.p, lf.data(), entries * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (`lf` leaves scope)
    b.lf_n = entries;
    return FK_OK;
}

int fk_score_power_scan(fk_ctx *c, const fk_power_cell *cells, int64_t n_cells, double critical_value, double *power) {
    using namespace fkpp;
    if (!c) return FK_ERR_ARG;
    if (n_cells < 0) return fail(c, FK_ERR_ARG, "n_cells must not be negative, got %lld", (long long)n_cells);
    if (n_cells == 0) return FK_OK;
    if (!cells || !power) return fail(c, FK_ERR_ARG, "cells and power are required");
    if (n_cells > 0x7fffffffll) return fail(c, FK_ERR_ARG, "a scan takes at most 2^31 - 1 cells, got %lld", (long long)n_cells);
    if (!std::isfinite(critical_value) || !(critical_value > 0.0))
        return fail(c, FK_ERR_ARG, "critical_value must be finite and positive, got %g", critical_value);
    int32_t n_max = 0;
    for (int64_t i = 0; i < n_cells; ++i) {
        const fk_power_cell &cell = cells[i];
        if (cell.n < 1 || cell.n > FK_POWER_MAX_N)
            return fail(c, FK_ERR_ARG, "cell %lld: n must be in [1, %d], got %d", (long long)i, FK_POWER_MAX_N, (int)cell.n);
        for (const double q : {cell.q_ab, cell.q_ba})
            if (!std::isfinite(q) || !(q > 0.0 && q < 1.0))
                return fail(c, FK_ERR_ARG, "cell %lld: a probability must lie strictly between 0 and 1, got %g", (long long)i, q);
        n_max = std::max(n_max, cell.n);
    }
    HIPCHK(c, hipSetDevice(c->device));
    begin_call(c);
    PowerPlanBufs &b = c->pp;
    // largest first (cost is proportional to n); cells of one size keep the caller's order
    std::vector<uint32_t> order((size_t)n_cells);
    for (uint32_t i = 0; i < (uint32_t)n_cells; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cells[x].n > cells[y].n; });
    std::vector<Cell> sorted((size_t)n_cells);
    uint32_t beyond = 0; // cells whose tails do not fit LDS: the head of the order
    for (size_t at = 0; at < sorted.size(); ++at) {
        const fk_power_cell &cell = cells[order[at]];
        sorted[at] = Cell{cell.n, order[at], std::log(cell.q_ab), std::log1p(-cell.q_ab), std::log(cell.q_ba), std::log1p(-cell.q_ba)};
        beyond += cell.n > FK_POWER_LDS_MAX_N ? 1u : 0u;
    }
    // the workspace: one slot per workgroup of the global kernel, at most PW_WORKSPACE_BYTES in all and one slot at least
    constexpr size_t PW_WORKSPACE_BYTES = (size_t)256 << 20;
    constexpr uint32_t PW_MAX_GRID = 1024;
    const uint64_t slot_entries = beyond ? (uint64_t)n_max + 1u : 0u;
    const uint32_t beyond_grid =
        beyond ? (uint32_t)std::min<uint64_t>(beyond, std::clamp<uint64_t>(PW_WORKSPACE_BYTES / (16u * slot_entries), 1u, PW_MAX_GRID)) : 0u;
    if (const int rc = power_plan_table(c, n_max)) return rc;
    if (const int rc = ensure_all(c, b.cells, (size_t)n_cells, b.power, (size_t)n_cells, b.workspace, (size_t)(2u * slot_entries * beyond_grid))) return rc;
    HIPCHK(c, hipMemcpyAsync(b.cells.p, sorted.data(), sorted.size() * sizeof(Cell), hipMemcpyHostToDevice, c->stream));
    volatile double two = 2.0; // libm's pow itself, which the reference's `critical ** 2` calls: not folded into a product
    const double critical_squared = std::pow(critical_value, two);
    Timer device_work(c, &c->timing.play_ms, SLOT_CALL);
    if (beyond)
        hipLaunchKernelGGL(fk_pp_scan_kernel<false>, dim3(beyond_grid), dim3(PW_BLOCK), 0, c->stream, b.cells.p, beyond, b.lf.p, critical_squared,
                           b.workspace.p, slot_entries, b.power.p);
    const uint32_t within = (uint32_t)n_cells - beyond;
    if (within)
        hipLaunchKernelGGL(fk_pp_scan_kernel<true>, dim3(within), dim3(PW_BLOCK), 0, c->stream, b.cells.p + beyond, within, b.lf.p, critical_squared,
                           (double *)nullptr, (uint64_t)0, b.power.p);
    HIPCHK(c, hipGetLastError());
    device_work.stop();
    HIPCHK(c, hipMemcpyAsync(power, b.power.p, (size_t)n_cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (`sorted` leaves scope)
    HIPCHK(c, collect_timers(c));
    c->timing.total_ms = c->timing.play_ms;
    return FK_OK;
}

// The NEXT fk_tournament_run / _stats call on this context will play shuffles [shuffle_begin, shuffle_end) of the same table,
// k and root seed as the call that follows this hint (need_state: it will ask for rows or all-seat statistics).  That call
// then enqueues the hinted range's permutations and seat seeding on a low-priority stream behind its own game kernel, where
// they fill the kernel's drain tail; the hinted call finds them done.  Purely a scheduling hint: a wrong one wastes work only.
int fk_tournament_hint_next(fk_ctx *c, uint64_t shuffle_begin, uint64_t shuffle_end, int32_t need_state) {
    if (!c) return FK_ERR_ARG;
    if (shuffle_end < shuffle_begin) return fail(c, FK_ERR_ARG, "bad shuffle range");
    c->hint_valid = shuffle_end > shuffle_begin;
    c->hint_begin = shuffle_begin;
    c->hint_end = shuffle_end;
    c->hint_state = need_state ? 1 : 0;
    return FK_OK;
}

// ---- multi-GPU: one RCCL sum of the tally (the analogue of OutcomeCounter.absorb, run_tournament.py:197-213) ----
int fk_comm_unique_id(fk_comm_id *out) {
    if (!out) return FK_ERR_ARG;
    Rccl &r = rccl();
    if (!r.lib) return FK_ERR_COMM;
    return r.GetUniqueId(out) == 0 ? FK_OK : FK_ERR_COMM;
}

// A blocking initialisation under a deadline, on a helper thread.  Ownership of what `init` made is decided by ONE atomic state
// (0 running, 1 done, 2 abandoned): the helper EXCHANGES in "done" when `init` returns and, if the waiter had already abandoned the call,
// tears its own product down with `orphaned`; the waiter, at the deadline, COMPARE-EXCHANGES running -> abandoned and, if that fails, the
// helper has finished and the product is the waiter's.  Exactly one side ever touches the product (the round-5 handshake of two flags
// let both act when `init` returned at the deadline itself: the waiter installed a communicator the helper was about to abort).
// Returns true when `init` finished in time (rc / product handed over), false when the call was abandoned (the helper stays detached).
extern "C++" {
struct DeadlineCall {
    std::atomic<int> state{0};
    int rc = 0;
    void *product = nullptr;
};
template <class Init, class Orphaned>
static bool init_under_deadline(Init init, Orphaned orphaned, int timeout_ms, int &rc, void *&product, std::atomic<int> *helper_exits = nullptr) {
    auto call = std::make_shared<DeadlineCall>();
    const double t0 = now_ms();
    std::thread([call, init, orphaned, helper_exits]() {
        call->rc = init(&call->product);
        if (call->state.exchange(1) == 2 && call->rc == 0 && call->product) { // abandoned before this returned: built for nobody
            void *mine = call->product;
            call->product = nullptr;
            orphaned(mine);
        }
        if (helper_exits) helper_exits->fetch_add(1);
    }).detach();
    while (call->state.load(std::memory_order_acquire) != 1) {
        if (now_ms() - t0 > (double)timeout_ms) {
            int expected = 0;
            if (call->state.compare_exchange_strong(expected, 2)) return false; // the helper will find "abandoned" and clean up after itself
            break;                                                               // it finished in this very moment: the product is ours
        }
        usleep(200);
    }
    rc = call->rc;
    product = call->product;
    return true;
}
} // extern "C++"

// FK_COMM_TIMEOUT_MS is the default for contexts whose "comm_timeout_ms" option was never set (an explicit fk_set_option wins);
// anything that is not a non-negative integer is ignored rather than silently turned into the blocking path
static int32_t effective_comm_timeout_ms(const fk_ctx *c) {
    if (!c->comm_timeout_set) {
        if (const char *env = getenv("FK_COMM_TIMEOUT_MS")) {
            char *endp = nullptr;
            const long v = strtol(env, &endp, 10);
            if (endp != env && *endp == '\0' && v >= 0 && v <= 86400000L) return (int32_t)v;
        }
    }
    return c->comm_timeout_ms;
}

// The handshake above with a stand-in for ncclCommInitRank that sleeps `init_ms` and hands out a token: out[0] = 1 the caller received
// the product (in time), 0 abandoned; out[1] = how many products were torn down as orphans, counted after the helper has exited.  For
// every timing exactly one of the two happens (tests/test_abi_cpu.py sweeps init_ms across the deadline).
int fk_debug_deadline_handshake(int32_t init_ms, int32_t timeout_ms, int64_t *out) {
    if (!out || init_ms < 0 || timeout_ms < 1) return FK_ERR_ARG;
    auto orphans = std::make_shared<std::atomic<int>>(0);
    std::atomic<int> exits{0};
    int rc = 0;
    void *product = nullptr;
    static int token;
    const bool in_time = init_under_deadline(
        [init_ms](void **made) {
            usleep((useconds_t)init_ms * 1000u);
            *made = &token;
            return 0;
        },
        [orphans](void *) { orphans->fetch_add(1); }, timeout_ms, rc, product, &exits);
    while (!exits.load()) usleep(200); // (a test wants the helper's verdict; fk_comm_init never waits for an abandoned helper)
    out[0] = in_time && product == &token ? 1 : 0;
    out[1] = orphans->load();
    return FK_OK;
}

int fk_comm_init(fk_ctx *c, const fk_comm_id *id, int32_t rank, int32_t world_size) {
    if (!c) return FK_ERR_ARG;
    if (!id || world_size < 1 || rank < 0 || rank >= world_size) return fail(c, FK_ERR_ARG, "bad communicator id / rank / world size");
    Rccl &r = rccl();
    if (!r.lib) return fail(c, FK_ERR_COMM, "%s", r.why.c_str());
    HIPCHK(c, hipSetDevice(c->device));
    if (c->comm) {
        (void)r.CommDestroy(c->comm);
        c->comm = nullptr;
    }
    c->comm_timeout_ms = effective_comm_timeout_ms(c);
    c->comm_async = false;
    const bool dbg = getenv("FK_DEBUG_COMM") != nullptr;
    if (c->comm_timeout_ms > 0) {
        // ncclCommInitRank blocks until every rank has joined (measured on RCCL 2.27.7: so does ncclCommInitRankConfig with
        // blocking = 0 when it is called outside a group).  A rank that died between the rendezvous and this call must not park its
        // peers here until the job's time limit: the call runs on a helper thread and this thread waits for it under the deadline.
        // On expiry the helper stays parked in RCCL's bootstrap (a socket wait; it owns nothing of this context and is never
        // joined), the context has no communicator, and the caller gets FK_ERR_COMM — bench.py / farkle run then agree on gloo.
        // Should the peer join after all, the helper finds the call abandoned and aborts the communicator it just made itself
        // (ncclCommAbort: nobody else holds it), so a late join leaks nothing — init_under_deadline decides with ONE atomic who owns the
        // result.  A process that has seen this error should end (exit code != 0 is the caller's call): a thread may still sit inside librccl.
        const fk_comm_id id_copy = *id;
        const int device = c->device;
        const double t0 = now_ms();
        Rccl *rp = &r;
        int init_rc = 0;
        void *made = nullptr;
        const bool in_time = init_under_deadline(
            [id_copy, device, world_size, rank, rp](void **out) {
                (void)hipSetDevice(device);
                return rp->CommInitRank(out, world_size, id_copy, rank);
            },
            [rp](void *orphan) { (void)(rp->CommAbort ? rp->CommAbort(orphan) : rp->CommDestroy(orphan)); }, c->comm_timeout_ms, init_rc, made);
        if (!in_time) {
            if (dbg) fprintf(stderr, "[fk comm] ncclCommInitRank still waiting after %.0f ms: giving up\n", now_ms() - t0);
            return fail(c, FK_ERR_COMM, "ncclCommInitRank did not complete within %d ms (comm_timeout_ms): a peer rank never joined",
                        c->comm_timeout_ms);
        }
        struct { int rc; void *comm; } done{init_rc, made}, *pending = &done;
        if (dbg) fprintf(stderr, "[fk comm] ncclCommInitRank returned %d after %.1f ms\n", pending->rc, now_ms() - t0);
        if (pending->rc != 0) return rccl_fail(c, "ncclCommInitRank", pending->rc);
        if (!pending->comm) return fail(c, FK_ERR_COMM, "ncclCommInitRank returned no communicator");
        c->comm = pending->comm;
        c->comm_rank = rank;
        c->comm_world = world_size;
        c->comm_lost = false;
        return FK_OK;
    }
    const int rc = r.CommInitRank(&c->comm, world_size, *id, rank);
    if (rc != 0) {
        c->comm = nullptr;
        return rccl_fail(c, "ncclCommInitRank", rc);
    }
    c->comm_rank = rank;
    c->comm_world = world_size;
    c->comm_lost = false;
    return FK_OK;
}

int fk_reduce_tally(fk_ctx *c, int64_t *tally, int64_t n, int32_t root_rank) {
    if (!c) return FK_ERR_ARG;
    if (!tally || n < 0) return fail(c, FK_ERR_ARG, "tally is required");
    if (c->comm_lost) return fail(c, FK_ERR_COMM, "the communicator was aborted after a failed or timed-out collective: call fk_comm_init again");
    if (!c->comm) return fail(c, FK_ERR_COMM, "no communicator: call fk_comm_init first");
    if (root_rank < 0 || root_rank >= c->comm_world) return fail(c, FK_ERR_ARG, "root rank outside the communicator");
    if (n == 0) return FK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n * sizeof(int64_t);
    int rc = ensure(c, c->comm_buf, bytes);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->comm_buf.p, tally, bytes, hipMemcpyHostToDevice, c->stream));
    const double t0 = now_ms();
    const bool is_root = c->comm_rank == root_rank;
    const int nrc = rccl().Reduce(c->comm_buf.p, c->comm_buf.p, (size_t)n, 4 /* ncclInt64 */, 0 /* ncclSum */, root_rank, c->comm, c->stream);
    if ((rc = comm_settle(c, "ncclReduce", nrc, t0))) return rc;
    if (is_root) HIPCHK(c, hipMemcpyAsync(tally, c->comm_buf.p, bytes, hipMemcpyDeviceToHost, c->stream));
    return comm_wait_stream(c, "ncclReduce", t0);
}

// The resident accumulator summed over the communicator ON THE DEVICE (ncclReduce on the engine's stream) and copied to the
// host on the root rank only; single-rank contexts (no communicator) just copy it.  The accumulator is cleared afterwards.
int fk_tally_resident_reduce(fk_ctx *c, int64_t *out, int64_t n, int32_t root_rank) {
    if (!c) return FK_ERR_ARG;
    if (n < 0 || (size_t)n != c->acc_n || !c->acc.p) return fail(c, FK_ERR_ARG, "resident tally holds %lld elements, %lld asked for", (long long)c->acc_n, (long long)n);
    if (c->comm_lost) return fail(c, FK_ERR_COMM, "the communicator was aborted after a failed or timed-out collective: call fk_comm_init again");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n * sizeof(int64_t);
    bool root = true;
    if (c->comm && c->comm_world > 1) {
        if (root_rank < 0 || root_rank >= c->comm_world) return fail(c, FK_ERR_ARG, "root rank outside the communicator");
        const double t0 = now_ms();
        root = c->comm_rank == root_rank;
        const int nrc = rccl().Reduce(c->acc.p, c->acc.p, (size_t)n, 4 /* ncclInt64 */, 0 /* ncclSum */, root_rank, c->comm, c->stream);
        int rc = comm_settle(c, "ncclReduce", nrc, t0);
        if (!rc) rc = comm_wait_stream(c, "ncclReduce", t0);
        if (rc) return rc;
    }
    if (root) {
        if (!out) return fail(c, FK_ERR_ARG, "the root rank needs an output buffer");
        HIPCHK(c, hipMemcpyAsync(out, c->acc.p, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipMemsetAsync(c->acc.p, 0, bytes, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FK_OK;
}

// ranks of the communicator as RCCL itself counts them (ncclCommCount); 1 without a communicator
int fk_comm_ranks(fk_ctx *c) {
    if (!c) return FK_ERR_ARG;
    if (!c->comm) return 1;
    int n = 0;
    auto count = reinterpret_cast<int (*)(void *, int *)>(dlsym(rccl().lib, "ncclCommCount"));
    if (!count || count(c->comm, &n) != 0) return c->comm_world;
    return n;
}

int fk_comm_destroy(fk_ctx *c) {
    if (!c) return FK_ERR_ARG;
    if (c->comm) {
        HIPCHK(c, hipSetDevice(c->device));
        (void)rccl().CommDestroy(c->comm);
        c->comm = nullptr;
    }
    c->comm_world = 1;
    c->comm_rank = 0;
    c->comm_async = false;
    c->comm_lost = false;
    return FK_OK;
}

// ---- probes ----
int fk_debug_score(fk_ctx *c, int64_t n, const uint8_t *faces, const int32_t *len, const int32_t *pre,
                   const fk_strategy *strategy, int32_t *out) {
    if (!c || n < 0 || !faces || !len || !pre || !strategy || !out) return c ? fail(c, FK_ERR_ARG, "bad arguments") : FK_ERR_ARG;
    if (n == 0) return FK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    for (int64_t i = 0; i < n; ++i) {
        if (pre[i] < 0 || pre[i] % 50) return fail(c, FK_ERR_ARG, "turn_score_pre must be a non-negative multiple of 50 (every Farkle score is)");
        if (len[i] < 0 || len[i] > 6) return fail(c, FK_ERR_ARG, "roll cannot contain more than six dice");
        for (int32_t j = 0; j < len[i]; ++j)
            if (faces[i * 6 + j] < 1 || faces[i * 6 + j] > 6) return fail(c, FK_ERR_ARG, "dice faces must be between 1 and 6");
    }
    int rc = validate_strategies(c, strategy, (int32_t)std::min<int64_t>(n, 0x7fffffff));
    if (rc) return rc;
    std::vector<uint2> packed((size_t)n);
    for (int64_t i = 0; i < n; ++i) packed[(size_t)i] = pack_strategy(strategy[i]);
    const size_t sz[5] = {(size_t)n * 6, (size_t)n * 4, (size_t)n * 4, (size_t)n * 8, (size_t)n * 20};
    if ((rc = ensure_all(c, c->dbg.a, sz[0], c->dbg.b, sz[1], c->dbg.c, sz[2], c->dbg.d, sz[3], c->dbg.e, sz[4]))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->dbg.a.p, faces, sz[0], hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dbg.b.p, len, sz[1], hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dbg.c.p, pre, sz[2], hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dbg.d.p, packed.data(), sz[3], hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(fk_dbg_score_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, c->dbg.a.as<const uint8_t>(),
                       c->dbg.b.as<const int32_t>(), c->dbg.c.as<const int32_t>(), c->dbg.d.as<const uint2>(), c->score_lut.p, c->discard_lut.p,
                       c->dbg.e.as<int32_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->dbg.e.p, sz[4], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FK_OK;
}

int fk_debug_should_continue(fk_ctx *c, int64_t n, const int32_t *args, const fk_strategy *strategy, int32_t *out) {
    if (!c || n < 0 || !args || !strategy || !out) return c ? fail(c, FK_ERR_ARG, "bad arguments") : FK_ERR_ARG;
    if (n == 0) return FK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = validate_strategies(c, strategy, (int32_t)std::min<int64_t>(n, 0x7fffffff));
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (args[i * 6] < 0 || args[i * 6] % 50 || args[i * 6 + 5] < 0 || args[i * 6 + 5] % 50)
            return fail(c, FK_ERR_ARG, "turn_score and player_score must be non-negative multiples of 50 (every Farkle score is)");
    std::vector<uint2> packed((size_t)n);
    for (int64_t i = 0; i < n; ++i) packed[(size_t)i] = pack_strategy(strategy[i]);
    const size_t sz[3] = {(size_t)n * 24, (size_t)n * 8, (size_t)n * 4};
    if ((rc = ensure_all(c, c->dbg.a, sz[0], c->dbg.b, sz[1], c->dbg.c, sz[2]))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->dbg.a.p, args, sz[0], hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dbg.b.p, packed.data(), sz[1], hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(fk_dbg_continue_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, c->dbg.a.as<const int32_t>(),
                       c->dbg.b.as<const uint2>(), c->dbg.c.as<int32_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->dbg.c.p, sz[2], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FK_OK;
}

static int debug_dice_common(fk_ctx *c, int64_t n, const fk_coord *coords, const uint64_t *state, int32_t n_calls,
                             const int32_t *sizes, uint8_t *faces, uint64_t *raw64, uint64_t *state_out) {
    if (!c || n < 0 || n_calls < 0 || !sizes || !faces) return c ? fail(c, FK_ERR_ARG, "bad arguments") : FK_ERR_ARG;
    if (n == 0) return FK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int32_t total = 0;
    for (int32_t i = 0; i < n_calls; ++i) {
        if (sizes[i] < 1 || sizes[i] > 6) return fail(c, FK_ERR_ARG, "roll sizes must be in [1, 6]");
        total += sizes[i];
    }
    int rc;
    const uint4 *d_seeds = nullptr, *d_incs = nullptr;
    const uint64_t *d_state = nullptr;
    if (coords) {
        if ((rc = ensure_all(c, c->coords, (size_t)n, CSET(c).state, (size_t)n * 4, CSET(c).inc, (size_t)n))) return rc;
        // one 1-seat "game" per coordinate; the seed kernel offsets the seat stream by coords[i].seat_index
        HIPCHK(c, hipMemcpyAsync(c->coords.p, coords, sizeof(fk_coord) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        SeedArgs sa{};
        sa.coords = c->coords.p;
        sa.k = 1;
        sa.n_games = (uint32_t)n;
        sa.state = CSET(c).state.p;
        sa.state_dw = 4;
        sa.inc = CSET(c).inc.p;
        hipLaunchKernelGGL(fk_seed_kernel, dim3((unsigned)((n + SEED_BLOCK - 1) / SEED_BLOCK)), dim3(SEED_BLOCK), 0, c->stream, sa);
        HIPCHK(c, hipGetLastError());
        d_seeds = reinterpret_cast<const uint4 *>(CSET(c).state.p);
        d_incs = sa.inc;
    } else {
        if (!state) return fail(c, FK_ERR_ARG, "state is required");
        if ((rc = ensure(c, c->dbg.a, (size_t)n * 48))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->dbg.a.p, state, (size_t)n * 48, hipMemcpyHostToDevice, c->stream));
        d_state = c->dbg.a.as<const uint64_t>();
    }
    if ((rc = ensure_all(c, c->dbg.b, (size_t)n_calls * 4 + 4, c->dbg.c, (size_t)n * std::max(total, 1), c->dbg.d, (size_t)n * 32, c->dbg.e, (size_t)n * 48)))
        return rc;
    if (n_calls) HIPCHK(c, hipMemcpyAsync(c->dbg.b.p, sizes, (size_t)n_calls * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(fk_dbg_dice_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, n, d_seeds, d_incs, d_state, n_calls,
                       c->dbg.b.as<const int32_t>(), total, c->dbg.c.as<uint8_t>(), raw64 ? c->dbg.d.as<uint64_t>() : nullptr,
                       state_out ? c->dbg.e.as<uint64_t>() : nullptr);
    HIPCHK(c, hipGetLastError());
    if (total) HIPCHK(c, hipMemcpyAsync(faces, c->dbg.c.p, (size_t)n * total, hipMemcpyDeviceToHost, c->stream));
    if (raw64) HIPCHK(c, hipMemcpyAsync(raw64, c->dbg.d.p, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream));
    if (state_out) HIPCHK(c, hipMemcpyAsync(state_out, c->dbg.e.p, (size_t)n * 48, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FK_OK;
}

int fk_coordinate_seeds(fk_ctx *c, int64_t n, const fk_coord *coords, uint32_t *seed32, uint64_t *seed64) {
    if (!c || n < 0 || !coords || (!seed32 && !seed64)) return c ? fail(c, FK_ERR_ARG, "bad arguments") : FK_ERR_ARG;
    if (n == 0) return FK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_all(c, c->coords, (size_t)n, c->dbg.a, (size_t)n * 4, c->dbg.b, (size_t)n * 8);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->coords.p, coords, sizeof(fk_coord) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(fk_coordinate_seed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, c->coords.p,
                       seed32 ? c->dbg.a.as<uint32_t>() : nullptr, seed64 ? c->dbg.b.as<uint64_t>() : nullptr);
    HIPCHK(c, hipGetLastError());
    if (seed32) HIPCHK(c, hipMemcpyAsync(seed32, c->dbg.a.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (seed64) HIPCHK(c, hipMemcpyAsync(seed64, c->dbg.b.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FK_OK;
}

int fk_game_seeds(fk_ctx *c, uint32_t purpose, uint64_t root_seed, uint64_t k, uint64_t shuffle_begin, uint64_t n_shuffles,
                  uint32_t games_per_shuffle, uint32_t *seed32) {
    if (!c) return FK_ERR_ARG;
    if (!seed32 || games_per_shuffle == 0 || n_shuffles > 0xffffffffull || n_shuffles * games_per_shuffle > ((uint64_t)1 << 33))
        return fail(c, FK_ERR_ARG, "bad arguments");
    if (n_shuffles == 0) return FK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    c->letters.clear();
    c->mail_used = 0;
    const size_t n = (size_t)n_shuffles * games_per_shuffle;
    int rc = ensure(c, c->seeds, n * 4);
    if (rc) return rc;
    hipLaunchKernelGGL(fk_game_seed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, seed_prefix(purpose, root_seed, k),
                       shuffle_begin, (uint32_t)n_shuffles, games_per_shuffle, c->seeds.as<uint32_t>());
    HIPCHK(c, hipGetLastError());
    rc = post_d2h(c, seed32, c->seeds.p, n * 4);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    deliver_mail(c);
    return FK_OK;
}

int fk_debug_dice(fk_ctx *c, int64_t n, const fk_coord *coords, int32_t n_calls, const int32_t *sizes, uint8_t *faces,
                  uint64_t *raw64) {
    if (!coords) return c ? fail(c, FK_ERR_ARG, "coords is required") : FK_ERR_ARG;
    return debug_dice_common(c, n, coords, nullptr, n_calls, sizes, faces, raw64, nullptr);
}

int fk_debug_dice_state(fk_ctx *c, int64_t n, const uint64_t *state, int32_t n_calls, const int32_t *sizes, uint8_t *faces,
                        uint64_t *state_out) {
    return debug_dice_common(c, n, nullptr, state, n_calls, sizes, faces, nullptr, state_out);
}

int fk_debug_dice_keys(fk_ctx *c, int64_t n, const uint64_t *state, int32_t n_calls, const int32_t *sizes, uint32_t *keys,
                       uint64_t *state_out) {
    if (!c) return FK_ERR_ARG;
    if (n < 0 || n_calls < 1 || !state || !sizes || !keys || !state_out) return fail(c, FK_ERR_ARG, "bad arguments");
    for (int32_t i = 0; i < n_calls; ++i)
        if (sizes[i] < 1 || sizes[i] > 6) return fail(c, FK_ERR_ARG, "roll sizes must be in 1..6");
    if (n == 0) return FK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_all(c, c->dbg.a, (size_t)n * 48, c->dbg.b, (size_t)n_calls * 4, c->dbg.c, (size_t)n * n_calls * 4, c->dbg.e, (size_t)n * 48))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->dbg.a.p, state, (size_t)n * 48, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dbg.b.p, sizes, (size_t)n_calls * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(fk_dbg_dice_key_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, n, c->dbg.a.as<const uint64_t>(), n_calls,
                       c->dbg.b.as<const int32_t>(), c->dbg.c.as<uint32_t>(), c->dbg.e.as<uint64_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(keys, c->dbg.c.p, (size_t)n * n_calls * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(state_out, c->dbg.e.p, (size_t)n * 48, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FK_OK;
}

int fk_debug_bounded_draws(fk_ctx *c, int64_t n, const fk_coord *coords, uint64_t bound, int32_t n_draws, uint32_t *out) {
    if (!c) return FK_ERR_ARG;
    if (n < 0 || n_draws < 0 || !coords || !out) return fail(c, FK_ERR_ARG, "bad arguments");
    if (bound < 1 || bound > 0xffffffffull) return fail(c, FK_ERR_ARG, "bound must be in [1, 2^32 - 1]");
    if (n == 0 || n_draws == 0) return FK_OK;
    if ((uint64_t)n * (uint64_t)n_draws > ((uint64_t)1 << 31)) return fail(c, FK_ERR_ARG, "more than 2^31 draws in one probe");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->coords, (size_t)n))) return rc;
    if ((rc = ensure(c, c->dbg.c, (size_t)n * n_draws * 4))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->coords.p, coords, sizeof(fk_coord) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(fkb::fk_boot_draws_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, n,
                       c->coords.p, (uint32_t)bound, (uint32_t)n_draws, c->dbg.c.as<uint32_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->dbg.c.p, (size_t)n * n_draws * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FK_OK;
}

int fk_debug_perm_from_draws(fk_ctx *c, int32_t S, int64_t n_sh, const uint16_t *draws, int32_t path, int32_t *perms) {
    if (!c) return FK_ERR_ARG;
    if (S < 1 || S > 65535) return fail(c, FK_ERR_ARG, "S=%d: a table has 1 to 65535 strategies", S);
    if (n_sh < 1 || (uint64_t)n_sh * (uint64_t)S > ((uint64_t)1 << 28)) return fail(c, FK_ERR_ARG, "1 shuffle at least, 2^28 entries at most in one probe");
    if (path != 1 && path != 2) return fail(c, FK_ERR_ARG, "path %d: 1 = the swap chains, 2 = the chain-free kernel", (int)path);
    if (path == 2 && !perm_parallel_fits(S)) return fail(c, FK_ERR_ARG, "S=%d is beyond the chain-free kernel's LDS reach", S);
    if (!perms || (S > 1 && !draws)) return fail(c, FK_ERR_ARG, "draws and perms are required");
    const uint32_t N = (uint32_t)S - 1u, full = N & ~7u, tail = N & 7u, n = (uint32_t)n_sh;
    // the kernels index LDS with the draws: one beyond its step's bound never reaches the device
    for (uint32_t sh = 0; sh < n; ++sh)
        for (uint32_t p = 0; p < N; ++p)
            if (draws[(size_t)sh * N + p] > N - p)
                return fail(c, FK_ERR_ARG, "shuffle %u, draw %u: %u is beyond its step's bound %u", sh, p, (unsigned)draws[(size_t)sh * N + p], N - p);
    HIPCHK(c, hipSetDevice(c->device));
    const DrawLayout dl = draw_layout(path, (uint32_t)S, n);
    std::vector<uint16_t> packed(dl.bytes / 2, (uint16_t)0);
    for (uint32_t sh = 0; sh < n; ++sh) {
        uint16_t *const row = packed.data() + (size_t)sh * dl.sh_stride * 8u;
        const size_t group_u16 = (size_t)dl.g_stride * 8u;
        for (uint32_t p = 0; p < N; ++p) {
            const uint16_t j = draws[(size_t)sh * N + p];
            if (p < full) row[(size_t)(p >> 3) * group_u16 + (p & 7u)] = j;
            if (tail && p + 8u >= N) row[(size_t)(full >> 3) * group_u16 + (p + 8u - N)] = j; // the right-aligned last group
        }
    }
    int rc = configure_perm_kernels(c);
    if (rc) return rc;
    // the chunk set no prepared (hinted) tournament chunk sits in; whatever it held is void afterwards
    ChunkSet &cs = c->sets[c->sets[c->cur].prepared ? c->cur ^ 1 : c->cur];
    cs.prepared = false;
    HIPCHK(c, hipStreamWaitEvent(c->stream, cs.ready, 0)); // an unused side-stream preparation may still own the set
    const uint32_t slots = perm_slots(S), perm_blocks = (n + slots - 1u) / slots;
    if ((rc = ensure(c, cs.perm, (size_t)perm_blocks * S * slots))) return rc;
    if ((rc = ensure(c, cs.draws, dl.bytes))) return rc;
    if (dl.bytes) HIPCHK(c, hipMemcpyAsync(cs.draws.p, packed.data(), packed.size() * 2, hipMemcpyHostToDevice, c->stream));
    launch_perm_consumers(cs, c->stream, path, dl, n, (uint32_t)S, slots);
    HIPCHK(c, hipGetLastError());
    std::vector<uint16_t> perm_host((size_t)perm_blocks * S * slots);
    HIPCHK(c, hipMemcpyAsync(perm_host.data(), cs.perm.p, perm_host.size() * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t s = 0; s < n; ++s)
        for (int32_t i = 0; i < S; ++i)
            perms[(size_t)s * S + i] = perm_host[((size_t)(s / slots) * S + i) * slots + s % slots];
    return FK_OK;
}

// ---- what both bootstrap entries state once (their device code is shared too: fk_bootstrap.h) ----
// One cell of the stacked matrices (a player count of a root, named `who` in the messages): checks it and appends its descriptor.
static int boot_add_cell(fk_ctx *c, std::vector<fkb::KDesc> &kd, uint64_t &sum_B, uint64_t root, int32_t k, int64_t n_batches, const int64_t *wins,
                         const int64_t *exposures, int32_t S, const char *who) {
    if (n_batches < 1 || n_batches > 0xffffffffll || !wins || !exposures)
        return fail(c, FK_ERR_ARG, "%s needs 1 to 2^32 - 1 eligible batches and both matrices", who);
    kd.push_back({root, (uint64_t)k, (uint32_t)n_batches, (uint32_t)sum_B, 1.0 / (double)k});
    sum_B += (uint64_t)n_batches;
    if (sum_B > ((uint64_t)1 << 31)) return fail(c, FK_ERR_ARG, "more than 2^31 batches");
    if (!boot_totals_exact(wins, exposures, (uint64_t)n_batches, (size_t)S))
        return fail(c, FK_ERR_ARG, "%s: a negative count, or one whose resampled total can pass 2^63", who);
    return FK_OK;
}

// both stacked matrices and the descriptors, resident for the call
static int boot_upload(fk_ctx *c, const std::vector<fkb::KDesc> &kd, const int64_t *const *wins, const int64_t *const *exposures, uint64_t sum_B, int32_t S) {
    BootBufs &b = c->boot;
    const size_t cells = (size_t)sum_B * (size_t)S;
    if (const int rc = ensure_all(c, b.wins, cells, b.exposures, cells, b.kd, kd.size())) return rc;
    for (int which = 0; which < 2; ++which)
        for (size_t i = 0; i < kd.size(); ++i)
            HIPCHK(c, hipMemcpyAsync((which ? b.exposures : b.wins).p + (size_t)kd[i].row0 * (size_t)S, (which ? exposures : wins)[i],
                                     (size_t)kd[i].B * (size_t)S * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.kd.p, kd.data(), kd.size() * sizeof(fkb::KDesc), hipMemcpyHostToDevice, c->stream));
    return FK_OK;
}

// replicates of one device block: what half the workspace budget holds at `per_rep` bytes each (4096 at most; option "bootstrap_block" caps it),
// in whole groups of `group`, no more than the range needs
static int64_t boot_block(fk_ctx *c, size_t per_rep, int64_t group, int64_t n_rep) {
    int64_t block = std::max<int64_t>((int64_t)(workspace_budget(c) / 2 / (int64_t)per_rep), 1);
    block = std::min<int64_t>(block, 4096);
    if (c->bootstrap_block > 0) block = std::min(block, c->bootstrap_block);
    return std::min<int64_t>(std::max<int64_t>(block / group * group, group), (n_rep + group - 1) / group * group);
}

// one block: its multiplicity rows zeroed, then the draws of `nr` replicates from replicate `rep0`
static int boot_counts(fk_ctx *c, uint32_t purpose, uint64_t rep0, uint32_t nr, uint32_t nr_pad, uint32_t n_cells, uint32_t sum_B) {
    HIPCHK(c, hipMemsetAsync(c->boot.counts.p, 0, (size_t)nr_pad * sum_B * 4, c->stream));
    hipLaunchKernelGGL(fkb::fk_boot_counts_kernel, dim3((nr * n_cells + 63) / 64), dim3(64), 0, c->stream, purpose, rep0, nr, n_cells,
                       c->boot.kd.p, sum_B, c->boot.counts.p);
    return FK_OK;
}

// the flag the rate kernels raise on a replicate without complete-support exposure; waits for the stream
static int boot_read_bad(fk_ctx *c, int32_t &bad) {
    HIPCHK(c, hipMemcpyAsync(&bad, c->boot.bad.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FK_OK;
}

int fk_performance_bootstrap(fk_ctx *c, uint64_t root_seed, int32_t n_k, const int32_t *ks, const int64_t *batch_counts,
                             const int64_t *const *wins, const int64_t *const *exposures, int32_t S, int64_t replicate_begin,
                             int64_t replicate_end, int32_t top_n, double delta, int32_t n_controls, const int32_t *controls,
                             double *scores, int64_t *rank_sum, int64_t *rank_square_sum, int64_t *top_counts, int64_t *shortlist_counts,
                             double *contrast_sum, double *contrast_square_sum) {
    if (!c) return FK_ERR_ARG;
    if (n_k < 1 || n_k > 64 || !ks || !batch_counts || !wins || !exposures) return fail(c, FK_ERR_ARG, "1 to 64 player counts with their matrices are required");
    if (S < 1 || S > (1 << 24)) return fail(c, FK_ERR_ARG, "S must be in [1, 2^24]");
    if (replicate_begin < 0 || replicate_end < replicate_begin) return fail(c, FK_ERR_ARG, "bad replicate range");
    if (top_n < 0 || top_n > S) return fail(c, FK_ERR_ARG, "top_n must be in [0, S]");
    if (!(delta == delta)) return fail(c, FK_ERR_ARG, "delta is NaN");
    if (!rank_sum || !rank_square_sum || !top_counts || !shortlist_counts) return fail(c, FK_ERR_ARG, "the four counter outputs are required");
    if (n_controls < 0 || (n_controls > 0 && (!controls || !contrast_sum || !contrast_square_sum)))
        return fail(c, FK_ERR_ARG, "controls need their index list and both accumulators");
    for (int32_t i = 0; i < n_controls; ++i)
        if (controls[i] < 0 || controls[i] >= S) return fail(c, FK_ERR_ARG, "control %d: column %d outside [0, S)", i, controls[i]);
    std::vector<fkb::KDesc> kd;
    uint64_t sum_B = 0;
    int rc;
    for (int32_t i = 0; i < n_k; ++i) {
        if (ks[i] < 1) return fail(c, FK_ERR_ARG, "player count %d: k = %d", i, ks[i]);
        char who[48];
        snprintf(who, sizeof(who), "player count %d", ks[i]);
        if ((rc = boot_add_cell(c, kd, sum_B, root_seed, ks[i], batch_counts[i], wins[i], exposures[i], S, who))) return rc;
    }
    const int64_t n_rep = replicate_end - replicate_begin;
    HIPCHK(c, hipSetDevice(c->device));
    // resident for the call: both stacked matrices, the descriptors, the counters and the contrast accumulators
    BootBufs &b = c->boot;
    const size_t n_contrast = (size_t)n_controls * S, contrast_bytes = n_contrast * 8; // of the sums; the squares lie behind them
    if ((rc = boot_upload(c, kd, wins, exposures, sum_B, S))) return rc;
    if ((rc = ensure_all(c, b.counters, (size_t)4 * S, b.contrast, 2 * n_contrast, b.controls, (size_t)n_controls, b.bad, 1))) return rc;
    HIPCHK(c, hipMemsetAsync(b.counters.p, 0, (size_t)4 * S * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(b.bad.p, 0, 4, c->stream));
    if (n_controls) {
        HIPCHK(c, hipMemcpyAsync(b.contrast.p, contrast_sum, contrast_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.contrast.p + n_contrast, contrast_square_sum, contrast_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.controls.p, controls, (size_t)n_controls * 4, hipMemcpyHostToDevice, c->stream));
    }
    // the replicate range in blocks sized from the workspace budget: per replicate one multiplicity row and one score row
    const int64_t block = boot_block(c, (size_t)sum_B * 4 + (size_t)S * 8, fkb::RB, n_rep);
    if (n_rep > 0 && (rc = ensure_all(c, b.counts, (size_t)block * sum_B, b.scores, (size_t)block * S))) return rc;
    const unsigned s_tiles = (unsigned)((S + fkb::TS - 1) / fkb::TS);
    for (int64_t b0 = 0; b0 < n_rep; b0 += block) {
        const uint32_t nr = (uint32_t)std::min<int64_t>(block, n_rep - b0), nr_pad = (nr + fkb::RB - 1) / fkb::RB * fkb::RB;
        if ((rc = boot_counts(c, fkb::PURPOSE_BOOTSTRAP, (uint64_t)(replicate_begin + b0), nr, nr_pad, (uint32_t)n_k, (uint32_t)sum_B))) return rc;
        hipLaunchKernelGGL(fkb::fk_boot_score_kernel, dim3(s_tiles, nr_pad / fkb::RB), dim3(fkb::TS), 0, c->stream,
                           b.wins.p, b.exposures.p, b.counts.p, b.kd.p, (uint32_t)n_k, (uint32_t)sum_B, (uint32_t)S, nr, b.scores.p, b.bad.p);
        hipLaunchKernelGGL(fkb::fk_boot_rank_kernel, dim3(s_tiles, (nr + fkb::RC - 1) / fkb::RC), dim3(fkb::TS), 0, c->stream, b.scores.p,
                           (uint32_t)S, nr, (uint32_t)top_n, delta, b.counters.p);
        if (n_controls)
            hipLaunchKernelGGL(fkb::fk_boot_contrast_kernel, dim3((unsigned)((n_contrast + 255) / 256)), dim3(256), 0, c->stream, b.scores.p,
                               (uint32_t)S, nr, b.controls.p, (uint32_t)n_controls, b.contrast.p);
        HIPCHK(c, hipGetLastError());
        if (scores) HIPCHK(c, hipMemcpyAsync(scores + (size_t)b0 * S, b.scores.p, (size_t)nr * S * 8, hipMemcpyDeviceToHost, c->stream));
    }
    int32_t bad = 0;
    if ((rc = boot_read_bad(c, bad))) return rc;
    if (bad) return fail(c, FK_ERR_ARG, "joint batch resampling produced zero complete-support exposure");
    int64_t *outs[4] = {rank_sum, rank_square_sum, top_counts, shortlist_counts};
    for (int i = 0; i < 4; ++i)
        HIPCHK(c, hipMemcpyAsync(outs[i], b.counters.p + (size_t)i * S, (size_t)S * 8, hipMemcpyDeviceToHost, c->stream));
    if (n_controls) {
        HIPCHK(c, hipMemcpyAsync(contrast_sum, b.contrast.p, contrast_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(contrast_square_sum, b.contrast.p + n_contrast, contrast_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FK_OK;
}

int fk_root_stability_bootstrap(fk_ctx *c, const uint64_t *roots, int32_t n_k, const int32_t *ks, const int64_t *batch_counts,
                                const int64_t *const *wins, const int64_t *const *exposures, int32_t S, const double *weights,
                                int64_t replicate_begin, int64_t replicate_end, int32_t top_n, const double *observed,
                                const double *expected, const double *observed_across, const double *expected_across,
                                int64_t *top_counts, double *maxima, uint8_t *membership) {
    if (!c) return FK_ERR_ARG;
    if (!roots || roots[0] >= roots[1]) return fail(c, FK_ERR_ARG, "two roots (a, b) with a < b are required");
    if (n_k < 1 || n_k > 64 || !ks || !batch_counts || !wins || !exposures || !weights)
        return fail(c, FK_ERR_ARG, "1 to 64 player counts with their weights and the matrices of both roots are required");
    if (S < 1 || S > (1 << 24)) return fail(c, FK_ERR_ARG, "S must be in [1, 2^24]");
    if (replicate_begin < 0 || replicate_end < replicate_begin) return fail(c, FK_ERR_ARG, "bad replicate range");
    if (top_n < 0 || top_n > S) return fail(c, FK_ERR_ARG, "top_n must be in [0, S]");
    if (!top_counts) return fail(c, FK_ERR_ARG, "top_counts is required");
    const int given = (observed ? 1 : 0) + (expected ? 1 : 0) + (observed_across ? 1 : 0) + (expected_across ? 1 : 0);
    if (given != 0 && given != 4) return fail(c, FK_ERR_ARG, "observed / expected by k and across k come as a group of four");
    const bool joint = given == 4;
    if (joint && !maxima) return fail(c, FK_ERR_ARG, "the joint family needs the maxima output");
    for (int32_t i = 0; i < n_k; ++i) {
        if (ks[i] < 1) return fail(c, FK_ERR_ARG, "player count %d: k = %d", i, ks[i]);
        if (!std::isfinite(weights[i])) return fail(c, FK_ERR_ARG, "player count %d: its weight is not finite", ks[i]);
    }
    if (joint) { // expected may be NaN or <= 0 (the column is no estimand); a non-finite observed would poison a maximum
        for (size_t j = 0; j < (size_t)n_k * (size_t)S; ++j)
            if (!std::isfinite(observed[j])) return fail(c, FK_ERR_ARG, "player count %d: observed is not finite", ks[j / (size_t)S]);
        for (size_t j = 0; j < (size_t)S; ++j)
            if (!std::isfinite(observed_across[j])) return fail(c, FK_ERR_ARG, "across k: observed is not finite");
    }
    const int32_t n_cells = 2 * n_k;
    std::vector<fkb::KDesc> kd;
    uint64_t sum_B = 0;
    int rc;
    for (int32_t i = 0; i < n_cells; ++i) {
        char who[64];
        snprintf(who, sizeof(who), "root %llu, player count %d", (unsigned long long)roots[i / n_k], ks[i % n_k]);
        if ((rc = boot_add_cell(c, kd, sum_B, roots[i / n_k], ks[i % n_k], batch_counts[i], wins[i], exposures[i], S, who))) return rc;
    }
    const int64_t n_rep = replicate_end - replicate_begin;
    HIPCHK(c, hipSetDevice(c->device));
    // resident for the call: both stacked matrices, the descriptors, the parameter block, the counters of both roots
    BootBufs &b = c->boot;
    const fkl::RootParams par((size_t)n_k, (size_t)S, joint);
    const size_t by_k = (size_t)n_k * (size_t)S, n_counters = (size_t)2 * 4 * S; // the rank kernel's four counters per root
    if ((rc = boot_upload(c, kd, wins, exposures, sum_B, S))) return rc;
    if ((rc = ensure_all(c, b.bad, 1, b.params, par.n, b.root_counters, n_counters))) return rc;
    double *d_weights = b.params.p + par.weights, *d_observed = b.params.p + par.observed, *d_expected = b.params.p + par.expected;
    double *d_observed_across = b.params.p + par.observed_across, *d_expected_across = b.params.p + par.expected_across;
    HIPCHK(c, hipMemcpyAsync(d_weights, weights, (size_t)n_k * 8, hipMemcpyHostToDevice, c->stream));
    if (joint) {
        HIPCHK(c, hipMemcpyAsync(d_observed, observed, by_k * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_expected, expected, by_k * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_observed_across, observed_across, (size_t)S * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_expected_across, expected_across, (size_t)S * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemsetAsync(b.root_counters.p, 0, n_counters * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(b.bad.p, 0, 4, c->stream));
    // the replicate range in blocks sized from the workspace budget: per replicate one multiplicity row, one score row per root, one
    // maximum and (when asked for) one membership row per root.  Counts are integers and maxima per replicate: no carried state.
    const int64_t block = boot_block(c, (size_t)sum_B * 4 + (size_t)2 * S * 8 + 8 + (membership ? (size_t)2 * S : 0), fkr::RRB, n_rep);
    if (n_rep > 0) {
        if ((rc = ensure_all(c, b.counts, (size_t)block * sum_B, b.scores, (size_t)block * 2 * S, b.maxima, (size_t)block))) return rc;
        if (membership && (rc = ensure(c, b.member, (size_t)block * 2 * S))) return rc;
    }
    const fkb::KDesc *d_kd = b.kd.p;
    const int64_t *d_W = b.wins.p, *d_E = b.exposures.p;
    uint32_t *d_counts = b.counts.p;
    double *d_scores = b.scores.p;
    ull *d_maxima = b.maxima.p, *d_counters = b.root_counters.p;
    uint8_t *d_member = b.member.p;
    int32_t *d_bad = b.bad.p;
    const unsigned s_tiles = (unsigned)((S + fkb::TS - 1) / fkb::TS);
    for (int64_t b0 = 0; b0 < n_rep; b0 += block) {
        const uint32_t nr = (uint32_t)std::min<int64_t>(block, n_rep - b0), nr_pad = (nr + fkr::RRB - 1) / fkr::RRB * fkr::RRB;
        if ((rc = boot_counts(c, fkb::PURPOSE_ROOT_STABILITY_BOOTSTRAP, (uint64_t)(replicate_begin + b0), nr, nr_pad, (uint32_t)n_cells, (uint32_t)sum_B)))
            return rc;
        const dim3 rates_grid(s_tiles, nr_pad / fkr::RRB);
        if (joint) {
            HIPCHK(c, hipMemsetAsync(d_maxima, 0, (size_t)nr_pad * 8, c->stream));
            hipLaunchKernelGGL(fkr::fk_root_rates_kernel<true>, rates_grid, dim3(fkb::TS), 0, c->stream, d_W, d_E, d_counts, d_kd, (uint32_t)n_k,
                               (uint32_t)sum_B, (uint32_t)S, nr, d_weights, d_observed, d_expected, d_observed_across, d_expected_across,
                               d_scores, d_maxima, d_bad);
        } else {
            hipLaunchKernelGGL(fkr::fk_root_rates_kernel<false>, rates_grid, dim3(fkb::TS), 0, c->stream, d_W, d_E, d_counts, d_kd, (uint32_t)n_k,
                               (uint32_t)sum_B, (uint32_t)S, nr, d_weights, nullptr, nullptr, nullptr, nullptr, d_scores, nullptr, d_bad);
        }
        for (int root = 0; root < 2; ++root) // the rank kernel's top-n counter (third of four) is this root's inclusion count
            hipLaunchKernelGGL(fkb::fk_boot_rank_kernel, dim3(s_tiles, (nr + fkb::RC - 1) / fkb::RC), dim3(fkb::TS), 0, c->stream,
                               d_scores + (size_t)root * nr * S, (uint32_t)S, nr, (uint32_t)top_n, 0.0, d_counters + (size_t)root * 4 * S);
        if (membership)
            hipLaunchKernelGGL(fkr::fk_root_member_kernel, dim3(s_tiles, 2 * nr), dim3(fkb::TS), 0, c->stream, d_scores, (uint32_t)S, nr,
                               (uint32_t)top_n, d_member);
        HIPCHK(c, hipGetLastError());
        if (joint) HIPCHK(c, hipMemcpyAsync(maxima + b0, d_maxima, (size_t)nr * 8, hipMemcpyDeviceToHost, c->stream));
        if (membership) HIPCHK(c, hipMemcpyAsync(membership + (size_t)b0 * 2 * S, d_member, (size_t)nr * 2 * S, hipMemcpyDeviceToHost, c->stream));
    }
    int32_t bad = 0;
    if ((rc = boot_read_bad(c, bad))) return rc;
    if (bad) return fail(c, FK_ERR_ARG, "root bootstrap produced zero complete-support exposure");
    for (int root = 0; root < 2; ++root)
        HIPCHK(c, hipMemcpyAsync(top_counts + (size_t)root * S, d_counters + ((size_t)root * 4 + 2) * S, (size_t)S * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!joint && maxima)
        for (int64_t r = 0; r < n_rep; ++r) maxima[r] = 0.0;
    return FK_OK;
}

// workgroups of a performance kernel over `blocks` blocks of work: option "performance_grid" caps them, the kernels stride
static unsigned perf_grid(fk_ctx *c, uint64_t blocks) {
    uint64_t grid = std::min<uint64_t>(std::max<uint64_t>(blocks, 1), fkp::MAX_GRID);
    if (c->performance_grid > 0) grid = std::min<uint64_t>(grid, (uint64_t)c->performance_grid);
    return (unsigned)grid;
}

int fk_performance_by_k(fk_ctx *c, int32_t k, int64_t B, int32_t S, const int64_t *wins, const int64_t *exposures, const int64_t *completed,
                        const int64_t *safety, int64_t *total_wins, int64_t *total_exposures, int64_t *total_completed, int64_t *total_safety,
                        int64_t *total_losses, int64_t *positive_batches, double *rate_sum, double *ssd) {
    if (!c) return FK_ERR_ARG;
    if (k < 1) return fail(c, FK_ERR_ARG, "player count k = %d", k);
    if (B < 1 || B > 0x7fffffffll) return fail(c, FK_ERR_ARG, "%dp: B = %lld: a batch matrix has 1 to 2^31 - 1 batches", k, (long long)B);
    if (S < 1 || S > (1 << 24)) return fail(c, FK_ERR_ARG, "%dp: S must be in [1, 2^24]", k);
    if (!wins || !exposures || !completed || !safety) return fail(c, FK_ERR_ARG, "%dp: the four count matrices are required", k);
    if (!total_wins || !total_exposures || !total_completed || !total_safety || !total_losses || !positive_batches || !rate_sum || !ssd)
        return fail(c, FK_ERR_ARG, "%dp: the eight outputs are required", k);
    // the reference's matrix checks (_validate_matrix_array :134-160) and its support check (:486-488), before anything is uploaded
    const size_t cells = (size_t)B * (size_t)S;
    std::vector<uint64_t> support((size_t)S, 0);
    const uint64_t limit = (uint64_t)1 << 62;
    for (size_t b = 0, at = 0; b < (size_t)B; ++b)
        for (size_t s = 0; s < (size_t)S; ++s, ++at) {
            const int64_t w = wins[at], e = exposures[at], done = completed[at], f = safety[at];
            if (w < 0 || e < 0 || done < 0 || f < 0) return fail(c, FK_ERR_ARG, "%dp: a negative count in batch row %zu, column %zu", k, b, s);
            if (w > done) return fail(c, FK_ERR_ARG, "%dp: wins > completed in batch row %zu, column %zu: impossible win/exposure counts", k, b, s);
            if ((uint64_t)done + (uint64_t)f != (uint64_t)e)
                return fail(c, FK_ERR_ARG, "%dp: exposures != completed + safety in batch row %zu, column %zu: attempted exposure conservation", k, b, s);
            if ((uint64_t)e > limit - support[s]) return fail(c, FK_ERR_ARG, "%dp: the exposure total of column %zu passes 2^62", k, s);
            support[s] += (uint64_t)e;
        }
    for (size_t s = 0; s < (size_t)S; ++s)
        if (support[s] == 0) return fail(c, FK_ERR_ARG, "%dp: strategies have no positive exposure support: column %zu", k, s);
    HIPCHK(c, hipSetDevice(c->device));
    PerformanceBufs &p = c->pf;
    if (const int rc = ensure_all(c, p.wins, cells, p.exposures, cells, p.completed, cells, p.safety, cells, p.totals, (size_t)6 * S, p.sums, (size_t)2 * S))
        return rc;
    const int64_t *host[4] = {wins, exposures, completed, safety};
    int64_t *dev[4] = {p.wins.p, p.exposures.p, p.completed.p, p.safety.p};
    for (int i = 0; i < 4; ++i) HIPCHK(c, hipMemcpyAsync(dev[i], host[i], cells * 8, hipMemcpyHostToDevice, c->stream));
    const unsigned grid = perf_grid(c, ((uint64_t)S + fkp::COLUMN_BLOCK - 1) / fkp::COLUMN_BLOCK);
    hipLaunchKernelGGL(fkp::fk_perf_by_k_kernel, dim3(grid), dim3(fkp::COLUMN_BLOCK), 0, c->stream, p.wins.p, p.exposures.p, p.completed.p,
                       p.safety.p, (uint32_t)B, (uint32_t)S, p.totals.p, p.sums.p);
    HIPCHK(c, hipGetLastError());
    // into the caller's arrays only once the stream has come through: a failed call leaves them as they were
    std::vector<long long> totals((size_t)6 * S);
    std::vector<double> sums((size_t)2 * S);
    HIPCHK(c, hipMemcpyAsync(totals.data(), p.totals.p, totals.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sums.data(), p.sums.p, sums.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t *outs[6] = {total_wins, total_exposures, total_completed, total_safety, total_losses, positive_batches};
    for (int i = 0; i < 6; ++i) std::copy(totals.begin() + (size_t)i * S, totals.begin() + (size_t)(i + 1) * S, outs[i]);
    std::copy(sums.begin(), sums.begin() + S, rate_sum);
    std::copy(sums.begin() + S, sums.end(), ssd);
    return FK_OK;
}

int fk_performance_across_k(fk_ctx *c, int32_t n, int32_t d, const double *deltas, const double *variances, double *delta_sum,
                            double *variance_sum, double *minimum, int32_t *worst_index, uint8_t *pareto_member, int32_t *leader_row) {
    if (!c) return FK_ERR_ARG;
    if (n < 1 || n > (1 << 24)) return fail(c, FK_ERR_ARG, "n = %d: 1 to 2^24 complete-support strategies", n);
    if (d < 1 || d > (int32_t)fkp::MAX_D) return fail(c, FK_ERR_ARG, "d = %d: 1 to %u required player counts", d, fkp::MAX_D);
    if (!deltas || !variances) return fail(c, FK_ERR_ARG, "deltas and variances are required");
    if (!delta_sum || !variance_sum || !minimum || !worst_index || !pareto_member || !leader_row) return fail(c, FK_ERR_ARG, "the six outputs are required");
    const size_t cells = (size_t)n * (size_t)d;
    for (size_t i = 0; i < cells; ++i) {
        if (!std::isfinite(deltas[i])) return fail(c, FK_ERR_ARG, "row %zu, player count %zu: the chance delta is not finite", i / (size_t)d, i % (size_t)d);
        if (variances[i] < 0.0 || std::isinf(variances[i])) // (NaN: a column with fewer than two positive batches has no mcse)
            return fail(c, FK_ERR_ARG, "row %zu, player count %zu: the variance is negative or infinite", i / (size_t)d, i % (size_t)d);
    }
    HIPCHK(c, hipSetDevice(c->device));
    PerformanceBufs &p = c->pf;
    if (const int rc = ensure_all(c, p.deltas, cells, p.variances, cells, p.stats, (size_t)3 * n, p.worst, (size_t)n, p.member, (size_t)n, p.best, 2))
        return rc;
    const ull start[2] = {0ull, (ull)(uint32_t)n}; // the key of no value; no leader yet
    HIPCHK(c, hipMemcpyAsync(p.best.p, start, 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.deltas.p, deltas, cells * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.variances.p, variances, cells * 8, hipMemcpyHostToDevice, c->stream));
    const unsigned row_grid = perf_grid(c, ((uint64_t)n + 63) / 64), pareto_grid = perf_grid(c, ((uint64_t)n + fkp::PARETO_BLOCK - 1) / fkp::PARETO_BLOCK);
    uint32_t *leader = reinterpret_cast<uint32_t *>(p.best.p + 1);
    hipLaunchKernelGGL(fkp::fk_perf_rows_kernel, dim3(row_grid), dim3(64), 0, c->stream, p.deltas.p, p.variances.p, (uint32_t)n, (uint32_t)d,
                       p.stats.p, p.worst.p, p.best.p);
    hipLaunchKernelGGL(fkp::fk_perf_pareto_kernel, dim3(pareto_grid), dim3(fkp::PARETO_BLOCK), 0, c->stream, p.deltas.p, (uint32_t)n, (uint32_t)d,
                       p.member.p);
    hipLaunchKernelGGL(fkp::fk_perf_leader_kernel, dim3(row_grid), dim3(64), 0, c->stream, p.stats.p + 2 * (size_t)n, (uint32_t)n, p.best.p, leader);
    HIPCHK(c, hipGetLastError());
    std::vector<double> stats((size_t)3 * n);
    std::vector<int32_t> worst((size_t)n);
    std::vector<uint8_t> member((size_t)n);
    ull best[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(stats.data(), p.stats.p, stats.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(worst.data(), p.worst.p, worst.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(member.data(), p.member.p, member.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(best, p.best.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t leader_found = (uint32_t)best[1];
    if (leader_found >= (uint32_t)n) return fail(c, FK_ERR_HIP, "the maximin reduction found no leader among %d rows", n);
    std::copy(stats.begin(), stats.begin() + n, delta_sum);
    std::copy(stats.begin() + n, stats.begin() + 2 * (size_t)n, variance_sum);
    std::copy(stats.begin() + 2 * (size_t)n, stats.end(), minimum);
    std::copy(worst.begin(), worst.end(), worst_index);
    std::copy(member.begin(), member.end(), pareto_member);
    *leader_row = (int32_t)leader_found;
    return FK_OK;
}

static_assert(fkl::RootWindowOut::N_TOTALS == fkw::N_TOTALS && fkl::RootWindowOut::N_SUMS == fkw::N_SUMS, "fk_layouts.h and fk_root_windows.h agree");

// workgroups of a window kernel over `tasks` wave tasks: option "root_windows_grid" caps them, the kernels stride
static unsigned root_windows_grid(fk_ctx *c, uint64_t tasks) {
    uint64_t grid = std::min<uint64_t>(std::max<uint64_t>(tasks, 1), fkw::MAX_GRID);
    if (c->root_windows_grid > 0) grid = std::min<uint64_t>(grid, (uint64_t)c->root_windows_grid);
    return (unsigned)grid;
}

int fk_root_window_estimates(fk_ctx *c, int32_t n_cells, const int64_t *batch_counts, const int64_t *const *wins, const int64_t *const *exposures,
                             const int64_t *const *completed, const int64_t *const *safety, int32_t S, int64_t n_windows, const int64_t *windows,
                             int64_t *totals, double *sums) {
    if (!c) return FK_ERR_ARG;
    if (n_cells < 1 || n_cells > FK_ROOT_WINDOW_MAX_CELLS) return fail(c, FK_ERR_ARG, "n_cells = %d: 1 to %d cells", n_cells, FK_ROOT_WINDOW_MAX_CELLS);
    if (S < 1 || S > (1 << 24)) return fail(c, FK_ERR_ARG, "S must be in [1, 2^24]");
    if (n_windows < 1 || n_windows > ((int64_t)1 << 24)) return fail(c, FK_ERR_ARG, "n_windows = %lld: 1 to 2^24 windows", (long long)n_windows);
    if (!batch_counts || !wins || !exposures || !completed || !safety || !windows) return fail(c, FK_ERR_ARG, "the cells' matrices and the windows are required");
    if (!totals || !sums) return fail(c, FK_ERR_ARG, "totals and sums are required");
    for (int32_t i = 0; i < n_cells; ++i) {
        if (batch_counts[i] < 1 || batch_counts[i] > 0x7fffffffll)
            return fail(c, FK_ERR_ARG, "cell %d: B = %lld: a batch matrix has 1 to 2^31 - 1 batches", i, (long long)batch_counts[i]);
        if (!wins[i] || !exposures[i] || !completed[i] || !safety[i]) return fail(c, FK_ERR_ARG, "cell %d: the four count matrices are required", i);
    }
    const size_t nS = (size_t)S;
    std::vector<std::vector<int64_t>> bounds((size_t)n_cells); // per cell: the rows at which a window begins or ends
    for (int64_t i = 0; i < n_windows; ++i) {
        const int64_t cell = windows[4 * i], begin = windows[4 * i + 1], end = windows[4 * i + 2], pairwise = windows[4 * i + 3];
        if (cell < 0 || cell >= n_cells) return fail(c, FK_ERR_ARG, "window %lld: cell %lld of %d", (long long)i, (long long)cell, n_cells);
        if (begin < 0 || end <= begin || end > batch_counts[cell])
            return fail(c, FK_ERR_ARG, "window %lld: rows [%lld, %lld) of a cell with %lld batches: root stability matrix slice is empty or invalid",
                        (long long)i, (long long)begin, (long long)end, (long long)batch_counts[cell]);
        if (pairwise < 0 || pairwise > S) return fail(c, FK_ERR_ARG, "window %lld: pairwise_begin = %lld outside [0, %d]", (long long)i, (long long)pairwise, S);
        bounds[(size_t)cell].push_back(begin), bounds[(size_t)cell].push_back(end);
    }
    // the reference's matrix checks (_validate_matrix_array :134-160) over every cell, and the exposure prefix of every column at every window
    // boundary: a window's column total is a difference of two of them (the scope's support check, :442-443), before anything is uploaded
    const uint64_t limit = (uint64_t)1 << 62;
    std::vector<std::vector<uint64_t>> prefix((size_t)n_cells); // [boundary][S]
    for (int32_t ci = 0; ci < n_cells; ++ci) {
        std::vector<int64_t> &bd = bounds[(size_t)ci];
        std::sort(bd.begin(), bd.end());
        bd.erase(std::unique(bd.begin(), bd.end()), bd.end());
        prefix[(size_t)ci].assign(bd.size() * nS, 0);
        std::vector<uint64_t> support(nS, 0);
        const int64_t *W = wins[ci], *E = exposures[ci], *D = completed[ci], *F = safety[ci];
        size_t next = 0, at = 0;
        for (int64_t b = 0; b <= batch_counts[ci]; ++b) {
            if (next < bd.size() && bd[next] == b) std::copy(support.begin(), support.end(), prefix[(size_t)ci].begin() + (next++) * nS);
            if (b == batch_counts[ci]) break;
            for (size_t s = 0; s < nS; ++s, ++at) {
                const int64_t w = W[at], e = E[at], done = D[at], f = F[at];
                if (w < 0 || e < 0 || done < 0 || f < 0) return fail(c, FK_ERR_ARG, "cell %d: a negative count in batch row %lld, column %zu", ci, (long long)b, s);
                if (w > done)
                    return fail(c, FK_ERR_ARG, "cell %d: wins > completed in batch row %lld, column %zu: impossible win/exposure counts", ci, (long long)b, s);
                if ((uint64_t)done + (uint64_t)f != (uint64_t)e)
                    return fail(c, FK_ERR_ARG, "cell %d: exposures != completed + safety in batch row %lld, column %zu: attempted exposure conservation", ci,
                                (long long)b, s);
                if ((uint64_t)e > limit - support[s]) return fail(c, FK_ERR_ARG, "cell %d: the exposure total of column %zu passes 2^62", ci, s);
                support[s] += (uint64_t)e;
            }
        }
    }
    for (int64_t i = 0; i < n_windows; ++i) {
        const size_t ci = (size_t)windows[4 * i];
        const std::vector<int64_t> &bd = bounds[ci];
        const size_t lo = (size_t)(std::lower_bound(bd.begin(), bd.end(), windows[4 * i + 1]) - bd.begin());
        const size_t hi = (size_t)(std::lower_bound(bd.begin(), bd.end(), windows[4 * i + 2]) - bd.begin());
        const uint64_t *p_lo = prefix[ci].data() + lo * nS, *p_hi = prefix[ci].data() + hi * nS;
        for (size_t s = 0; s < nS; ++s)
            if (p_hi[s] == p_lo[s])
                return fail(c, FK_ERR_ARG, "window %lld: root stability scope contains a strategy without positive exposure: column %zu", (long long)i, s);
    }
    // the windows in (cell, row_begin, row_end, position) order: a group per (cell, row_begin), its snapshots ascending
    std::vector<int64_t> order((size_t)n_windows);
    for (int64_t i = 0; i < n_windows; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        for (int j = 0; j < 3; ++j)
            if (windows[4 * a + j] != windows[4 * b + j]) return windows[4 * a + j] < windows[4 * b + j];
        return a < b;
    });
    std::vector<fkw::Group> groups;
    std::vector<fkw::Snap> snaps((size_t)n_windows);
    std::vector<fkw::PairTask> pairs;
    for (size_t j = 0; j < order.size(); ++j) {
        const int64_t *w = windows + 4 * order[j];
        if (groups.empty() || groups.back().cell != (uint32_t)w[0] || groups.back().row_begin != w[1])
            groups.push_back(fkw::Group{(uint32_t)w[0], (uint32_t)j, 0u, 0u, w[1]});
        ++groups.back().count;
        snaps[j] = fkw::Snap{w[2], (uint32_t)order[j], (uint32_t)w[3]};
        if (w[3] < S) pairs.push_back(fkw::PairTask{(uint32_t)w[0], (uint32_t)order[j], (uint32_t)w[3], 0u, w[1], w[2]});
    }
    HIPCHK(c, hipSetDevice(c->device));
    RootWindowBufs &b = c->rw;
    const fkl::RootWindowCells stacked((size_t)n_cells, batch_counts, nS);
    const fkl::RootWindowOut out((size_t)n_windows, nS);
    if (const int rc = ensure_all(c, b.wins, stacked.n_i64, b.exposures, stacked.n_i64, b.completed, stacked.n_i64, b.safety, stacked.n_i64, b.cells,
                                  (size_t)n_cells, b.groups, groups.size(), b.snaps, snaps.size(), b.pairs, std::max<size_t>(pairs.size(), 1), b.totals,
                                  out.n_totals, b.sums, out.n_sums))
        return rc;
    std::vector<fkw::Cell> cells((size_t)n_cells);
    for (int32_t ci = 0; ci < n_cells; ++ci) {
        const size_t at = stacked.cell_at(batch_counts, (size_t)ci), bytes = (size_t)batch_counts[ci] * nS * 8;
        cells[(size_t)ci] = fkw::Cell{b.wins.p + at, b.exposures.p + at, b.completed.p + at, b.safety.p + at, batch_counts[ci]};
        HIPCHK(c, hipMemcpyAsync(b.wins.p + at, wins[ci], bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.exposures.p + at, exposures[ci], bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.completed.p + at, completed[ci], bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b.safety.p + at, safety[ci], bytes, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(b.cells.p, cells.data(), cells.size() * sizeof(fkw::Cell), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.groups.p, groups.data(), groups.size() * sizeof(fkw::Group), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.snaps.p, snaps.data(), snaps.size() * sizeof(fkw::Snap), hipMemcpyHostToDevice, c->stream));
    if (!pairs.empty()) HIPCHK(c, hipMemcpyAsync(b.pairs.p, pairs.data(), pairs.size() * sizeof(fkw::PairTask), hipMemcpyHostToDevice, c->stream));
    const uint64_t column_blocks = ((uint64_t)S + fkw::COLUMN_BLOCK - 1) / fkw::COLUMN_BLOCK;
    hipLaunchKernelGGL(fkw::fk_rw_walk_kernel, dim3(root_windows_grid(c, groups.size() * column_blocks)), dim3(fkw::COLUMN_BLOCK), 0, c->stream, b.cells.p,
                       b.groups.p, b.snaps.p, (uint32_t)groups.size(), (uint32_t)S, b.totals.p, b.sums.p);
    if (!pairs.empty())
        hipLaunchKernelGGL(fkw::fk_rw_pairwise_kernel, dim3(root_windows_grid(c, pairs.size() * column_blocks)), dim3(fkw::COLUMN_BLOCK), 0, c->stream,
                           b.cells.p, b.pairs.p, (uint32_t)pairs.size(), (uint32_t)S, b.sums.p);
    HIPCHK(c, hipGetLastError());
    // into the caller's arrays only once the stream has come through: a failed call leaves them as they were
    std::vector<long long> h_totals(out.n_totals);
    std::vector<double> h_sums(out.n_sums);
    HIPCHK(c, hipMemcpyAsync(h_totals.data(), b.totals.p, out.n_totals * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_sums.data(), b.sums.p, out.n_sums * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::copy(h_totals.begin(), h_totals.end(), totals);
    std::copy(h_sums.begin(), h_sums.end(), sums);
    return FK_OK;
}

} // extern "C"
