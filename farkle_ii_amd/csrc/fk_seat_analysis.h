// fk_seat_analysis.h — the seat-analysis stage on the device (included by farkle_hip.hip after fk_kernels.h and fk_matchups.h).
//
// Reference semantics (analysis/seat_analysis.py): per (deterministic batch, strategy, seat) the counts raw_wins,
// raw_completed_exposures, raw_safety_limit_exposures (_iter_seat_count_tables :170-235); for k = 2, per (batch, unordered pair
// a < b by strategy ID) the mirrored-game pairing of _MirroredPartitionWriter.__call__ (:618-714): a forward game (seat 1 = a)
// is paired with the oldest waiting reverse game and the other way round.  The two FIFO queues are never both non-empty, so the
// i-th completed forward game meets the i-th completed reverse game; with nF / nR completed forward / reverse games and
// m = min(nF, nR):   paired = m,   difference = sum(P1-win of the first m forward) - sum(P1-win of the first m reverse),
// unpaired forward / reverse = nF - m / nR - m, completed = nF + nR, safety = the segment's safety-limit games.
//
//   fk_seat_counts_kernel      thread = (strategy, part of a batch's shuffles), as fk_seat_stats_kernel: the strategy's position
//                              through the inverse permutation, that game's rec0 word, k x 3 32-bit counters in LDS
//                              (column-major over the workgroup's threads: conflict-free, no runtime-indexed registers), one
//                              64-bit atomic per non-zero counter at the end — none per exposure.
//   fk_mirror_record_kernel    per chunk, one lane per game: sort key (rank a, rank b, batch) and payload (orientation, P1-win)
//                              at the game's coordinate index of the call-resident arrays.
//   (stable radix sort by key, hipcub: coordinate order survives inside a (pair, batch) segment)
//   fk_mirror_flags_kernel     per sorted element: completed-forward / completed-reverse / safety indicators, segment and pair heads;
//                              exclusive sums of them give every element its rank among the completed games of its own
//                              orientation inside its segment, and every segment its totals.
//   fk_mirror_starts_kernel    segment / pair starts from the heads.
//   fk_mirror_segment_kernel   per element that is a completed P1 win: +1 (forward) / -1 (reverse) to its segment's difference
//                              when its rank < m.
//   fk_mirror_pair_sum_kernel  thread = pair: the closed form of each of its (adjacent) segments, summed over the batches.
#pragma once

namespace fksa {

constexpr uint32_t MAX_K = 16;
constexpr uint32_t COUNT_COLS = 3;   // wins, completed exposures, safety-limit exposures
constexpr uint32_t COUNT_BLOCK = 256;
constexpr uint32_t PAIR_COLS = 6;    // paired, difference sum, completed, safety, unpaired forward, unpaired reverse
constexpr unsigned long long KEY_DROPPED = ~0ull; // a game whose seats hold one strategy: sorts last, counts nowhere
constexpr uint32_t ORIENT_FORWARD = 0, ORIENT_REVERSE = 1, ORIENT_SAFETY = 2, ORIENT_NONE = 3, P1_WIN = 4;

// counts [n_batches][S][k][3] (added to: chunks continue the sums of a batch they cut); dynamic LDS: k * 3 * COUNT_BLOCK dwords
__global__ __launch_bounds__(COUNT_BLOCK) void fk_seat_counts_kernel(const uint32_t *rec0, const uint16_t *inv_T, uint32_t perm_slots, uint32_t S,
                                                                     uint32_t k, uint32_t gps, uint32_t n_sh, uint32_t sh_offset, uint32_t spb,
                                                                     uint32_t parts_per_batch, uint32_t first_batch, long long *counts) {
    extern __shared__ uint32_t fksa_acc[]; // [k * 3][COUNT_BLOCK]
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b_local = blockIdx.y / parts_per_batch, part = blockIdx.y - b_local * parts_per_batch;
    const uint32_t batch = first_batch + b_local;
    const uint64_t g_lo = (uint64_t)batch * spb, g_hi = g_lo + spb;
    const uint32_t sh_lo = g_lo > sh_offset ? (uint32_t)(g_lo - sh_offset) : 0u;
    const uint32_t sh_hi = (uint32_t)min<uint64_t>(n_sh, g_hi > sh_offset ? g_hi - sh_offset : 0u);
    if (s >= S || sh_hi <= sh_lo) return; // (no barrier below: every thread owns its LDS column)
    const uint32_t per_part = (sh_hi - sh_lo + parts_per_batch - 1u) / parts_per_batch;
    const uint32_t first = sh_lo + part * per_part, last = min(first + per_part, sh_hi);
    uint32_t *acc = fksa_acc + threadIdx.x;
    for (uint32_t c = 0; c < k * COUNT_COLS; ++c) acc[c * COUNT_BLOCK] = 0u;
    for (uint32_t sh = first; sh < last; ++sh) {
        const uint32_t p = perm_at(inv_T, S, perm_slots, sh, s); // position = game * k + seat of the strategy in this shuffle
        const uint32_t g = p / k, seat = p - g * k;
        const uint32_t d0 = rec0[(size_t)sh * gps + g];
        const bool safety = (d0 & REC_SAFETY) != 0u;
        uint32_t *cell = acc + seat * COUNT_COLS * COUNT_BLOCK;
        if (safety) {
            cell[2u * COUNT_BLOCK] += 1u;
        } else {
            cell[1u * COUNT_BLOCK] += 1u;
            if (((d0 >> 24) & 0x7fu) == seat) cell[0] += 1u;
        }
    }
    long long *out = counts + ((size_t)batch * S + s) * k * COUNT_COLS;
    for (uint32_t c = 0; c < k * COUNT_COLS; ++c) {
        const uint32_t v = acc[c * COUNT_BLOCK];
        if (v) atomicAdd(reinterpret_cast<unsigned long long *>(&out[c]), (unsigned long long)v);
    }
}

// k = 2.  One lane per chunk-local game id; the record goes to index game_base + id of the call's arrays.
__global__ __launch_bounds__(256) void fk_mirror_record_kernel(const uint32_t *rec0, const uint16_t *perm_T, uint32_t perm_slots, uint32_t S,
                                                               uint32_t gps, uint32_t n_games, uint32_t sh_offset, uint32_t spb,
                                                               const uint16_t *id_rank, uint32_t game_base, unsigned long long *keys,
                                                               uint32_t *vals) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_games) return;
    const uint32_t sh = id / gps, g = id - sh * gps;
    const uint32_t r0 = id_rank[perm_at(perm_T, S, perm_slots, sh, 2u * g)], r1 = id_rank[perm_at(perm_T, S, perm_slots, sh, 2u * g + 1u)];
    const uint32_t d0 = rec0[id];
    unsigned long long key = KEY_DROPPED;
    uint32_t val = ORIENT_NONE;
    if (r0 != r1) {
        const uint32_t a = min(r0, r1), b = max(r0, r1), batch = (sh_offset + sh) / spb;
        key = ((unsigned long long)a << 48) | ((unsigned long long)b << 32) | (unsigned long long)batch;
        if (d0 & REC_SAFETY) val = ORIENT_SAFETY;
        else val = (r0 < r1 ? ORIENT_FORWARD : ORIENT_REVERSE) | ((((d0 >> 24) & 0x7fu) == 0u) ? P1_WIN : 0u);
    }
    keys[game_base + id] = key;
    vals[game_base + id] = val;
}

// Sorted elements -> indicator words (arrays of n + 1 entries, the last one 0, so that an exclusive sum ends with the totals):
//   fr = completed forward | completed reverse << 32      sh = safety | segment head << 32      ph = pair head
__global__ void fk_mirror_flags_kernel(const unsigned long long *keys, const uint32_t *vals, uint32_t n, unsigned long long *fr,
                                       unsigned long long *sh, uint32_t *ph) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    unsigned long long f = 0, s = 0;
    uint32_t p = 0;
    if (i < n && keys[i] != KEY_DROPPED) {
        const unsigned long long key = keys[i], prev = i ? keys[i - 1] : KEY_DROPPED;
        const uint32_t o = vals[i] & 3u;
        f = o == ORIENT_FORWARD ? 1ull : o == ORIENT_REVERSE ? (1ull << 32) : 0ull;
        s = (o == ORIENT_SAFETY ? 1ull : 0ull) | ((i == 0u || key != prev) ? (1ull << 32) : 0ull);
        p = (i == 0u || (key >> 32) != (prev >> 32)) ? 1u : 0u;
    }
    fr[i] = f;
    sh[i] = s;
    ph[i] = p;
}

// e_sh / e_ph: the exclusive sums.  seg_start [G + 1] (the last segment ends at n: dropped games, all indicators 0, trail it),
// pair_start [P + 1] in segments.
__global__ void fk_mirror_starts_kernel(const unsigned long long *sh, const unsigned long long *e_sh, const uint32_t *ph, const uint32_t *e_ph,
                                        uint32_t n, uint32_t *seg_start, uint32_t *pair_start) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const uint32_t seg = (uint32_t)(e_sh[i] >> 32);
    if (i == n) {
        seg_start[seg] = n;
        pair_start[e_ph[n]] = seg;
        return;
    }
    if (sh[i] >> 32) seg_start[seg] = i;
    if (ph[i]) pair_start[e_ph[i]] = seg;
}

// seg_diff [G] (zeroed): the P1-win difference of every segment.  Only completed P1 wins reach the atomic.
__global__ void fk_mirror_segment_kernel(const unsigned long long *keys, const uint32_t *vals, uint32_t n, const unsigned long long *e_fr,
                                         const unsigned long long *e_sh, const uint32_t *seg_start, int32_t *seg_diff) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || keys[i] == KEY_DROPPED) return;
    const uint32_t v = vals[i], o = v & 3u;
    if (o > ORIENT_REVERSE || !(v & P1_WIN)) return;
    const uint32_t seg = (uint32_t)(e_sh[i + 1u] >> 32) - 1u;
    const uint32_t s0 = seg_start[seg], s1 = seg_start[seg + 1u];
    const unsigned long long tot = e_fr[s1] - e_fr[s0], mine = e_fr[i] - e_fr[s0]; // (both halves are monotone: no borrow)
    const uint32_t m = min((uint32_t)tot, (uint32_t)(tot >> 32));
    const uint32_t rank = o == ORIENT_FORWARD ? (uint32_t)mine : (uint32_t)(mine >> 32);
    if (rank < m) atomicAdd(&seg_diff[seg], o == ORIENT_FORWARD ? 1 : -1);
}

// total[0] = P.  Rows p < capacity: pair_rank [p][2] = (rank a, rank b), pair_sums [p][6].
__global__ void fk_mirror_pair_sum_kernel(const unsigned long long *keys, const unsigned long long *e_fr, const unsigned long long *e_sh,
                                          const uint32_t *e_ph, uint32_t n, const uint32_t *seg_start, const uint32_t *pair_start,
                                          const int32_t *seg_diff, unsigned long long capacity, uint16_t *pair_rank, long long *pair_sums,
                                          unsigned long long *total) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t P = e_ph[n];
    if (p == 0u) total[0] = P;
    if (p >= P || p >= capacity) return;
    long long v[PAIR_COLS] = {0, 0, 0, 0, 0, 0};
    const uint32_t g0 = pair_start[p], g1 = pair_start[p + 1u];
    for (uint32_t seg = g0; seg < g1; ++seg) {
        const uint32_t s0 = seg_start[seg], s1 = seg_start[seg + 1u];
        const unsigned long long tot = e_fr[s1] - e_fr[s0];
        const long long nf = (uint32_t)tot, nr = (uint32_t)(tot >> 32), m = nf < nr ? nf : nr;
        v[0] += m;
        v[1] += seg_diff[seg];
        v[2] += nf + nr;
        v[3] += (uint32_t)(e_sh[s1] - e_sh[s0]);
        v[4] += nf - m;
        v[5] += nr - m;
    }
    const unsigned long long key = keys[seg_start[g0]];
    pair_rank[2u * p] = (uint16_t)(key >> 48);
    pair_rank[2u * p + 1u] = (uint16_t)(key >> 32);
#pragma unroll
    for (int c = 0; c < (int)PAIR_COLS; ++c) pair_sums[(size_t)p * PAIR_COLS + c] = v[c];
}

} // namespace fksa
