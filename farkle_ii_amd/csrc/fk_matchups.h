// fk_matchups.h — the matchup family of the RNG diagnostics on the device (included by farkle_hip.hip after fk_kernels.h).
//
// Reference semantics (analysis/rng_diagnostics.py): a game's group key is its seat strategy IDs sorted ascending and padded
// with -1 to max_players columns (_extract_batch_arrays :1092-1150); its digest is
// blake2b(int32 LE [k, id_0 .. id_{k-1}, -1 ...], digest_size=8, person=b"farkle-m") read as a little-endian u64
// (_matchup_ids :1173-1185).  The group's series is n_rounds in (root_seed, k, shuffle_index, game_index) order; per lag the
// six sums of _OnlineMetric (:2032-2076) over pairs (position i - lag, position i) of the group.
//
//   fk_matchup_keys_kernel   one lane per game, beside fk_lag_values_kernel: seat table indices from the permutation, their
//                            strategy IDs, a register sorting network over (id, index), ONE BLAKE2b compression (the message is
//                            4 (1 + max_players) <= 128 bytes), and the game's record in coordinate order: digest (u64),
//                            table indices in ascending-ID order (u16 [k]), n_rounds (u16, 15 bits).
//   fkm_* kernels            the per-(root, k) reduce of fk_matchup_reduce: radix sort by digest (hipcub, stable: coordinate
//                            order survives inside a group), exact split of digest-collision runs, segments, counts,
//                            eligibility, priorities (_priority :1281), histogram bins (_observation_histogram_bin :1568), and
//                            one wave per selected group for its lag sums (no atomics on a group's sums).
#pragma once

#include <hipcub/hipcub.hpp>

namespace fkm {

constexpr uint64_t B2_IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                               0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
constexpr uint8_t B2_SIGMA[12][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
constexpr uint64_t PERSON = 0x6d2d656c6b726166ull; // b"farkle-m" read little-endian
constexpr uint32_t MAX_PLAYERS = 31;               // 4 (1 + 31) = 128 bytes: one block
constexpr uint32_t MAX_K = 16;                     // register sorting network instances

__host__ __device__ constexpr uint64_t rotr64(uint64_t x, uint32_t n) { return (x >> n) | (x << (64u - n)); }

#define FKM_G(a, b, c, d, x, y)          \
    do {                                 \
        a = a + b + (x);                 \
        d = rotr64(d ^ a, 32);           \
        c = c + d;                       \
        b = rotr64(b ^ c, 24);           \
        a = a + b + (y);                 \
        d = rotr64(d ^ a, 16);           \
        c = c + d;                       \
        b = rotr64(b ^ c, 63);           \
    } while (0)

// blake2b(msg, digest_size=8, person=b"farkle-m") of a message of `len` <= 128 bytes held in m[16] (zero padded): the first
// 8 bytes of h0 after the single, final compression = h0 ^ v0 ^ v8
__device__ __forceinline__ uint64_t blake2b8(const uint64_t (&m)[16], uint32_t len) {
    const uint64_t h0 = B2_IV[0] ^ 0x01010008ull; // digest_length 8, key_length 0, fanout 1, depth 1
    uint64_t v0 = h0, v1 = B2_IV[1], v2 = B2_IV[2], v3 = B2_IV[3], v4 = B2_IV[4], v5 = B2_IV[5], v6 = B2_IV[6] ^ PERSON, v7 = B2_IV[7];
    uint64_t v8 = B2_IV[0], v9 = B2_IV[1], v10 = B2_IV[2], v11 = B2_IV[3], v12 = B2_IV[4] ^ (uint64_t)len, v13 = B2_IV[5],
             v14 = ~B2_IV[6], v15 = B2_IV[7];
#pragma unroll
    for (int r = 0; r < 12; ++r) {
        FKM_G(v0, v4, v8, v12, m[B2_SIGMA[r][0]], m[B2_SIGMA[r][1]]);
        FKM_G(v1, v5, v9, v13, m[B2_SIGMA[r][2]], m[B2_SIGMA[r][3]]);
        FKM_G(v2, v6, v10, v14, m[B2_SIGMA[r][4]], m[B2_SIGMA[r][5]]);
        FKM_G(v3, v7, v11, v15, m[B2_SIGMA[r][6]], m[B2_SIGMA[r][7]]);
        FKM_G(v0, v5, v10, v15, m[B2_SIGMA[r][8]], m[B2_SIGMA[r][9]]);
        FKM_G(v1, v6, v11, v12, m[B2_SIGMA[r][10]], m[B2_SIGMA[r][11]]);
        FKM_G(v2, v7, v8, v13, m[B2_SIGMA[r][12]], m[B2_SIGMA[r][13]]);
        FKM_G(v3, v4, v9, v14, m[B2_SIGMA[r][14]], m[B2_SIGMA[r][15]]);
    }
    (void)v1, (void)v2, (void)v3, (void)v4, (void)v5, (void)v6, (void)v7;
    return h0 ^ v0 ^ v8;
}
#undef FKM_G

// One lane per chunk-local game id (shuffle-major, game within shuffle: coordinate order).  Safety-limit games are records
// like any other (only their winner is null, which this family does not read).
template <int K>
__global__ __launch_bounds__(256) void fk_matchup_keys_kernel(const uint32_t *recs, const uint16_t *perm_T, uint32_t perm_slots,
                                                              uint32_t S, uint32_t gps, uint32_t n_games, const int32_t *ids,
                                                              uint32_t max_players, unsigned long long *digest, uint16_t *seats,
                                                              uint16_t *rounds) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_games) return;
    const uint32_t sh = id / gps, g = id - sh * gps;
    int32_t sid[K];
    uint32_t idx[K];
#pragma unroll
    for (int s = 0; s < K; ++s) {
        idx[s] = perm_at(perm_T, S, perm_slots, sh, g * (uint32_t)K + (uint32_t)s);
        sid[s] = ids[idx[s]];
    }
    // odd-even transposition network: K rounds of compare-exchange, all indices compile-time (registers only)
#pragma unroll
    for (int r = 0; r < K; ++r) {
#pragma unroll
        for (int s = r & 1; s + 1 < K; s += 2) {
            const bool swap = sid[s + 1] < sid[s] || (sid[s + 1] == sid[s] && idx[s + 1] < idx[s]);
            const int32_t a = sid[s], b = sid[s + 1];
            const uint32_t ia = idx[s], ib = idx[s + 1];
            sid[s] = swap ? b : a, sid[s + 1] = swap ? a : b;
            idx[s] = swap ? ib : ia, idx[s + 1] = swap ? ia : ib;
        }
    }
    // int32 LE words [k, id_0 .. id_{K-1}, -1 up to max_players, 0 ...] -> sixteen u64 message words
    uint64_t m[16];
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        uint32_t lo, hi;
        const int j0 = 2 * w, j1 = 2 * w + 1;
        lo = j0 == 0 ? (uint32_t)K : j0 <= K ? (uint32_t)sid[j0 - 1 < K ? j0 - 1 : 0] : ((uint32_t)j0 <= max_players ? 0xffffffffu : 0u);
        hi = j1 <= K ? (uint32_t)sid[j1 - 1 < K ? j1 - 1 : 0] : ((uint32_t)j1 <= max_players ? 0xffffffffu : 0u);
        m[w] = (uint64_t)lo | ((uint64_t)hi << 32);
    }
    digest[id] = blake2b8(m, 4u * (1u + max_players));
    uint16_t *o = seats + (size_t)id * K;
#pragma unroll
    for (int s = 0; s < K; ++s) o[s] = (uint16_t)idx[s];
    const uint4 q0 = *reinterpret_cast<const uint4 *>(recs + (size_t)id * REC_DW);
    rounds[id] = (uint16_t)(q0.z & 0x7fffu);
}

// ---------------------------------------------------------------------------------------- reduce
__global__ void fkm_key_init(const unsigned long long *digest, unsigned long long mask, uint32_t n, unsigned long long *keys, uint32_t *vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = digest[i] & mask;
    vals[i] = i;
}

__global__ void fkm_iota(uint32_t n, uint32_t *vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) vals[i] = i;
}

// records in sorted order: sd / ss / sr [i] = digest / seats / rounds [order[i]]
__global__ void fkm_gather(const uint32_t *order, const unsigned long long *digest, const uint16_t *seats, const uint16_t *rounds, uint32_t n,
                           uint32_t k, unsigned long long *sd, uint16_t *ss, uint16_t *sr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = order[i];
    sd[i] = digest[o];
    sr[i] = rounds[o];
    for (uint32_t j = 0; j < k; ++j) ss[(size_t)i * k + j] = seats[(size_t)o * k + j];
}

__device__ __forceinline__ bool same_tuple(const uint16_t *ss, uint32_t k, uint32_t a, uint32_t b) {
    for (uint32_t j = 0; j < k; ++j)
        if (ss[(size_t)a * k + j] != ss[(size_t)b * k + j]) return false;
    return true;
}

// run_head[i]: a new run of the SORT key starts at i; tuple_break[i]: i continues a run with another tuple (a collision)
__global__ void fkm_run_heads(const unsigned long long *keys, const uint16_t *ss, uint32_t n, uint32_t k, uint32_t *run_head, uint32_t *tuple_break) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool head = i == 0 || keys[i] != keys[i - 1];
    run_head[i] = head ? 1u : 0u;
    tuple_break[i] = (!head && !same_tuple(ss, k, i, i - 1)) ? 1u : 0u;
}

// a run holding a tuple break is mixed (one atomic per break: collisions only)
__global__ void fkm_mark_mixed(const uint32_t *run_id, const uint32_t *tuple_break, uint32_t n, uint32_t *run_mixed) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && tuple_break[i]) atomicOr(&run_mixed[run_id[i] - 1u], 1u);
}

__global__ void fkm_mixed_flags(const uint32_t *run_id, const uint32_t *run_mixed, uint32_t n, uint8_t *flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (uint8_t)run_mixed[run_id[i] - 1u];
}

// secondary sort of the mixed runs: key of pass `col` (a tuple column, LSD) or the run (col == k, the last pass)
__global__ void fkm_mixed_keys(const uint32_t *pos, const uint16_t *ss, const uint32_t *run_id, uint32_t m, uint32_t k, uint32_t col,
                               uint32_t *key) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    key[j] = col < k ? (uint32_t)ss[(size_t)pos[j] * k + col] : run_id[pos[j]];
}

// the m mixed positions (ascending) receive, in order, the elements the secondary sort put there
__global__ void fkm_mixed_apply(const uint32_t *pos, const uint32_t *src_pos, const uint32_t *order_before, uint32_t m, uint32_t *order) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) order[pos[j]] = order_before[src_pos[j]];
}

// segment heads: the tuple changes (groups are contiguous now; equal tuples have equal digests)
__global__ void fkm_seg_heads(const uint16_t *ss, uint32_t n, uint32_t k, uint32_t *head) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) head[i] = (i == 0 || !same_tuple(ss, k, i, i - 1)) ? 1u : 0u;
}

__global__ void fkm_seg_starts(const uint32_t *head, const uint32_t *seg_id, uint32_t n, uint32_t *start) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && head[i]) start[seg_id[i] - 1u] = i;
    if (i == 0) start[seg_id[n - 1] ] = n;
}

__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// per segment: eligibility, priority (_priority: group_type 1 = matchup), histogram bin (_observation_histogram_bin)
__global__ void fkm_seg_info(const uint32_t *start, const unsigned long long *sd, uint32_t G, uint32_t k, uint32_t minimum,
                             uint8_t *eligible, unsigned long long *prio, int32_t *bin) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const uint32_t count = start[g + 1] - start[g];
    eligible[g] = count >= minimum ? 1 : 0;
    const uint64_t v = (uint64_t)sd[start[g]] ^ ((uint64_t)k << 48) ^ (1ull << 63);
    prio[g] = splitmix64(v ^ 0xD1B54A32D192ED03ull);
    bin[g] = count < minimum ? (int32_t)min(count, 32767u) : (int32_t)minimum + (int32_t)(31 - __clz(count - minimum + 1u));
}

// one wave per selected segment: lanes stride its positions, per-lag int64 sums in registers, butterfly reduction
constexpr uint32_t SUM_COLS = 6; // pairs, sum x, sum y, sum x^2, sum y^2, sum xy (x = the earlier observation)
__global__ __launch_bounds__(256) void fkm_group_sums(const uint32_t *sel, uint32_t M, const uint32_t *start, const unsigned long long *sd,
                                                      const uint16_t *ss, const uint16_t *sr, uint32_t k, const int32_t *lags, uint32_t n_lags,
                                                      unsigned long long *out_digest, uint16_t *out_seats, long long *out_count,
                                                      long long *out_sums) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (wave >= M) return;
    const uint32_t g = sel[wave], b = start[g], e = start[g + 1], n = e - b;
    if (lane == 0) {
        out_digest[wave] = sd[b];
        out_count[wave] = (long long)n;
    }
    for (uint32_t j = lane; j < k; j += 64u) out_seats[(size_t)wave * k + j] = ss[(size_t)b * k + j];
    for (uint32_t li = 0; li < n_lags; ++li) {
        const uint32_t lag = (uint32_t)lags[li];
        long long v[SUM_COLS] = {0, 0, 0, 0, 0, 0};
        for (uint32_t p = lag + lane; p < n; p += 64u) {
            const long long x = sr[b + p - lag], y = sr[b + p];
            v[0] += 1, v[1] += x, v[2] += y, v[3] += x * x, v[4] += y * y, v[5] += x * y;
        }
#pragma unroll
        for (int c = 0; c < (int)SUM_COLS; ++c) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_xor(v[c], off, 64);
        }
        if (lane == 0)
#pragma unroll
            for (int c = 0; c < (int)SUM_COLS; ++c) out_sums[((size_t)wave * n_lags + li) * SUM_COLS + c] = v[c];
    }
}

__global__ void fkm_gather_u64(const uint32_t *idx, const unsigned long long *src, uint32_t n, unsigned long long *dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

} // namespace fkm
