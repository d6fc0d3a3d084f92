// fk_bootstrap.h — the performance stage's joint deterministic-batch bootstrap on the device (included by farkle_hip.hip after
// fk_kernels.h).
//
// Reference semantics (analysis/performance.py: _BootstrapRangeWriter.__call__ :838-928, _reduce_bootstrap_ranges :1013-1111;
// _joint_batch_resampling :715-833 states the same in memory).  Per replicate r and player count k, stream = coordinate
// (BOOTSTRAP = 400, root, k, replicate_index = r); B_k bounded draws in [0, B_k) resample the k's eligible batches; the resampled
// integer totals give score[r][s] = mean over k of (wins / exposures - 1 / k); every replicate is ranked and reduced.
//
//   fk_boot_counts_kernel    one lane per (replicate, cell) stream (a cell: a player count here, a (root, player count) of
//                            fk_root_stability.h; the purpose is a launch argument): SeedSequence -> PCG64DXSM -> B_k Lemire draws on the
//                            buffered 32-bit stream (a rejected draw shifts every later one: a stream is sequential), counted into
//                            the stream's own multiplicity row counts[replicate][batch] (zeroed before the launch).
//   fk_boot_score_kernel     the hot path: [R x B] . [B x S] in exact 64-bit integers.  Strategy on the lane (matrix rows are read
//                            coalesced), RB replicates per workgroup in registers (a matrix tile is read once per RB replicates),
//                            their multiplicities for BT batches in LDS (uniform ds_read_b128).  The float tail is the reference's
//                            sequence of separate IEEE operations.  (A uint32 instance for matrices whose values fit 32 bits — half
//                            the bytes, one v_mad_u64_u32 per term — was measured and not kept: DESIGN.md section 5.5.)
//   fk_boot_rank_kernel      counting rank: rank_i = 1 + #{j : score_j > score_i or (score_j == score_i and j < i)} =
//                            lexsort((strategies, -score)) for ascending strategy columns.  Scores become order-preserving 64-bit keys
//                            (ties stay ties), tiles of keys pass through LDS; a workgroup walks RC replicates and adds its sums once.
//   fk_boot_contrast_kernel  one lane per (control, strategy) walks the block's replicates in ascending order, continuing the sums.
//
// Float code here must not be contracted into FMAs (numpy rounds every operation; hipcc contracts a * b + c by default): every kernel
// with float arithmetic opens with `#pragma clang fp contract(off)`.
#pragma once

namespace fkb {

constexpr uint32_t RB = 16;  // replicates per workgroup of the score kernel (2 x RB 64-bit accumulators per lane)
constexpr uint32_t BT = 64;  // batches per LDS tile of multiplicities
constexpr uint32_t TS = 256; // strategies per workgroup
constexpr uint32_t RC = 8;   // replicates per workgroup of the rank kernel
constexpr uint32_t JT = 2048; // keys per LDS tile of the rank kernel
constexpr uint32_t PURPOSE_BOOTSTRAP = 400;                // RandomPurpose.BOOTSTRAP
constexpr uint32_t PURPOSE_ROOT_STABILITY_BOOTSTRAP = 401; // RandomPurpose.ROOT_STABILITY_BOOTSTRAP (fk_root_stability.h)

// One resampled cell: a player count of the performance stage's root, or a (root, player count) of the two-root stability stage.
struct KDesc {
    uint64_t root;  // the coordinate's root_seed
    uint64_t k;     // player count (the coordinate's k)
    uint32_t B;     // eligible batches
    uint32_t row0;  // first row of this player count in the stacked matrices = its offset in a replicate's multiplicity row
    double chance;  // 1.0 / k, divided on the host
};

__device__ inline void rng_from_coord(Rng &r, const fk_coord &c) {
    SeedPool p;
    ss_begin(p, 2u, c.purpose, (uint32_t)c.root_seed, (uint32_t)(c.root_seed >> 32));
    ss_absorb64(p, c.k);
    ss_absorb64(p, c.shuffle_index);
    ss_absorb64(p, c.pair_id);
    ss_absorb64(p, c.order);
    ss_absorb64(p, c.game_index);
    ss_absorb64(p, c.seat_index);
    ss_absorb64(p, c.replicate_index);
    uint32_t g[8];
    ss_generate<8>(p, g);
    pcg_seed(r, g);
}

// Generator.integers(0, bound) for 2 <= bound < 2^32: numpy's buffered_bounded_lemire_uint32 (bound 1 draws nothing: the caller's case)
__device__ inline uint32_t bounded_draw(Rng &r, uint32_t bound) {
    uint64_t m = (uint64_t)pcg_next32(r) * bound;
    uint32_t left = (uint32_t)m;
    if (left < bound) {
        const uint32_t threshold = (0u - bound) % bound; // (2^32 - bound) mod bound
        while (left < threshold) {
            m = (uint64_t)pcg_next32(r) * bound;
            left = (uint32_t)m;
        }
    }
    return (uint32_t)(m >> 32);
}

// counts: [n_rep_padded][sum_B] uint32, zero on entry; stream t = (replicate r0 + t / n_k, cell t % n_k) of the caller's purpose
__global__ __launch_bounds__(64) void fk_boot_counts_kernel(uint32_t purpose, uint64_t r0, uint32_t n_rep, uint32_t n_k, const KDesc *kd,
                                                             uint32_t sum_B, uint32_t *counts) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rep * n_k) return;
    const uint32_t rr = t / n_k;
    const KDesc d = kd[t - rr * n_k];
    uint32_t *row = counts + (size_t)rr * sum_B + d.row0;
    if (d.B == 1u) { // numpy's rng == 0 branch: every result is 0, nothing is drawn
        row[0] = 1u;
        return;
    }
    fk_coord c{};
    c.purpose = purpose;
    c.root_seed = d.root;
    c.k = d.k;
    c.replicate_index = r0 + rr;
    Rng r;
    rng_from_coord(r, c);
    for (uint32_t i = 0; i < d.B; ++i) row[bounded_draw(r, d.B)] += 1u; // (the row is this lane's own)
}

// fk_debug_bounded_draws: out[i][0 .. n_draws) of stream coords[i]
__global__ __launch_bounds__(64) void fk_boot_draws_kernel(int64_t n, const fk_coord *coords, uint32_t bound, uint32_t n_draws, uint32_t *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t *o = out + (size_t)i * n_draws;
    if (bound == 1u) {
        for (uint32_t j = 0; j < n_draws; ++j) o[j] = 0u;
        return;
    }
    Rng r;
    rng_from_coord(r, coords[i]);
    for (uint32_t j = 0; j < n_draws; ++j) o[j] = bounded_draw(r, bound);
}

// One cell's resampled totals of NR replicates (rr0 ...) for the lane's strategy column sr: w[r] += counts[r][b] * W[b][sr], e likewise, in
// exact 64-bit integers over the cell's batches.  The multiplicities of BT batches pass through LDS (cnt) and are read as uniform
// ds_read_b128; every lane of the workgroup calls this together.
template <uint32_t NR>
__device__ inline void cell_totals(const int64_t *W, const int64_t *E, const uint32_t *counts, const KDesc &d, uint32_t sum_B, uint32_t S,
                                   uint32_t sr, uint32_t rr0, uint4 (*cnt)[NR / 4], uint64_t (&w)[NR], uint64_t (&e)[NR]) {
    for (uint32_t b0 = 0; b0 < d.B; b0 += BT) {
        const uint32_t nb = min(BT, d.B - b0);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < BT * NR; i += TS) {
            const uint32_t r = i / BT, b = i - r * BT; // consecutive lanes read consecutive batches of one replicate
            const uint32_t v = b < nb ? counts[(size_t)(rr0 + r) * sum_B + d.row0 + b0 + b] : 0u;
            reinterpret_cast<uint32_t *>(&cnt[b][0])[r] = v;
        }
        __syncthreads();
        const int64_t *wp = W + (size_t)(d.row0 + b0) * S + sr, *ep = E + (size_t)(d.row0 + b0) * S + sr;
        for (uint32_t b = 0; b < nb; ++b) {
            const uint64_t wv = (uint64_t)wp[(size_t)b * S], ev = (uint64_t)ep[(size_t)b * S];
#pragma unroll
            for (uint32_t q = 0; q < NR / 4; ++q) {
                const uint4 c4 = cnt[b][q];
                w[4 * q + 0] += (uint64_t)c4.x * wv, e[4 * q + 0] += (uint64_t)c4.x * ev;
                w[4 * q + 1] += (uint64_t)c4.y * wv, e[4 * q + 1] += (uint64_t)c4.y * ev;
                w[4 * q + 2] += (uint64_t)c4.z * wv, e[4 * q + 2] += (uint64_t)c4.z * ev;
                w[4 * q + 3] += (uint64_t)c4.w * wv, e[4 * q + 3] += (uint64_t)c4.w * ev;
            }
        }
    }
}

// grid = (ceil(S / TS), n_rep_padded / RB), block = TS.  W / E: the stacked [sum_B][S] matrices.  scores: [n_rep_padded][S].
// *bad is set when a resampled exposure total is <= 0 (the reference's ValueError).
__global__ __launch_bounds__(TS) void fk_boot_score_kernel(const int64_t *W, const int64_t *E, const uint32_t *counts, const KDesc *kd, uint32_t n_k,
                                                           uint32_t sum_B, uint32_t S, uint32_t n_rep, double *scores, int32_t *bad) {
#pragma clang fp contract(off)
    __shared__ uint4 cnt[BT][RB / 4];
    const uint32_t s = blockIdx.x * TS + threadIdx.x;
    const uint32_t sr = min(s, S - 1u); // lanes past the last strategy read its column and write nothing
    const uint32_t rr0 = blockIdx.y * RB;
    double score[RB];
#pragma unroll
    for (uint32_t r = 0; r < RB; ++r) score[r] = 0.0;
    bool any_bad = false;
    for (uint32_t ki = 0; ki < n_k; ++ki) {
        const KDesc d = kd[ki];
        uint64_t w[RB], e[RB];
#pragma unroll
        for (uint32_t r = 0; r < RB; ++r) w[r] = 0, e[r] = 0;
        cell_totals<RB>(W, E, counts, d, sum_B, S, sr, rr0, cnt, w, e);
#pragma unroll
        for (uint32_t r = 0; r < RB; ++r) {
            const long long tw = (long long)w[r], te = (long long)e[r];
            if (te <= 0 && rr0 + r < n_rep) any_bad = true;
            // total_wins / total_exposures - 1.0 / k, added to the replicate's score: three roundings (:925-927)
            const double rate = (double)tw / (double)(te > 0 ? te : 1);
            score[r] = score[r] + (rate - d.chance);
        }
    }
    if (s >= S) return;
    if (any_bad) *bad = 1;
    const double nk = (double)n_k;
#pragma unroll
    for (uint32_t r = 0; r < RB; ++r)
        if (rr0 + r < n_rep) scores[(size_t)(rr0 + r) * S + s] = score[r] / nk;
}

// Order-preserving key of a finite score: a > b <=> key(a) > key(b), a == b <=> key(a) == key(b) (-0.0 and 0.0 share a key).
// The smallest key (of -inf) is above 0, so key - 1 never wraps.
__device__ inline uint64_t score_key(double x) {
    const uint64_t b = x == 0.0 ? 0ull : (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ inline double key_score(uint64_t key) {
    const uint64_t b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
    return __longlong_as_double((long long)b);
}

// grid = (ceil(S / TS), ceil(n_rep / RC)), block = TS.  out: u64 [4][S] = rank sum | rank square sum | top-n count | shortlist count
__global__ __launch_bounds__(TS) void fk_boot_rank_kernel(const double *scores, uint32_t S, uint32_t n_rep, uint32_t top_n, double delta,
                                                          unsigned long long *out) {
#pragma clang fp contract(off)
    __shared__ unsigned long long keys[JT];
    __shared__ unsigned long long kmax;
    const uint32_t s0 = blockIdx.x * TS, s = s0 + threadIdx.x;
    const uint32_t sr = min(s, S - 1u);
    unsigned long long rank_sum = 0, rank_sq = 0, top = 0, shortlist = 0;
    const uint32_t r_end = min((blockIdx.y + 1u) * RC, n_rep);
    for (uint32_t r = blockIdx.y * RC; r < r_end; ++r) {
        const double *row = scores + (size_t)r * S;
        const double mine = row[sr];
        const uint64_t ki = score_key(mine);
        uint64_t seen_max = 0;
        uint32_t above = 0;
        if (threadIdx.x == 0) kmax = 0;
        for (uint32_t j0 = 0; j0 < S; j0 += JT) {
            const uint32_t nj = min(JT, S - j0);
            __syncthreads();
            for (uint32_t j = threadIdx.x; j < nj; j += TS) {
                const uint64_t kj = score_key(row[j0 + j]);
                keys[j] = kj;
                seen_max = max(seen_max, kj);
            }
            __syncthreads();
            // columns before this lane's win ties (kj >= ki <=> kj > ki - 1), columns after it do not
            const uint32_t split = s > j0 ? min(s - j0, nj) : 0u; // columns [0, split) of the tile come before s
            const uint64_t ki_before = ki - 1u;
            uint32_t j = 0;
            for (; j < split; ++j) above += keys[j] > ki_before ? 1u : 0u;
            for (; j < nj; ++j) above += keys[j] > ki ? 1u : 0u;
        }
        atomicMax(&kmax, (unsigned long long)seen_max);
        __syncthreads();
        const double best = key_score(kmax);
        const unsigned long long rank = (unsigned long long)above + 1ull;
        rank_sum += rank;
        rank_sq += rank * rank;
        top += rank <= top_n ? 1u : 0u;
        shortlist += mine >= best - delta ? 1u : 0u;
        __syncthreads(); // (kmax is reset by the next replicate)
    }
    if (s >= S) return;
    atomicAdd(&out[s], rank_sum);
    atomicAdd(&out[(size_t)S + s], rank_sq);
    atomicAdd(&out[2 * (size_t)S + s], top);
    atomicAdd(&out[3 * (size_t)S + s], shortlist);
}

// one lane per (control, strategy): sums[0][c][s] += d, sums[1][c][s] += d * d over the block's replicates in ascending order
__global__ __launch_bounds__(256) void fk_boot_contrast_kernel(const double *scores, uint32_t S, uint32_t n_rep, const int32_t *controls,
                                                               uint32_t n_controls, double *sums) {
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n_controls * S) return;
    const uint32_t c = (uint32_t)(t / S), s = (uint32_t)(t - (size_t)c * S);
    const uint32_t ctrl = (uint32_t)controls[c];
    double sum = sums[t], sq = sums[(size_t)n_controls * S + t];
    for (uint32_t r = 0; r < n_rep; ++r) {
        const double d = scores[(size_t)r * S + s] - scores[(size_t)r * S + ctrl];
        const double dd = d * d; // rounded, then added
        sum = sum + d;
        sq = sq + dd;
    }
    sums[t] = sum;
    sums[(size_t)n_controls * S + t] = sq;
}

} // namespace fkb
