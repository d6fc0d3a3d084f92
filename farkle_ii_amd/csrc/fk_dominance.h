// fk_dominance.h — the dominance graphs of a round robin on the device (fk_dominance_graph, fk_rr_dominance), included by
// farkle_hip.hip behind fk_rr_inference.h.  What the reference's analysis/dominance.py builds from the pairwise decision classes,
// for both of its graphs in one call (index 0 practical, index 1 statistical), on dense bit matrices: node ids are table rows, a row
// of a matrix is W = ceil(n / 64) 64-bit words, bit j of row i of `adj` says "i beats j", of `adj_t` "j beats i".
//
//   fk_dm_edges_kernel      one lane per pair: the class -> the bits of both graphs (dominance.py:285-334).  Pair ids ascend along a
//                           row of the triangle, so the lanes of a wave that share row i hold consecutive columns j: their ballot,
//                           shifted, IS a run of bits of row i — one atomicOr per (row, word) run; the column side (row j, bit i) is
//                           one atomicOr per edge
//   fk_dm_panel_kernel      \  the transitive closure of adj and adj_t of both graphs (four matrices), in place on a copy, as a blocked
//   fk_dm_close_kernel      /  Warshall with 64 pivots a phase: the panel kernel copies the 64 pivot rows aside and closes their
//                           64 x 64 diagonal block in one wave (64 shuffles); the close kernel gives every row i, one wave a row,
//                           row_i |= OR of the copied rows k' in M_i, M_i = m_i | OR_{k in m_i} D*_k, m_i the row's word of the pivot
//                           block.  (A path from i through pivots of the block enters it by an edge of m_i, moves inside it along
//                           D* and leaves from a copied row: one pass is a whole Warshall phase.)  2 ceil(n / 64) launches.
//   fk_dm_component_kernel  one wave per (graph, node): the component is reach & reach_t | self — its smallest row, its size; the row
//                           popcounts of adj and adj_t (wins, losses, :386-389); the component's in-degree from outside (atomicAdd)
//   fk_dm_front_kernel      the layer peeling of the condensation (:118-136) as Kahn's rounds, one workgroup per graph, the in-degrees
//                           in LDS: a round takes every node whose component has in-degree 0, then walks the out-edges of the taken
//                           nodes once — the whole peeling reads every edge once and every node once per round
//   fk_dm_rate_kernel       balanced_a_win_rate of a resident pair, as fk_ri_decide_kernel writes it into a row
//   fk_dm_mean_kernel       one lane per strategy: the rates of its pairs in pair-id order, summed left to right (:357-395)
//   fk_dm_cycle_kernel      one workgroup per (graph, start): breadth-first search on bit-set frontiers inside the component until
//                           the frontier holds a node with an edge back to the start
//   fk_dm_extreme_*         the strongest / weakest internal practical edge of every component (:504-520): atomicMax / atomicMin on
//                           the order-preserving bit pattern of the distance, then atomicMin of rank[winner] << 32 | rank[loser]
//                           among the edges that attain it, then the decode
//
// Vector stores and ordinary atomics only.  Floating-point contraction is off where a double is computed.
#pragma once

#include <cmath>
#include <cstdint>

namespace fkdm {
namespace { // internal linkage, as fk_round_robin.h

using ull = unsigned long long;

constexpr uint32_t DM_MAX_N = 8192;        // FK_DOM_MAX_N: the front kernel's LDS (in-degrees u32 + layer list u16) and one lane per
constexpr uint32_t DM_MAX_W = DM_MAX_N / 64; // word in the cycle kernel's 128-thread workgroup
constexpr uint32_t DM_NONE = 0xffffffffu;

// doubles -> unsigned keys of the same order (negative values: all bits flipped; others: the sign bit set)
__host__ __device__ inline ull dm_order_bits(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    const ull b = (ull)__double_as_longlong(v);
#else
    ull b;
    __builtin_memcpy(&b, &v, 8);
#endif
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double dm_order_value(ull k) {
    const ull b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)b);
#else
    double v;
    __builtin_memcpy(&v, &b, 8);
    return v;
#endif
}

// dominance.py:315-319, one subtraction
__host__ __device__ inline double dm_distance(uint32_t cls, double low, double high, double delta) {
#pragma clang fp contract(off)
    return cls == 0u ? low - delta : -high - delta;
}

// what the kernels share: the four matrices and their working copies, [graph][n][W] each
struct Mats {
    ull *adj, *adj_t, *reach; // reach: [4][n][W] = the closures of adj[0], adj[1], adj_t[0], adj_t[1]
    uint32_t n, W;
};

// One lane per pair.  `cls` < 2 is an edge of both graphs, < 4 of the statistical one; even classes are won by A = row i.
__global__ __launch_bounds__(256) void fk_dm_edges_kernel(const uint8_t *__restrict__ cls, uint32_t n, uint32_t n_pairs, Mats m) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // whole waves
    const bool live = p < n_pairs;
    uint32_t i = DM_NONE, j = DM_NONE, c = 7u;
    if (live) {
        fkrr::rr_unrank(n, p, i, j);
        c = cls[p];
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i_prev = __shfl_up(i, 1u, 64);
    // a run: the lanes of one row i whose columns fall into one word; its head is the first of them
    const bool head = live && (lane == 0u || i_prev != i || (j & 63u) == 0u);
    const ull heads = __ballot(head), above = lane == 63u ? 0ull : heads >> (lane + 1u);
    const uint32_t live_end = (uint32_t)__popcll(__ballot(live)); // live lanes are the low ones
    const uint32_t run_end = above ? lane + (uint32_t)__ffsll((long long)above) : live_end;
    const size_t plane = (size_t)n * m.W;
#pragma unroll
    for (uint32_t g = 0; g < 2u; ++g) {
        const uint32_t limit = g == 0u ? 2u : 4u;
        const ull won = __ballot(c < limit && (c & 1u) == 0u), lost = __ballot(c < limit && (c & 1u) == 1u);
        if (head) {
            const uint32_t len = run_end - lane; // 1 .. 64
            const ull run = len == 64u ? ~0ull : ((1ull << len) - 1ull);
            const size_t at = g * plane + (size_t)i * m.W + (j >> 6);
            const ull w_bits = ((won >> lane) & run) << (j & 63u), l_bits = ((lost >> lane) & run) << (j & 63u);
            if (w_bits) atomicOr(&m.adj[at], w_bits);     // i beats the columns of the run
            if (l_bits) atomicOr(&m.adj_t[at], l_bits);   // the columns of the run beat i
        }
        if (c < limit) { // the column side: row j, bit i
            ull *dst = (c & 1u) ? m.adj : m.adj_t;
            atomicOr(&dst[g * plane + (size_t)j * m.W + (i >> 6)], 1ull << (i & 63u));
        }
    }
}

// Phase `kb` of the closure, step 1: grid = 4 matrices, one workgroup each.  The pivot rows [64 kb, 64 kb + 64) go to `panel`
// [4][64][W] (rows past n as zeros), the closure of their diagonal block to `dstar` [4][64].
__global__ __launch_bounds__(256) void fk_dm_panel_kernel(const ull *__restrict__ reach, uint32_t n, uint32_t W, uint32_t kb, ull *__restrict__ panel,
                                                          ull *__restrict__ dstar) {
    const uint32_t mat = blockIdx.x;
    const ull *src = reach + (size_t)mat * n * W;
    ull *dst = panel + (size_t)mat * 64u * W;
    for (uint32_t t = threadIdx.x; t < 64u * W; t += blockDim.x) {
        const uint32_t row = kb * 64u + t / W;
        dst[t] = row < n ? src[(size_t)row * W + t % W] : 0ull;
    }
    if (threadIdx.x < 64u) { // one wave: Warshall on the 64 x 64 block, row `lane` in the lane's register
        const uint32_t row = kb * 64u + threadIdx.x;
        ull d = row < n ? src[(size_t)row * W + kb] : 0ull;
        for (uint32_t k = 0; k < 64u; ++k) {
            const ull dk = __shfl(d, (int)k, 64);
            if ((d >> k) & 1ull) d |= dk;
        }
        dstar[mat * 64u + threadIdx.x] = d;
    }
}

// Phase `kb`, step 2: one wave per row, grid (ceil(n / 4), 4 matrices), 256 threads.  The wave reads its row's pivot word before it
// writes any word of the row; the pivot rows are read from the panel copy.
__global__ __launch_bounds__(256) void fk_dm_close_kernel(ull *__restrict__ reach, uint32_t n, uint32_t W, uint32_t kb, const ull *__restrict__ panel,
                                                          const ull *__restrict__ dstar) {
    const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u, mat = blockIdx.y;
    if (row >= n) return;
    ull *r = reach + ((size_t)mat * n + row) * W;
    const ull *pan = panel + (size_t)mat * 64u * W, *ds = dstar + mat * 64u;
    const ull m_i = r[kb];
    if (m_i == 0ull) return; // (wave-uniform)
    ull M = m_i;
    for (ull b = m_i; b; b &= b - 1ull) M |= ds[__ffsll((long long)b) - 1];
    for (uint32_t w = lane; w < W; w += 64u) {
        ull acc = r[w];
        for (ull b = M; b; b &= b - 1ull) acc |= pan[(size_t)(__ffsll((long long)b) - 1) * W + w];
        r[w] = acc;
    }
}

__device__ inline uint32_t dm_wave_min(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ inline uint32_t dm_wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One wave per (graph, node), grid (ceil(n / 4), 2).  comp_deg [2][n] (zeroed) receives, at the component's smallest row, the edges
// that enter the component from outside.
__global__ __launch_bounds__(256) void fk_dm_component_kernel(Mats m, fk_dom_node *__restrict__ nodes, uint32_t *__restrict__ comp,
                                                              uint32_t *__restrict__ comp_deg) {
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u, g = blockIdx.y;
    if (i >= m.n) return;
    const size_t row = ((size_t)g * m.n + i) * m.W, row_t = ((size_t)(g + 2u) * m.n + i) * m.W;
    uint32_t first = DM_NONE, size = 0u, wins = 0u, losses = 0u, entering = 0u;
    for (uint32_t w = lane; w < m.W; w += 64u) {
        ull c = m.reach[row + w] & m.reach[row_t + w];
        if ((i >> 6) == w) c |= 1ull << (i & 63u);
        if (c && first == DM_NONE) first = w * 64u + (uint32_t)__ffsll((long long)c) - 1u;
        size += (uint32_t)__popcll(c);
        const ull beats = m.adj[row + w], beaten_by = m.adj_t[row + w];
        wins += (uint32_t)__popcll(beats), losses += (uint32_t)__popcll(beaten_by);
        entering += (uint32_t)__popcll(beaten_by & ~c);
    }
    first = dm_wave_min(first), size = dm_wave_sum(size), wins = dm_wave_sum(wins), losses = dm_wave_sum(losses), entering = dm_wave_sum(entering);
    if (lane == 0u) {
        fk_dom_node &o = nodes[i];
        o.component[g] = first, o.component_size[g] = size, o.wins[g] = wins, o.losses[g] = losses, o.front[g] = 0u, o.cycle_length[g] = 0u;
        comp[(size_t)g * m.n + i] = first;
        if (entering) atomicAdd(&comp_deg[(size_t)g * m.n + first], entering);
    }
}

// One workgroup of 1024 per graph.  Thread t owns the nodes t, t + 1024, ...: it alone reads and writes their front.
__global__ __launch_bounds__(1024) void fk_dm_front_kernel(Mats m, fk_dom_node *__restrict__ nodes, const uint32_t *__restrict__ comp_all,
                                                           const uint32_t *__restrict__ comp_deg) {
    __shared__ uint32_t deg[DM_MAX_N];
    __shared__ uint16_t layer[DM_MAX_N];
    __shared__ uint32_t count;
    const uint32_t g = blockIdx.x, n = m.n, W = m.W;
    const uint32_t *comp = comp_all + (size_t)g * n;
    const ull *adj = m.adj + (size_t)g * n * W, *fwd = m.reach + (size_t)g * n * W, *bwd = m.reach + (size_t)(g + 2u) * n * W;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) deg[i] = comp_deg[(size_t)g * n + i];
    uint32_t remaining = n;
    for (uint32_t front = 1u; remaining != 0u && front <= n; ++front) {
        if (threadIdx.x == 0u) count = 0u;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
            if (nodes[i].front[g] == 0u && deg[comp[i]] == 0u) {
                nodes[i].front[g] = front;
                layer[atomicAdd(&count, 1u)] = (uint16_t)i;
            }
        __syncthreads();
        const uint32_t taken = count;
        if (taken == 0u) break; // (a condensation has no cycle: not reached)
        for (uint32_t t = threadIdx.x; t < taken * W; t += blockDim.x) { // the out-edges of the layer that leave its components
            const uint32_t u = layer[t / W], w = t % W;
            const size_t at = (size_t)u * W + w;
            for (ull b = adj[at] & ~(fwd[at] & bwd[at]); b; b &= b - 1ull) atomicSub(&deg[comp[w * 64u + (uint32_t)__ffsll((long long)b) - 1u]], 1u);
        }
        remaining -= taken;
        __syncthreads();
    }
}

// (fk_ri_decide_kernel's row: balanced_a_wins / (n_ab + n_ba) of a viable pair, NaN otherwise)
__global__ void fk_dm_rate_kernel(const ull *__restrict__ acc, uint32_t n_pairs, double *__restrict__ rate) {
#pragma clang fp contract(off)
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const fkri::PairCounts c = fkri::ri_pair_counts(acc + (size_t)p * 2u * fkri::RI_COLS);
    rate[p] = c.viable ? (double)(c.x_ab + c.a_wins_ba) / (double)(c.n_ab + c.n_ba) : NAN;
}

// One lane per strategy s: its pairs in pair-id order are (0, s) .. (s - 1, s), then (s, s + 1) .. (s, n - 1).
__global__ void fk_dm_mean_kernel(const double *__restrict__ rate, uint32_t n, fk_dom_node *__restrict__ nodes) {
#pragma clang fp contract(off)
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    double sum = 0.0;
    uint64_t count = 0;
    for (uint32_t i = 0; i < s; ++i) {
        const double r = rate[fkrr::rr_row_begin(n, i) + (s - i - 1u)];
        if (!isnan(r)) sum = sum + (1.0 - r), ++count;
    }
    const uint64_t own = fkrr::rr_row_begin(n, s);
    for (uint32_t j = s + 1u; j < n; ++j) {
        const double r = rate[own + (j - s - 1u)];
        if (!isnan(r)) sum = sum + r, ++count;
    }
    nodes[s].rate_count = count;
    nodes[s].rate_mean = count ? sum / (double)count : __longlong_as_double(0x7ff8000000000000ll);
}

// One workgroup of 128 per (start, graph): thread w holds word w of the bit sets.
__global__ __launch_bounds__(128) void fk_dm_cycle_kernel(Mats m, fk_dom_node *__restrict__ nodes) {
    __shared__ ull frontier[DM_MAX_W];
    const uint32_t s = blockIdx.x, g = blockIdx.y, w = threadIdx.x, W = m.W;
    if (nodes[s].component_size[g] < 2u) return; // (uniform; the component kernel has written 0)
    const ull *adj = m.adj + (size_t)g * m.n * W;
    const size_t at = (size_t)s * W + w;
    ull inside = 0ull, back = 0ull, seen = 0ull, mine = 0ull;
    if (w < W) {
        inside = m.reach[(size_t)g * m.n * W + at] & m.reach[(size_t)(g + 2u) * m.n * W + at]; // (the start itself is never entered: see below)
        back = m.adj_t[(size_t)g * m.n * W + at] & inside; // the nodes with an edge to the start
        mine = seen = adj[at] & inside;
    }
    uint32_t length = 0u;
    for (uint32_t level = 1u; level < m.n; ++level) {
        if (__syncthreads_or((mine & back) != 0ull)) { // a node at distance `level` closes the cycle; none nearer did
            length = level + 1u;
            break;
        }
        if (w < W) frontier[w] = mine;
        __syncthreads();
        ull next = 0ull;
        if (w < W) {
            for (uint32_t fw = 0; fw < W; ++fw)
                for (ull b = frontier[fw]; b; b &= b - 1ull) next |= adj[(size_t)(fw * 64u + (uint32_t)__ffsll((long long)b) - 1u) * W + w];
            next &= inside & ~seen; // (the start's bit is not in `inside` unless it reaches itself, which the test above saw first)
            if ((s >> 6) == w) next &= ~(1ull << (s & 63u));
            seen |= next;
        }
        mine = next;
        if (!__syncthreads_or(next != 0ull)) break; // (a component of two or more nodes has a cycle through each: not reached)
    }
    if (w == 0u) nodes[s].cycle_length[g] = length;
}

struct ExtremeBufs {
    ull *max_bits, *min_bits, *strong_key, *weak_key; // [2][n] each, by the component's smallest row
};

// One lane per pair, pass 1 (`second` false): the largest and smallest distance of the practical edges inside each component.
// Pass 2: among the edges that attain them, the smallest (rank[winner], rank[loser]).
__global__ void fk_dm_extreme_kernel(const uint8_t *__restrict__ cls, const double2 *__restrict__ sim, double delta, uint32_t n, uint32_t n_pairs,
                                     const uint32_t *__restrict__ comp, const uint32_t *__restrict__ rank, ExtremeBufs e, bool second) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const uint32_t c = cls[p];
    if (c >= 2u) return;
    uint32_t i, j;
    fkrr::rr_unrank(n, p, i, j);
    const double2 s = sim[p];
    const ull bits = dm_order_bits(dm_distance(c, s.x, s.y, delta));
    const uint32_t winner = c == 0u ? i : j, loser = c == 0u ? j : i;
    const ull key = (ull)(rank ? rank[winner] : winner) << 32 | (ull)(rank ? rank[loser] : loser);
#pragma unroll
    for (uint32_t g = 0; g < 2u; ++g) {
        const uint32_t ci = comp[(size_t)g * n + i];
        if (ci != comp[(size_t)g * n + j]) continue;
        const size_t at = (size_t)g * n + ci;
        if (!second) {
            atomicMax(&e.max_bits[at], bits);
            atomicMin(&e.min_bits[at], bits);
        } else {
            if (bits == e.max_bits[at]) atomicMin(&e.strong_key[at], key);
            if (bits == e.min_bits[at]) atomicMin(&e.weak_key[at], key);
        }
    }
}

// One lane per (graph, row): the record of a component at its smallest row; every other row, and a component without an internal
// practical edge, reads "none".  `unrank` is the inverse of `rank` (NULL: table order).
__global__ void fk_dm_extreme_out_kernel(uint32_t n, const uint32_t *__restrict__ unrank, ExtremeBufs e, fk_dom_extreme *__restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2u * n) return;
    fk_dom_extreme o;
    const double none = __longlong_as_double(0x7ff8000000000000ll);
    o.strongest_winner = o.strongest_loser = o.weakest_winner = o.weakest_loser = DM_NONE;
    o.strongest_distance = o.weakest_distance = none;
    const ull ks = e.strong_key[t], kw = e.weak_key[t];
    if (ks != ~0ull) {
        const uint32_t a = (uint32_t)(ks >> 32), b = (uint32_t)ks, c = (uint32_t)(kw >> 32), d = (uint32_t)kw;
        o.strongest_winner = unrank ? unrank[a] : a, o.strongest_loser = unrank ? unrank[b] : b;
        o.weakest_winner = unrank ? unrank[c] : c, o.weakest_loser = unrank ? unrank[d] : d;
        o.strongest_distance = dm_order_value(e.max_bits[t]), o.weakest_distance = dm_order_value(e.min_bits[t]);
    }
    out[t] = o;
}

} // namespace
} // namespace fkdm
