// cluster_forest.hip — the minimum spanning forest of a thresholded all-vs-all, found on the device: the third consumer of pass A's
// ballots (finish_mark_kernel).  The reference has no such command (its user pipes `mash triangle -E` through a sort and a
// script); an EDGE is a pair that passes the filters of CommandDistance.cpp:409-422, the ORDER of the edges is the exact fraction
// numer/denom, larger first, equal fractions by ascending {row, col} (forest_key.h), and the FOREST is what Kruskal keeps when it
// walks the edges in that order.  The order is strict and total, so the minimum spanning forest is UNIQUE: whatever finds it finds
// the same set.  Cut at any threshold it is the single-linkage partition of that threshold; read in order, the dendrogram.
//
// The ballots of a matrix block live until the next block and every round needs every edge, so the edges are first appended to a list
// of {hi, lo, numer, denom} (hi > lo), one atomic on the cursor per wave and 64 ballot words (cf_append_kernel: cg_append_kernel's
// scheme with the pair's counts beside it).
//
// Boruvka rounds over that list.  Two arrays over the rows: parent[], cluster.hip's union-find, and comp[], the FLAT component of a
// row as of the end of the round before.  An edge is LIVE while comp[hi] != comp[lo].  A round is four launches:
//   K1 (cf_key_kernel), per live edge and end:  atomicMax(&best_key[comp[end]], key)          key: forest_key.h, orders as the fraction
//       (it also counts the round's live edges into live[r], one atomic per wave and launch: what tools/forest_bench.py reports)
//   K2 (cf_rc_kernel),  per live edge and end whose best_key == key:  atomicMin(&best_rc[comp[end]], hi << 32 | lo)
//   K3 (cf_pick_kernel), per live edge: CHOSEN iff hi << 32 | lo == best_rc of either end's component -- the best edge that leaves
//       that component.  A chosen edge is written to the forest list (a ballot, one atomic on its cursor per wave, which also counts
//       merged[r]) and its ends are united in parent[] (cl_unite).  An edge has one work-item and is live in one round only once
//       chosen -- its ends share a component from then on -- so it is written once.
//   K4 (cf_flatten_kernel), per row: comp[i] = find(i), and best_key / best_rc of the next round reset (0 / ~0).
// WHY STALE READS CANNOT HURT.
//   (F1) comp[], best_key[] and best_rc[] are only DECIDED ON in launches behind the one that wrote them: K1 reads comp (K4 of the
//        round before), K2 reads best_key (K1), K3 reads best_rc (K2).  The kernel boundary has made them visible; comp[] does not
//        change while edges are read, so "live" means the same to K1, K2 and K3 of a round.
//   (F2) Inside a launch the only racing accesses are the monotone atomics on best_key (only ever raised) and best_rc (only ever
//        lowered), and the union's on parent[], which has its proof in cluster.hip.  The relaxed agent-scope load in front of an atomic
//        (cf_offer_*, cluster_internal.h) only SKIPS an edge that cannot win: a stale value is an older one -- smaller for best_key, larger for best_rc --
//        so a stale read can only let through an atomic that changes nothing.  The final value is the max / min over all offers,
//        whatever the order.
//   (F3) The picks of a round are acyclic: were they a cycle of components, each edge of it would have to rank strictly before the
//        next one round the cycle, and the order is strict.  So every chosen edge joins two trees that no other chosen edge of any
//        round joins, the forest list holds at most n - 1 edges, and parent[] ends as cluster.hip's does: one tree per connected
//        component, its root the smallest row -- label[] and the clusters are mg_cluster_tri_host's.
//   (F4) The best edge out of a component belongs to the minimum spanning forest (the cut property, strict order), so K3 never writes
//        an edge Kruskal would drop; a round with a live edge chooses at least the best live edge of all, so merged[r] == 0 iff no edge
//        is live: the fixpoint.
// Termination: every component with a live edge is merged with another one in each round, so their number at least halves: a graph
// of n rows has chosen its last edge after floor(log2 n) rounds, and one more finds nothing.  Every launch of round r first reads
// merged[r - 1] and returns if it is zero (as the greedy rounds do with left[]), so the host queues forest_rounds(n) = floor(log2 n)
// + 2 rounds at once and waits once.
// Contention: in the last rounds a few components receive every live edge's atomic.  cf_offer_max / cf_offer_min first look (F2),
// and where all live lanes of a wave name one component (a ballot) they reduce over the wave and issue one atomic.
// Behind the rounds, in the same batch: the labels (cl_label_kernel), the forest list padded to a power of two and sorted by a bitonic
// network on the exact cross-multiplication (forest_before, not the key: the order of the output leans on the definition alone), the
// denominators it carries.  cf_finish_kernel then finishes the records as topk.hip does: distance from the host-libm table, p-value by
// pvalue.h -- the doubles are bit-equal to mg_compare_tri_results_host's.
//
// Compiles for tools/hipemu too (MG_HIP_EMU, tests/test_forest_emu.py): wave operations sit in uniform control flow, nothing relies on
// the lock step of a wave.
#include "cluster_internal.h"
#include "forest_key.h"
#ifndef MG_HIP_EMU
#include "pvalue.h"
#endif

namespace mg {

constexpr int CF_NT = 256;

// cg_append_kernel with the counts: a wave loads 64 ballot words, counts their bits, takes room for all of them with ONE atomicAdd on
// the cursor, then writes the words that are not zero one after the other, a lane per bit.  An entry whose place is at or behind `cap`
// is not written (the cursor still counts it: the host reads how much room the block needed).
__global__ __launch_bounds__(CF_NT) void cf_append_kernel(FinishArgs a, uint32_t n, uint4 *edges, unsigned long long cap, unsigned long long *cursor,
                                                         uint32_t *overflow)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t words = (a.pairs + 63) / 64;
    const uint64_t nwaves = (uint64_t)gridDim.x * (CF_NT / 64);
    for (uint64_t w0 = ((uint64_t)blockIdx.x * (CF_NT / 64) + (threadIdx.x >> 6)) * 64; w0 < words; w0 += nwaves * 64) {   // (wave-uniform)
        unsigned long long mine = w0 + lane < words ? a.masks[w0 + lane] : 0ull;
        if (w0 + lane + 1 == words && (a.pairs & 63)) mine &= (1ull << (a.pairs & 63)) - 1;      // (bits behind a.pairs are zero anyway)
        unsigned long long nz = __ballot(mine != 0);
        if (!nz) continue;
        const uint32_t cnt = (uint32_t)__popcll(mine);
        uint32_t incl = cnt;                                   // inclusive scan of the words' bit counts over the wave
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const uint32_t total = __shfl(incl, 63);
        unsigned long long base = 0;
        if (lane == 0) {
            base = atomicAdd(cursor, (unsigned long long)total);
            if (base + total > cap) atomicOr(overflow, 1u);
        }
        base = __shfl(base, 0);
        const uint32_t excl = incl - cnt;
        while (nz) {                                           // (wave-uniform)
            const uint32_t j = (uint32_t)__builtin_ctzll(nz);
            nz &= nz - 1;
            const unsigned long long m = __shfl(mine, j);
            const uint32_t off = __shfl(excl, j);
            if ((m >> lane) & 1) {
                const unsigned long long at = base + off + (uint32_t)__popcll(m & ((1ull << lane) - 1));
                if (at < cap) {
                    const uint64_t idx = (w0 + j) * 64 + lane;
                    uint64_t row, col;
                    pair_rc(a, idx, row, col);
                    uint4 e = make_uint4(0u, 0u, 0u, 0u);      // (a pair outside the table: an entry every reader skips, hi == lo)
                    if (row < n && col < n) {
                        const uint2 c = a.counts[idx];
                        e = make_uint4((uint32_t)(row > col ? row : col), (uint32_t)(row > col ? col : row), c.x, c.y);
                    }
                    edges[at] = e;
                }
            }
        }
    }
}

__global__ __launch_bounds__(CF_NT) void cf_init_kernel(ForestBufs b, uint32_t n)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        b.parent[i] = i;
        b.comp[i] = i;
        b.best_key[i] = 0;
        b.best_rc[i] = CF_NONE;
    }
}

// One edge per lane of a wave-uniform loop: what K1, K2 and K3 all start from.  live: the edge exists and its ends lie in two components
struct CfEdge {
    uint4 x;
    uint32_t ch, cl;                                           // comp[hi], comp[lo]
    bool live;
};

__device__ __forceinline__ CfEdge cf_edge(const uint4 *edges, unsigned long long e, unsigned long long m, const uint32_t *comp)
{
    CfEdge r;
    r.x = make_uint4(0u, 0u, 0u, 0u);
    r.ch = r.cl = 0;
    r.live = false;
    if (e < m) {
        r.x = edges[e];
        if (r.x.x > r.x.y) {
            r.ch = comp[r.x.x];
            r.cl = comp[r.x.y];
            r.live = r.ch != r.cl;
        }
    }
    return r;
}

// `go`: the edges the round before chose (nullptr: the first round); a round queued behind the fixpoint does nothing
// *live += the live edges this round starts with (a wave counts over its whole stride: one atomic per wave and launch)
__global__ __launch_bounds__(CF_NT) void cf_key_kernel(const uint4 *edges, unsigned long long m, ForestBufs b, const uint32_t *go, unsigned long long *live)
{
    if (go && *go == 0) return;                                // (written by an earlier launch; uniform over the grid)
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long n_live = 0;
    for (unsigned long long e0 = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); e0 < m; e0 += stride) {   // (wave-uniform)
        const CfEdge e = cf_edge(edges, e0 + lane, m, b.comp);
        const unsigned long long key = e.live ? forest_key(e.x.z, e.x.w) : 0ull;
        n_live += (unsigned long long)__popcll(__ballot(e.live));
        cf_offer_max(b.best_key, e.live, e.ch, key);
        cf_offer_max(b.best_key, e.live, e.cl, key);
    }
    if (lane == 0 && n_live) atomicAdd(live, n_live);
}

__global__ __launch_bounds__(CF_NT) void cf_rc_kernel(const uint4 *edges, unsigned long long m, ForestBufs b, const uint32_t *go)
{
    if (go && *go == 0) return;
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e0 = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); e0 < m; e0 += stride) {   // (wave-uniform)
        const CfEdge e = cf_edge(edges, e0 + lane, m, b.comp);
        const unsigned long long key = e.live ? forest_key(e.x.z, e.x.w) : 0ull, rc = forest_rc(e.x.x, e.x.y);
        cf_offer_min(b.best_rc, e.live && b.best_key[e.ch] == key, e.ch, rc);      // (best_key: K1's, an earlier launch)
        cf_offer_min(b.best_rc, e.live && b.best_key[e.cl] == key, e.cl, rc);
    }
}

// n: a forest has fewer than n edges (F3); the guard keeps every write inside the list whatever the list holds
__global__ __launch_bounds__(CF_NT) void cf_pick_kernel(const uint4 *edges, unsigned long long m, ForestBufs b, uint32_t n, const uint32_t *go, uint32_t *merged)
{
    if (go && *go == 0) return;
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e0 = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); e0 < m; e0 += stride) {   // (wave-uniform)
        const CfEdge e = cf_edge(edges, e0 + lane, m, b.comp);
        const unsigned long long rc = forest_rc(e.x.x, e.x.y);
        const bool chosen = e.live && (b.best_rc[e.ch] == rc || b.best_rc[e.cl] == rc);        // (best_rc: K2's, an earlier launch)
        const unsigned long long pick = __ballot(chosen);
        if (!pick) continue;                                   // (wave-uniform)
        const uint32_t first = (uint32_t)__builtin_ctzll(pick), cnt = (uint32_t)__popcll(pick);
        unsigned long long base = 0;
        if (lane == first) {
            base = atomicAdd(b.count, (unsigned long long)cnt);
            atomicAdd(merged, cnt);
        }
        base = __shfl(base, first);
        if (chosen) {
            const unsigned long long at = base + (uint32_t)__popcll(pick & ((1ull << lane) - 1));
            if (at < n) b.forest[at] = e.x;
            cl_unite(b.parent, e.x.x, e.x.y);
        }
    }
}

// one work-item per row; the walks end at the true roots: every link was made by an earlier launch
__global__ __launch_bounds__(CF_NT) void cf_flatten_kernel(ForestBufs b, uint32_t n, const uint32_t *go)
{
    if (go && *go == 0) return;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        b.comp[i] = cl_find(b.parent, i);
        b.best_key[i] = 0;
        b.best_rc[i] = CF_NONE;
    }
}

// forest[*count .. room): entries that rank behind every edge (0/1 under the largest row pair there is)
__global__ __launch_bounds__(CF_NT) void cf_pad_kernel(uint4 *forest, const unsigned long long *count, unsigned long long room)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = *count + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < room; i += stride)
        forest[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 1u);
}

// one compare-exchange step (k, j) of the bitonic network over forest[0 .. room), best first
__global__ __launch_bounds__(CF_NT) void cf_sort_step_kernel(uint4 *forest, unsigned long long room, unsigned long long k, unsigned long long j)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < room; i += stride) {
        const unsigned long long l = i ^ j;
        if (l <= i) continue;
        const uint4 a = forest[i], c = forest[l];
        const bool c_first = forest_before(c.z, c.w, forest_rc(c.x, c.y), a.z, a.w, forest_rc(a.x, a.y));
        if (((i & k) == 0) == c_first) {                       // (the pair {a, c} is strictly ordered: c_first false means a ranks first)
            forest[i] = c;
            forest[l] = a;
        }
    }
}

__global__ __launch_bounds__(CF_NT) void cf_denoms_kernel(const uint4 *forest, const unsigned long long *count, uint32_t s, uint32_t *seen)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x, cnt = *count;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += stride)
        if (forest[i].w <= s) __hip_atomic_store(seen + forest[i].w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a store, no
                                                               //  read-modify-write: at one species every edge names the same word)
}

static uint32_t cf_blocks(uint64_t items, uint32_t cap)
{
    const uint64_t b = (items + CF_NT - 1) / CF_NT;
    return (uint32_t)(b < 1 ? 1 : b > cap ? cap : b);
}

hipError_t launch_forest_append(const FinishArgs &a, uint32_t n, uint4 *edges, uint64_t cap, unsigned long long *cursor, uint32_t *overflow,
                                hipStream_t stream)
{
    if (a.pairs == 0 || n == 0) return hipSuccess;
    // a work-item per mask word up to 2048 workgroups (8 per CU of an MI355X): beyond that the waves stride
    hipLaunchKernelGGL(cf_append_kernel, dim3(cf_blocks((a.pairs + 63) / 64, 2048)), dim3(CF_NT), 0, stream, a, n, edges, (unsigned long long)cap,
                       cursor, overflow);
    return hipGetLastError();
}

uint32_t forest_rounds(uint32_t n)
{
    uint32_t lg = 0;
    while ((n >> lg) > 1) lg++;
    return lg + 2;
}

uint64_t forest_room(uint32_t n)
{
    uint64_t room = 2;
    while (room < n) room <<= 1;
    return room;
}

hipError_t launch_forest_rounds(const uint4 *edges, uint64_t m, const ForestBufs &b, uint32_t n, uint32_t *label, unsigned long long *n_roots,
                                uint32_t *seen, uint32_t s, hipStream_t stream)
{
    const uint32_t rounds = forest_rounds(n);
    const uint64_t room = forest_room(n);
    hipError_t e = hipMemsetAsync(b.merged, 0, (size_t)rounds * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(b.live, 0, (size_t)rounds * sizeof(unsigned long long), stream);
    if (e == hipSuccess) e = hipMemsetAsync(b.count, 0, sizeof(unsigned long long), stream);
    if (e == hipSuccess) e = hipMemsetAsync(seen, 0, ((size_t)s + 1) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (n) hipLaunchKernelGGL(cf_init_kernel, dim3(cf_blocks(n, 2048)), dim3(CF_NT), 0, stream, b, n);
    for (uint32_t r = 0; r < rounds && m && n; r++) {
        const uint32_t *go = r ? b.merged + (r - 1) : nullptr;
        const dim3 grid(cf_blocks(m, 2048));
        hipLaunchKernelGGL(cf_key_kernel, grid, dim3(CF_NT), 0, stream, edges, (unsigned long long)m, b, go, b.live + r);
        hipLaunchKernelGGL(cf_rc_kernel, grid, dim3(CF_NT), 0, stream, edges, (unsigned long long)m, b, go);
        hipLaunchKernelGGL(cf_pick_kernel, grid, dim3(CF_NT), 0, stream, edges, (unsigned long long)m, b, n, go, b.merged + r);
        hipLaunchKernelGGL(cf_flatten_kernel, dim3(cf_blocks(n, 2048)), dim3(CF_NT), 0, stream, b, n, go);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_cluster_label(b.parent, n, label, n_roots, stream)) != hipSuccess) return e;
    if (m && n > 1) {
        const dim3 grid(cf_blocks(room, 2048));
        hipLaunchKernelGGL(cf_pad_kernel, grid, dim3(CF_NT), 0, stream, b.forest, b.count, (unsigned long long)room);
        for (uint64_t k = 2; k <= room; k <<= 1)
            for (uint64_t j = k >> 1; j; j >>= 1)
                hipLaunchKernelGGL(cf_sort_step_kernel, grid, dim3(CF_NT), 0, stream, b.forest, (unsigned long long)room, (unsigned long long)k,
                                   (unsigned long long)j);
        hipLaunchKernelGGL(cf_denoms_kernel, grid, dim3(CF_NT), 0, stream, b.forest, b.count, s, seen);
    }
    return hipGetLastError();
}

#ifndef MG_HIP_EMU
__global__ __launch_bounds__(CF_NT) void cf_finish_kernel(FinishArgs f, const uint4 *forest, unsigned long long count, FinishEdge *out)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const uint4 x = forest[i];
        FinishEdge e;
        e.row = x.x;
        e.col = x.y;
        e.numer = x.z;
        e.denom = x.w;
        e.distance = lut_distance(f, x.z, x.w);
        e.p_value = p_value(x.z, f.len_row[x.x], f.len_col[x.y], f.kmer_space, x.w);
        out[i] = e;
    }
}

hipError_t launch_forest_finish(const FinishArgs &f, const uint4 *forest, uint64_t count, FinishEdge *out, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(cf_finish_kernel, dim3(cf_blocks(count, 2048)), dim3(CF_NT), 0, stream, f, forest, (unsigned long long)count, out);
    return hipGetLastError();
}
#endif  // !MG_HIP_EMU

}  // namespace mg
