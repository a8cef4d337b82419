// cluster_internal.h — launch interface between host_cluster.cpp and cluster.hip (single-linkage clusters of a thresholded triangle),
// cluster_medoid.hip (the same clusters with their medoids), cluster_greedy.hip (greedy representative clusters of the same graph) and
// cluster_forest.hip (its minimum spanning forest), cluster_complete.hip (its complete-linkage clusters) and cluster_density.hip (its
// density clusters), and the lock-free union-find that cluster.hip, cluster_medoid.hip, cluster_forest.hip and cluster_density.hip share.
#pragma once
#include "finish_internal.h"          // (under MG_HIP_EMU that header brings tools/hipemu: tests/test_cluster_emu.py)
#include <stdint.h>

namespace mg {

// ---- the union-find over parent[n] (invariants and the staleness argument: the head of cluster.hip)
__device__ __forceinline__ uint32_t cl_load(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x as far as this work-item can see, halving the path on the way
__device__ __forceinline__ uint32_t cl_find(uint32_t *parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = cl_load(parent + x);
        if (p == x) return x;
        const uint32_t g = cl_load(parent + p);
        if (g == p) return p;
        atomicMin(parent + x, g);
        x = g;
    }
}

__device__ __forceinline__ void cl_unite(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = cl_find(parent, a);
        b = cl_find(parent, b);
        if (a == b) return;                                    // one tree already: no atomic (nearly every edge of a dense cluster)
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t was = atomicCAS(parent + hi, hi, lo);
        if (was == hi) return;
        a = was;                                               // hi had been linked by somebody else: go on from where it points
        b = lo;
    }
}

// Where the pairs of a job stand in the index space of a larger table (extending an earlier clustering: ref's rows, then qry's):
// the job's own {row, col} must be below {rows, cols}, and the pair is {row_base + row, col_base + col} there.  The whole
// triangle of a table of n rows is {n, n, 0, 0}.
struct PairSpace { uint32_t rows, cols, row_base, col_base; };

// parent[i] = i for the n rows
hipError_t launch_cluster_init(uint32_t *parent, uint32_t n, hipStream_t stream);
// parent[i] = seed[i] for i < n_old (an earlier partition in the form launch_cluster_label writes: seed[i] <= i, which the caller
// has checked -- (I1) holds from the first union on), parent[i] = i for n_old <= i < n
hipError_t launch_cluster_seed(uint32_t *parent, const uint32_t *seed, uint32_t n_old, uint32_t n, hipStream_t stream);
// Every set bit of a.masks (finish_mark_kernel's ballots: bit idx = pair idx of a.counts) joins the clusters of its {row, col}
// (pair_rc: a.list_rc, or the flat triangle from a.first_row on).  Only a.masks, a.pairs, a.list_rc, a.first_row, a.ncols and
// a.triangle are read.  Rows and columns must be < n.
hipError_t launch_cluster_union(const FinishArgs &a, uint32_t *parent, uint32_t n, hipStream_t stream);
// The same with a base per side: pair {row, col} of the job joins rows sp.row_base + row and sp.col_base + col of parent[], which
// must hold sp.row_base + sp.rows and sp.col_base + sp.cols rows at least.  A rect job gives row = query, col = reference.
hipError_t launch_cluster_union(const FinishArgs &a, uint32_t *parent, const PairSpace &sp, hipStream_t stream);
// label[i] = smallest row of i's cluster, *n_roots = number of clusters.  A launch of its own behind the last union.
hipError_t launch_cluster_label(uint32_t *parent, uint32_t n, uint32_t *label, unsigned long long *n_roots, hipStream_t stream);

// ---- cluster_medoid.hip
// launch_cluster_union (the form with a PairSpace) that also scores: every set bit inside sp joins the clusters of its {row, col} AND
// adds medoid_weight(a.counts[idx]) (forest_key.h) to score[row] and score[col], 64-bit adds.  score[] holds what parent[] holds and
// lives across the blocks of a call; the caller clears it once, before the first block.  a.counts is read besides what
// launch_cluster_union reads, at set bits only.  Bits that are clear, behind a.pairs or outside sp add nothing.  plain: two atomics
// per edge; otherwise the lanes of a word that hold the same row -- in any order, adjacent or not -- combine in the wave first.  Both
// leave the same bits.
hipError_t launch_medoid_union(const FinishArgs &a, uint32_t *parent, unsigned long long *score, const PairSpace &sp, hipStream_t stream,
                               bool plain = false);
// Behind launch_cluster_label, on the same stream: medoid[i] = among the rows of label[i]'s cluster the one with the largest score,
// equal scores to the smallest row (a row without an edge: itself).  best[n] and pick[n] are scratch, cleared here.
hipError_t launch_medoid_pick(const uint32_t *label, const unsigned long long *score, uint32_t n, unsigned long long *best, uint32_t *pick,
                              uint32_t *medoid, hipStream_t stream);

// ---- cluster_greedy.hip
// Every set bit of a.masks (as launch_cluster_union reads them) is appended as {x = larger, y = smaller index} at
// edges[atomicAdd(cursor, ...)], in no particular order.  *cursor always advances by the number of set bits; an entry whose place
// is at or behind `cap` is not written and *overflow is set: the caller regrows, puts *cursor back and appends the job again.
hipError_t launch_greedy_append(const FinishArgs &a, uint32_t n, uint2 *edges, uint64_t cap, unsigned long long *cursor, uint32_t *overflow,
                                hipStream_t stream);
// The same with a base per side (launch_cluster_union): {hi, lo} in the larger table's index space.  Cursor, `cap` and *overflow as above.
hipError_t launch_greedy_append(const FinishArgs &a, const PairSpace &sp, uint2 *edges, uint64_t cap, unsigned long long *cursor,
                                uint32_t *overflow, hipStream_t stream);
// state[i] for i < n_old: REP where seed[i] == i (seed == nullptr: everywhere), else MEMBER -- an earlier result in the form
// launch_greedy_assign writes; state[i] = UNDECIDED for n_old <= i < n.  The rounds then run over all n rows.
hipError_t launch_greedy_seed(uint32_t *state, const uint32_t *seed, uint32_t n_old, uint32_t n, hipStream_t stream);
// `rounds` rounds of the fixpoint over state[n] (all zero before the first round: every row open).  left[r] = rows still open
// behind round r of this batch (the launcher zeroes left[0 .. rounds)); a round behind one that left none does nothing.  The
// fixpoint is reached with the first left[r] == 0; at most n rounds are ever needed.
hipError_t launch_greedy_rounds(const uint2 *edges, uint64_t m, uint32_t *state, uint32_t n, uint32_t *left, uint32_t rounds, hipStream_t stream);
// Behind the fixpoint: rep[i] = i for a representative, else the smallest representative i has an edge to; *n_reps = representatives.
// With `first`: rep[] holds rows first .. n - 1 only (rep[i - first], values in the index space of all n rows), from the edges whose
// hi >= first; *n_reps still counts over all n rows.
hipError_t launch_greedy_assign(const uint2 *edges, uint64_t m, const uint32_t *state, uint32_t n, uint32_t *rep, unsigned long long *n_reps,
                                hipStream_t stream, uint32_t first = 0);
// The rounds over a list with counts (launch_forest_append's {hi, lo, numer, denom}): the same fixpoint, the counts are not read.
hipError_t launch_greedy_rounds(const uint4 *edges, uint64_t m, uint32_t *state, uint32_t n, uint32_t *left, uint32_t rounds, hipStream_t stream);
// Behind the fixpoint over that list: rep[i] = i for a representative, else the representative -- of smaller or larger index -- whose
// edge to i is best in the order of forest_key.h (the larger numer/denom exactly; equal fractions: the smaller representative);
// *n_reps = representatives.  best_key[n] is scratch (cleared here).  Denominators must be below FOREST_DENOM_LIMIT.
hipError_t launch_nearest_assign(const uint4 *edges, uint64_t m, const uint32_t *state, uint32_t n, unsigned long long *best_key, uint32_t *rep,
                                 unsigned long long *n_reps, hipStream_t stream);

// ---- what cluster_forest.hip and cluster_complete.hip share: a per-row best under a monotone 64-bit atomic
constexpr unsigned long long CF_NONE = ~0ull;

__device__ __forceinline__ unsigned long long cf_load(unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// atomicMax(&best[c], v) for the lanes with `on`, skipping what cannot win (F2 of cluster_forest.hip); one atomic for the wave where they all name one
// component.  Called by whole waves.
__device__ __forceinline__ void cf_offer_max(unsigned long long *best, bool on, uint32_t c, unsigned long long v)
{
    const unsigned long long act = __ballot(on);
    if (!act) return;                                          // (wave-uniform)
    const uint32_t first = (uint32_t)__builtin_ctzll(act);
    const uint32_t c0 = __shfl(c, first);
    if (__ballot(on && c != c0) == 0) {
        unsigned long long k = on ? v : 0ull;
        for (uint32_t d = 32; d; d >>= 1) {
            const unsigned long long o = __shfl_xor(k, d);
            if (o > k) k = o;
        }
        if ((threadIdx.x & 63) == first && k > cf_load(best + c0)) atomicMax(best + c0, k);
    } else if (on && v > cf_load(best + c)) {
        atomicMax(best + c, v);
    }
}

__device__ __forceinline__ void cf_offer_min(unsigned long long *best, bool on, uint32_t c, unsigned long long v)
{
    const unsigned long long act = __ballot(on);
    if (!act) return;                                          // (wave-uniform)
    const uint32_t first = (uint32_t)__builtin_ctzll(act);
    const uint32_t c0 = __shfl(c, first);
    if (__ballot(on && c != c0) == 0) {
        unsigned long long k = on ? v : CF_NONE;
        for (uint32_t d = 32; d; d >>= 1) {
            const unsigned long long o = __shfl_xor(k, d);
            if (o < k) k = o;
        }
        if ((threadIdx.x & 63) == first && k < cf_load(best + c0)) atomicMin(best + c0, k);
    } else if (on && v < cf_load(best + c)) {
        atomicMin(best + c, v);
    }
}

// ---- cluster_forest.hip
// launch_greedy_append with the pair's counts beside it: {x = larger, y = smaller index, z = numer, w = denom} of a.counts, 16 bytes an
// edge.  Cursor, `cap` and *overflow as there.
hipError_t launch_forest_append(const FinishArgs &a, uint32_t n, uint4 *edges, uint64_t cap, unsigned long long *cursor, uint32_t *overflow,
                                hipStream_t stream);
// What the rounds work on, all of it written by the launches below (nothing has to be cleared before the call)
struct ForestBufs {
    uint32_t *parent, *comp;                   // [n] the union-find; the flat component of a row as of the end of the round before
    unsigned long long *best_key, *best_rc;    // [n] per component of this round: its best weight key, the smallest {hi, lo} that has it
    uint4 *forest;                             // [forest_room(n)] the chosen edges: in the order they were picked, then sorted
    unsigned long long *count;                 // [1] how many of them
    uint32_t *merged;                          // [forest_rounds(n)] edges chosen by round r
    unsigned long long *live;                  // [forest_rounds(n)] edges that were live when round r began
};
uint32_t forest_rounds(uint32_t n);            // floor(log2 n) + 2: one more than any graph of n rows needs, the last of them finds nothing
uint64_t forest_room(uint32_t n);              // the power of two >= max(n, 2): room for the n - 1 edges and the sort's padding
// Everything behind the last append, queued as one batch: the rounds (a round behind one that chose no edge does nothing), then
// label / *n_roots as launch_cluster_label gives them, then the chosen edges best first by the exact comparator, forest[*count ..
// forest_room(n)) padded, and seen[d] = 1 for every denominator d <= s they carry (seen[0 .. s] cleared first).
hipError_t launch_forest_rounds(const uint4 *edges, uint64_t m, const ForestBufs &b, uint32_t n, uint32_t *label, unsigned long long *n_roots,
                                uint32_t *seen, uint32_t s, hipStream_t stream);
// out[i] = the finished record of forest[i], i < count: f's distance table and lengths, the device functions of finish.hip
hipError_t launch_forest_finish(const FinishArgs &f, const uint4 *forest, uint64_t count, FinishEdge *out, hipStream_t stream);

// ---- cluster_complete.hip
// What the complete-linkage rounds work on.  The LINKS are the appended list itself ({hi, lo, numer, denom}; an entry with hi == lo
// is skipped by every reader); everything here is written by launch_complete_begin and the rounds.
struct CompleteBufs {
    uint32_t *parent, *mate;                   // [n] "larger id under smaller" of every merge so far; this round's partner of an id (~0: none)
    unsigned long long *best_key, *best_rc;    // [n] per id of this round: the best weight key of its links, the smallest {hi, lo} that has it
    unsigned long long *key, *next;            // [m] a link's weight key (forest_key.h) or CC_DEAD; what K4 decided it becomes
    unsigned long long *slot_rc, *slot_e;      // [slots] the lookup: forest_rc(hi, lo) of a link (CF_NONE: empty) and its place in the list
    uint64_t slots;                            // complete_slots(m): the load is below one half
    uint64_t hash_and, hash_or;                // ~0 and 0; a test narrows the hash with them so that probes collide and wrap
    uint32_t *merged;                          // [rounds of a batch] links merged by round r
    unsigned long long *live;                  // [rounds of a batch] links alive when round r began
};
constexpr unsigned long long CC_DEAD = ~0ull;  // (a key is at most 2^42)
uint64_t complete_slots(uint64_t m);           // 2 m + 1
// Behind the last append: parent[i] = i, the rows' round state cleared, key[e] = forest_key(numer, denom) (CC_DEAD for an entry with
// hi == lo), and the lookup built -- every slot emptied, then every link's {hi, lo} put in by a 64-bit compare-and-swap on slot_rc.
hipError_t launch_complete_begin(const uint4 *edges, uint64_t m, const CompleteBufs &b, uint32_t n, hipStream_t stream);
// `rounds` rounds as one batch (the launcher zeroes merged / live [0 .. rounds)): round r of the batch does nothing once round r - 1
// of it merged nothing.  The fixpoint is the first merged[r] == 0; at most n rounds are ever needed.
hipError_t launch_complete_rounds(const uint4 *edges, uint64_t m, const CompleteBufs &b, uint32_t n, uint32_t rounds, hipStream_t stream);

// ---- cluster_density.hip
// What the density passes work on, all of it written by launch_density (nothing has to be cleared before the call)
struct DensityBufs {
    uint32_t *deg, *parent;                    // [n] edges with an end at the row; the union-find over the cores
    uint32_t *label, *via, *first;             // [n] the results; per label the smallest row filed under it
    unsigned long long *best_key;              // [n] per row that is not a core: the best weight key among its edges to cores
    unsigned long long *counts;                // [5] cores, borders, noise, clusters, scratch
};
// Everything behind the last append of {hi, lo, numer, denom} (launch_forest_append; an entry with hi == lo is skipped), queued as one
// batch: deg[i] = edges at i; a row is a core iff deg >= min_neighbours; the cores united over the edges between two of them; a row
// that is no core but has an edge to one is a border under via[i] = the core whose edge is best in the order of forest_key.h (equal
// fractions: the smaller core); via[i] = i for cores and for the rest (noise); label[i] = the smallest row of i's cluster, borders
// included; counts[0 .. 3] = cores, borders, noise, rows with label[i] == i.  Denominators must be below FOREST_DENOM_LIMIT.
// plain_degree: two atomic adds per edge instead of one per run of equal rows in a wave; the same deg[].
hipError_t launch_density(const uint4 *edges, uint64_t m, const DensityBufs &b, uint32_t n, uint32_t min_neighbours, bool plain_degree, hipStream_t stream);

}  // namespace mg
