// knn_internal.h — launch interface between host_compare.cpp and knn.hip (the k nearest neighbours of every row of a triangle).
#pragma once
#include "topk_internal.h"

namespace mg {

constexpr uint32_t KNN_NT = 256;               // work-items per workgroup of the mirror passes
constexpr uint32_t KNN_SCAN_TILE = 8 * KNN_NT; // entries of the degree array one workgroup of the scan takes

// The mirror of a thresholded triangle list.  The list holds every unordered pair once: entry idx is pair {row, col} = rc[idx],
// col < row, counts cnt[idx], and it is eligible iff bit idx of `masks` is set (finish_mark_kernel's ballots).  The mirror gives
// every eligible entry to BOTH its rows: row i's segment is sym_counts / sym_nbr[base[i] .. base[i] + deg[i]), sym_nbr the other
// end of the pair.  The order of the entries inside a segment is unspecified (atomic cursors): launch_topk_select_keyed ranks
// by sym_nbr, so nothing depends on it.
struct KnnMirror {
    const uint2 *rc, *cnt;
    const unsigned long long *masks;
    uint64_t K;                        // list entries
    uint32_t n;                        // rows of the table
    uint32_t *deg;                     // [n + 1] eligible neighbours per row; deg[n] = 0
    uint32_t *base;                    // [n + 1] exclusive scan of deg; base[n] = 2 * eligible < 2^32
    uint32_t *cur;                     // [n] the scatter's cursors, zeroed by launch_knn_mirror
    uint32_t *block_sum;               // [knn_scan_blocks(n)] the scan's scratch
    uint2 *sym_counts;                 // [2 * eligible]
    uint32_t *sym_nbr;                 // [2 * eligible]
};

uint64_t knn_scan_blocks(uint32_t n);
// degree pass, scan, scatter (deg, base, cur and the segments are written; everything else is read)
hipError_t launch_knn_degree(const KnnMirror &m, hipStream_t stream);
hipError_t launch_knn_scan(const KnnMirror &m, hipStream_t stream);
hipError_t launch_knn_scatter(const KnnMirror &m, hipStream_t stream);

#ifndef MG_HIP_EMU
// matrix route: row r of a block of `nrows` rows x ncols columns that starts at table row first_row loses its own column
// (bit r * ncols + first_row + r of the eligibility ballots)
hipError_t launch_knn_clear_self(unsigned long long *masks, uint32_t nrows, uint64_t ncols, uint64_t first_row, hipStream_t stream);
// topk_finish_kernel for the mirrored segments: a.counts = the mirror's sym_counts, row = f.first_row + r, col = sym_nbr[sel];
// distance and p-value take their arguments in the triangle's order (the later row first), so the doubles are those of
// mg_compare_tri_pairs_host for the unordered pair
hipError_t launch_knn_finish(const FinishArgs &f, const TopkArgs &a, const uint32_t *sym_nbr, const unsigned long long *row_off, FinishEdge *out,
                             hipStream_t stream);
#endif

}  // namespace mg
