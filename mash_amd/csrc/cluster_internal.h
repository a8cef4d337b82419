// cluster_internal.h — launch interface between host_compare.cpp and cluster.hip (single-linkage clusters of a thresholded triangle)
// and cluster_greedy.hip (greedy representative clusters of the same graph).
#pragma once
#include "finish_internal.h"          // (under MG_HIP_EMU that header brings tools/hipemu: tests/test_cluster_emu.py)
#include <stdint.h>

namespace mg {

// parent[i] = i for the n rows
hipError_t launch_cluster_init(uint32_t *parent, uint32_t n, hipStream_t stream);
// Every set bit of a.masks (finish_mark_kernel's ballots: bit idx = pair idx of a.counts) joins the clusters of its {row, col}
// (pair_rc: a.list_rc, or the flat triangle from a.first_row on).  Only a.masks, a.pairs, a.list_rc, a.first_row, a.ncols and
// a.triangle are read.  Rows and columns must be < n.
hipError_t launch_cluster_union(const FinishArgs &a, uint32_t *parent, uint32_t n, hipStream_t stream);
// label[i] = smallest row of i's cluster, *n_roots = number of clusters.  A launch of its own behind the last union.
hipError_t launch_cluster_label(uint32_t *parent, uint32_t n, uint32_t *label, unsigned long long *n_roots, hipStream_t stream);

// ---- cluster_greedy.hip
// Every set bit of a.masks (as launch_cluster_union reads them) is appended as {x = larger, y = smaller index} at
// edges[atomicAdd(cursor, ...)], in no particular order.  *cursor always advances by the number of set bits; an entry whose place
// is at or behind `cap` is not written and *overflow is set: the caller regrows, puts *cursor back and appends the job again.
hipError_t launch_greedy_append(const FinishArgs &a, uint32_t n, uint2 *edges, uint64_t cap, unsigned long long *cursor, uint32_t *overflow,
                                hipStream_t stream);
// `rounds` rounds of the fixpoint over state[n] (all zero before the first round: every row open).  left[r] = rows still open
// behind round r of this batch (the launcher zeroes left[0 .. rounds)); a round behind one that left none does nothing.  The
// fixpoint is reached with the first left[r] == 0; at most n rounds are ever needed.
hipError_t launch_greedy_rounds(const uint2 *edges, uint64_t m, uint32_t *state, uint32_t n, uint32_t *left, uint32_t rounds, hipStream_t stream);
// Behind the fixpoint: rep[i] = i for a representative, else the smallest representative i has an edge to; *n_reps = representatives.
hipError_t launch_greedy_assign(const uint2 *edges, uint64_t m, const uint32_t *state, uint32_t n, uint32_t *rep, unsigned long long *n_reps,
                                hipStream_t stream);

}  // namespace mg
