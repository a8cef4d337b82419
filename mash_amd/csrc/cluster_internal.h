// cluster_internal.h — launch interface between host_compare.cpp and cluster.hip (single-linkage clusters of a thresholded triangle).
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

}  // namespace mg
