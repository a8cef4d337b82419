// topk_internal.h — launch interface between host_compare.cpp and topk.hip (the k nearest references per query).
#pragma once
#ifdef MG_HIP_EMU                    // tools/hipemu: the selection kernel on host fibers (tests/test_topk_emu.py)
#include "hipemu.h"
#else
#include <hip/hip_runtime.h>
#include "finish_internal.h"
#endif
#include <stdint.h>

namespace mg {

constexpr uint32_t TOPK_MAX = 1024;          // = MG_TOPK_MAX (include/mashgpu.h): the kept list and one chunk share the LDS buffer
constexpr uint32_t TOPK_NT = 256;            // work-items per row
constexpr uint32_t TOPK_CHUNK = 4 * TOPK_NT; // pairs streamed between two looks at the buffer
constexpr uint32_t TOPK_SHORT = 64;          // rows of up to this many pairs are ranked by one wave, a lane per pair
constexpr uint32_t TOPK_BUF = TOPK_MAX + TOPK_CHUNK;   // 2048: a power of two, the largest sort

// A row's pairs are counts[begin .. begin + n) IN COLUMN ORDER, where
//   matrix block: begin = row * ncols, n = ncols                        (seg_base == nullptr)
//   candidate list: begin = seg_base[row], n = seg_cnt[row]             (cand_lists: base / byrow)
// and pair idx is eligible iff bit idx of `masks` is set (finish_mark_kernel's ballots; nullptr: every pair).
struct TopkArgs {
    const uint2 *counts;               // {numer, denom}
    const unsigned long long *masks;
    const uint32_t *seg_base, *seg_cnt;
    uint32_t ncols, nrows, k;          // 1 <= k <= TOPK_MAX
    uint32_t *sel;                     // [nrows * k] index into counts of the row's j-th best, best first
    uint32_t *row_n;                   // [nrows] min(k, eligible)
    uint32_t *denom_seen;              // [s + 1] denominators of the selected (for the distance table); may be nullptr
    uint32_t s;
    const uint32_t *key;               // launch_topk_select_keyed only: pair idx's second key, unique within its row (else nullptr)
};

hipError_t launch_topk_select(const TopkArgs &a, hipStream_t stream);
// the same selection with equal fractions by ascending key[idx] instead of by position: a row's pairs may lie in any order
// (candidate-list layout only: seg_base and seg_cnt are set)
hipError_t launch_topk_select_keyed(const TopkArgs &a, hipStream_t stream);

#ifndef MG_HIP_EMU
// row_off = exclusive scan of row_n, *total = its sum (one workgroup)
hipError_t launch_topk_scan(const uint32_t *row_n, unsigned long long *row_off, uint32_t nrows, unsigned long long *total, hipStream_t stream);
// the selected pairs as full records, query major and best first: out[row_off[row] + j].  f: counts, first_row, ncols, lengths,
// distance table, kmer_space and list_rc as for the other finish kernels.
hipError_t launch_topk_finish(const FinishArgs &f, const TopkArgs &a, const unsigned long long *row_off, FinishEdge *out, hipStream_t stream);
#endif

}  // namespace mg
