// finish_internal.h — launch interface between host_compare.cpp and finish.hip.
#pragma once
#ifdef MG_HIP_EMU                    // tools/hipemu: cluster.hip on host fibers (tests/test_cluster_emu.py)
#include <math.h>
#include "hipemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

namespace mg {

struct FinishPair {            // = mg_pair (include/mashgpu.h)
    uint32_t numer, denom;
    double distance, p_value;
    uint8_t pass;
    uint8_t _pad[7];
};

struct FinishEdge {            // = mg_result (include/mashgpu.h)
    uint32_t row, col, numer, denom;
    double distance, p_value;
};

struct FinishArgs {
    const uint2 *counts;           // {numer, denom} in the layout the compare kernels write
    uint64_t pairs;
    uint64_t first_row;            // triangle row / query index of counts[0]
    uint64_t ncols;                // rect: number of references
    const uint64_t *len_row;       // Reference::length by row (triangle row i / query)
    const uint64_t *len_col;       // ... by column (triangle column j / reference)
    const uint32_t *min_numer;     // [s + 1] smallest numer passing the distance filter per denom; nullptr = no filter
    const uint32_t *lut_start;     // [s + 1] first entry of denom's row in lut, 0xFFFFFFFF = not tabulated
    const double *lut;             // distances by (denom, numer), host libm
    double kmer_space;
    double max_p;                  // < 0: p-value filter off
    uint32_t s;
    uint32_t triangle;
    FinishPair *pairs_out;         // finish_pairs_kernel
    unsigned long long *masks;     // [finish_mask_words(pairs)] ballots of pass A
    uint32_t *seg_count;           // [finish_segments(pairs)]
    unsigned long long *seg_off;   // exclusive scan of seg_count
    uint32_t *denom_seen;          // [s + 1] denominators carried by survivors (pass A)
    FinishEdge *edges;             // pass B: survivors with rank in [win_lo, win_lo + win_n)
    uint64_t win_lo, win_n;
    const uint2 *list_rc;          // list mode: counts[idx] belongs to pair {row, col} = list_rc[idx] (reference order); nullptr: flat order
};

// distance of a pair from the host-libm table (finish.hip, topk.hip)
__device__ __forceinline__ double lut_distance(const FinishArgs &a, uint32_t numer, uint32_t denom)
{
    if (numer == denom) return 0.0;                                       // CommandDistance.cpp:389-392
    if (numer == 0) return 1.0;                                           // :393-396
    const uint32_t st = denom <= a.s ? a.lut_start[denom] : 0xFFFFFFFFu;
    if (st == 0xFFFFFFFFu) return __builtin_nan("");                      // not tabulated: the host patches it
    return a.lut[(uint64_t)st + numer];
}

// {row, col} of pair idx of a finish job (finish.hip, cluster.hip)
__device__ __forceinline__ void pair_rc(const FinishArgs &a, uint64_t idx, uint64_t &row, uint64_t &col)
{
    if (a.list_rc) {                                       // a list of pairs (the sparse engine's candidates), not a block of the matrix
        const uint2 rc = a.list_rc[idx];
        row = rc.x;
        col = rc.y;
        return;
    }
    if (a.triangle) {
        const uint64_t f = a.first_row;
        const uint64_t g = (f ? f * (f - 1) / 2 : 0) + idx;               // index in the whole triangle
        row = (uint64_t)((1.0 + sqrt(1.0 + 8.0 * (double)g)) * 0.5);
        while (row * (row - 1) / 2 > g) row--;
        while ((row + 1) * row / 2 <= g) row++;
        col = g - row * (row - 1) / 2;
    } else {
        row = a.first_row + idx / a.ncols;
        col = idx % a.ncols;
    }
}

uint64_t finish_segments(uint64_t pairs);
uint64_t finish_mask_words(uint64_t pairs);
hipError_t launch_finish_pairs(const FinishArgs &a, hipStream_t stream);
hipError_t launch_finish_mark(const FinishArgs &a, unsigned long long *total, hipStream_t stream);
hipError_t launch_finish_write(const FinishArgs &a, hipStream_t stream);
hipError_t launch_denom_flags(const uint2 *counts, uint64_t pairs, uint32_t s, uint32_t *seen, hipStream_t stream);

}  // namespace mg
