// screen_finish_internal.h — launch interface between host_screen.cpp and screen_finish.hip (the tail of `mash screen`).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mg {

struct ScreenResult {          // = mg_screen_result (include/mashgpu.h)
    uint32_t row, shared, denom, median;
    double identity, p_value;
};

constexpr uint32_t SRF_LONG_RUN = 16;      // holder runs above this are walked by the whole wave, one after the other
constexpr uint32_t SRF_LONG_ROW = 4096;    // rows with more counts than this get a workgroup for their selection, not a wave
constexpr uint32_t SRF_NO_LUT = 0xFFFFFFFFu;

// device counters of one call (ScreenFinish::ctr): [0] hits (run entries of the observed slots), [1] touched rows,
// [2] rows left to the workgroup selection, [3] rows written
enum { SRF_CTR_HITS = 0, SRF_CTR_ROWS = 1, SRF_CTR_LONG = 2, SRF_CTR_OUT = 3, SRF_CTRS = 4 };

struct ScreenFinishArgs {
    // what the mixture touched and the rows-by-slot index (mg_screen)
    const uint32_t *touched;
    uint64_t nt;
    const uint32_t *obs, *slot_end, *ent;
    // the database's rows
    const uint32_t *nhash;
    const uint64_t *lengths;               // nullptr unless `winner`
    uint64_t n;
    uint32_t s;
    // identity table of the host's libm: lut[lut_start[denom] + x] = mg_identity(x, denom, k)
    const double *lut;
    const uint32_t *lut_start;
    // per row, zero between calls: shared (every holder), shared_w (winners only), fill (scatter cursor)
    uint32_t *shared, *shared_w, *fill;
    uint32_t *row_off, *median;            // per row, written before they are read
    double *score;                         // per touched row (winner)
    uint32_t *rows;                        // touched rows, in no order [n]
    uint32_t *long_rows;                   // [n]
    uint32_t *winner_row;                  // per touched slot (winner) [nt]
    uint32_t *vals;                        // observation counts grouped by row [hits, or nt with winner]
    unsigned long long *ctr;               // [SRF_CTRS]
    // rows out
    double r, min_identity, max_p;         // r = set_size / kmer_space
    uint32_t all_rows;                     // min_identity < 0: rows with shared == 0 are candidates too
    unsigned long long *masks;
    uint32_t *seg_count;
    unsigned long long *seg_off;
    ScreenResult *out;
    uint64_t out_cap;
};

uint64_t screen_finish_segments(uint64_t n);
uint64_t screen_finish_mask_words(uint64_t n);
size_t screen_finish_scan_temp_bytes(uint64_t n);

// shared[row] over every holder of every observed slot, the touched-rows list, the hit total
hipError_t launch_srf_shared(const ScreenFinishArgs &a, hipStream_t stream);
// score[row] of the first nrows touched rows, then per observed slot its winning holder and shared_w
hipError_t launch_srf_winners(const ScreenFinishArgs &a, uint64_t nrows, hipStream_t stream);
// row_off = exclusive scan of the rows' counts (shared, or shared_w with winner)
hipError_t launch_srf_offsets(const ScreenFinishArgs &a, bool winner, void *temp, size_t temp_bytes, hipStream_t stream);
// the observation counts into vals [vals_cap], grouped by row
hipError_t launch_srf_scatter(const ScreenFinishArgs &a, bool winner, uint64_t vals_cap, hipStream_t stream);
// median[row] = the count of rank cnt / 2 for the first nrows touched rows
hipError_t launch_srf_medians(const ScreenFinishArgs &a, bool winner, uint64_t nrows, hipStream_t stream);
// filters and ordered compaction: ctr[SRF_CTR_OUT] = rows that pass, the first out_cap of them written in row order
hipError_t launch_srf_rows(const ScreenFinishArgs &a, bool winner, hipStream_t stream);
// per-row state back to zero over the first nrows touched rows
hipError_t launch_srf_clear(const ScreenFinishArgs &a, uint64_t nrows, hipStream_t stream);

}  // namespace mg
