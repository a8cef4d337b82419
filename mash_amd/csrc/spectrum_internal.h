// spectrum_internal.h — launch interface between host_spectrum.cpp and spectrum.hip (the distance spectrum of a job: how many of
// its pairs have each {numer, denom}).
#pragma once
#include "cluster_internal.h"         // PairSpace, CF_NONE, cf_load (under MG_HIP_EMU it brings tools/hipemu: tests/test_spectrum_emu.py)
#include <stdint.h>

namespace mg {

// The bins of one call; they live across its pieces.  A key {numer, denom} has one of two homes:
//   denom == s      : full[numer], s + 1 64-bit counts;
//   any other denom : the open-addressing table keys[slots] / vals[slots] (slots a power of two), key = numer << 32 | denom (never
//                     CF_NONE: denom <= s < 2^32 - 1), CF_NONE an empty slot; an entry that finds neither its key nor an empty slot
//                     in `slots` probes sets *overflow and is NOT counted: the host enlarges the table and runs the call again.
// The caller clears full[] and vals[] to 0, keys[] to CF_NONE and *overflow to 0 before the first piece.
struct SpectrumBins {
    unsigned long long *full, *keys, *vals;
    uint64_t slots;
    uint32_t *overflow;
    uint32_t s;
};

// LDS bins are used where 4 (s + 1) bytes fit in 64 KiB
constexpr uint32_t SPECTRUM_LDS_MAX_S = 16383;

// Every set bit of a.masks (finish_mark_kernel's ballots: bit idx = pair idx of a.counts) whose {row, col} (pair_rc) lies inside sp
// adds 1 to the bin of a.counts[idx].  Bits that are clear, behind a.pairs or outside sp add nothing; counts beside clear bits are
// not read.  plain: one atomic per entry straight to memory; otherwise lanes of a wave with the same key combine first and
// denom == s goes through 32-bit LDS bins where they fit.  Both leave the same bits.
hipError_t launch_spectrum_marked(const FinishArgs &a, const PairSpace &sp, const SpectrumBins &b, hipStream_t stream, bool plain = false);
// Every one of the `pairs` counts adds 1 to its bin (the matrix with the filters off).  Not plain: {0, s} is counted in a register
// and leaves as one atomic per wave.
hipError_t launch_spectrum_all(const uint2 *counts, uint64_t pairs, const SpectrumBins &b, hipStream_t stream, bool plain = false);
// The list form: entry e of cnt[K] adds 1 to its bin, and 1 to rule[min(s, min(nh_row[rc[e].x], s) + min(nh_col[rc[e].y], s))]
// (rule[s + 1], 64-bit, cleared by the caller); *listed_zero counts the entries with numer == 0.
hipError_t launch_spectrum_list(const uint2 *cnt, const uint2 *rc, uint64_t K, const uint32_t *nh_row, const uint32_t *nh_col, const SpectrumBins &b,
                                unsigned long long *rule, unsigned long long *listed_zero, hipStream_t stream, bool plain = false);

}  // namespace mg
