// copy_gate.h -- which entries of a row the copy gate looks at (compare_sparse.hip: sp_row_gate_kernel; host_index.cpp: scan_rows).
//
// Whether a table holds copies of rows at all is asked once per index build, of every row.  The gate's digest is taken over
// at most COPY_GATE_SAMPLES positions of the row, spread evenly over the row's own entry count, the LAST entry among them;
// a row of no more entries than that is taken whole.  Each sampled (value, position) is mixed exactly as the full digest mixes
// it (sp_row_digest_kernel), and the rows' counts are compared beside the digests as before.  Equal rows have equal counts, so the
// same positions are sampled and the digests are equal: the gate never misses a copy.  Rows that differ only where the gate
// does not look are false suspects: find_copies() digests every row in full and compares the suspects value by value, so a
// false suspect costs that second stage and never a result.
// (16 samples gave 13 false suspects among 8 192 sketches of one species, whose rows differ in a handful of values; 32 gave none
//  there nor on clustered and random tables of 10 000 rows.)
#pragma once
#include <stdint.h>

namespace mg {

constexpr uint32_t COPY_GATE_SAMPLES = 32;

constexpr uint32_t copy_gate_samples(uint32_t cnt) { return cnt < COPY_GATE_SAMPLES ? cnt : COPY_GATE_SAMPLES; }

// position of sample k (k < copy_gate_samples(cnt)) in a row of cnt entries: ascending in k, sample 31 of a long row is cnt - 1
constexpr uint32_t copy_gate_position(uint32_t k, uint32_t cnt)
{
    return cnt <= COPY_GATE_SAMPLES ? k : (uint32_t)(((uint64_t)(k + 1u) * cnt) / COPY_GATE_SAMPLES) - 1u;
}

static_assert(copy_gate_position(0, 1000) == 30 && copy_gate_position(1, 1000) == 61 && copy_gate_position(31, 1000) == 999, "evenly spread, the last entry among them");
static_assert(copy_gate_position(0, 33) == 0 && copy_gate_position(31, 33) == 32 && copy_gate_position(5, 7) == 5, "short rows are taken whole");

}  // namespace mg
