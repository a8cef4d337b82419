// within_internal.h — launch interface between host_within.cpp and within.hip (`mash within`: containment of queries in references).
#pragma once
#ifdef MG_HIP_EMU                    // tools/hipemu: the kernels on host fibers (tests/test_within_emu.py)
#include "hipemu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

namespace mg {

constexpr uint32_t WITHIN_NT = 256;            // work-items per workgroup of every pass; the count pass gives a wave to a pair

// A block of the query-major matrix: pair idx is {query first_q + idx / nref, reference idx % nref}.  Row r of a table is
// hashes[r * s .. r * s + min(nhash[r], s)), ascending and distinct; what lies behind it (MG_HASH_PAD) is never read as a hash.
struct WithinArgs {
    const uint64_t *ref, *qry;
    const uint32_t *ref_n, *qry_n;
    uint64_t ref_s, qry_s;             // row strides = sketch sizes; they may differ, either way round
    uint64_t nref, first_q, pairs;
    unsigned long long *ref_last;      // [nref] a reference's largest hash (launch_within_last; unspecified for an empty row)
    uint32_t j_min;                    // a query or a reference of fewer hashes gets j = 0 without a search; 0: none does
    uint2 *counts;                     // [pairs] {common, j}: the j pass writes {0, j}, the count pass the first field
    uint4 *edges;                      // list form of the count pass: {query, reference, common, j}, the third field written
    uint64_t nedges;
};

// ref_last[r] for every reference (once per call: the j pass reads it per pair)
hipError_t launch_within_last(const WithinArgs &a, hipStream_t stream);
// counts[idx] = {0, j}, j = min(|R|, |Q|, #{q in Q : q <= max(R)})
hipError_t launch_within_j(const WithinArgs &a, hipStream_t stream);
// counts[idx].x = #(Q[0 .. j) ∩ R) for every pair of the block
hipError_t launch_within_count(const WithinArgs &a, hipStream_t stream);
// the same for edges[0 .. nedges): the survivors of a threshold, wherever they lie in the matrix
hipError_t launch_within_count_list(const WithinArgs &a, hipStream_t stream);

}  // namespace mg
