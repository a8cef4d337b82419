// within.hip — `mash within`: how much of a query's sketch lies inside a reference's (containSketches, CommandContain.cpp:231-263).
//
// The reference walks both ascending lists with two pointers, i over R and j over Q, counts the equal steps in `common`, and
// stops when j reaches min(|R|, |Q|) or i reaches |R|; the pair's score is common / j, its error bound 1 / sqrt(j).  The walk
// has a closed form, in integers:
//   c      = #{q in Q : q <= max(R)}       R is exhausted exactly when the walk has passed every q <= max(R): a smaller q is
//                                          stepped over, one equal to max(R) is consumed by the equal step (hence <=)
//   j      = min(|R|, |Q|, c)              0 if either list is empty
//   common = #(Q[0 .. j) ∩ R)              the walk sees every element of Q[0 .. j) against all of R below it
// so the pairs need no serial walk and the two numbers come from two passes:
//   j pass      a work-item per pair: one binary search of max(R) in the query's row.  A threshold on the error bound is a
//               threshold j >= j_min (the host converts it), and a row of fewer than j_min hashes -- query or reference --
//               cannot reach it: those pairs get j = 0 without a search.
//   count pass  a wave per pair -- every pair of a block, or only the survivors of the threshold, compacted in between by
//               compare.hip's filter passes --: the lanes stride Q[0 .. j), each looks its hash up in R by binary search, a
//               ballot and a popcount add the hits.  No row is staged in LDS, so no sketch size takes another path.
// A row is its first min(nhash, s) hashes and nothing else: every search is bounded by that count, never by the padding value
// (two short rows carry the same padding, and a real 64-bit hash may equal it).  No float takes part.
//
// Compiles for tools/hipemu too (MG_HIP_EMU, tests/test_within_emu.py): wave operations sit in wave-uniform control flow.
#include "within_internal.h"

namespace mg {

__device__ __forceinline__ uint32_t within_row_n(const uint32_t *nhash, uint64_t row, uint64_t s)
{
    const uint32_t n = nhash[row];
    return n < s ? n : (uint32_t)s;
}

// the number of row[0 .. n) that are <= key (upper bound)
__device__ __forceinline__ uint32_t within_rank_le(const uint64_t *row, uint32_t n, uint64_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (row[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// whether key is one of row[0 .. n)
__device__ __forceinline__ bool within_member(const uint64_t *row, uint32_t n, uint64_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (row[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && row[lo] == key;
}

__global__ __launch_bounds__(WITHIN_NT) void within_last_kernel(WithinArgs a)
{
    const uint64_t r = (uint64_t)blockIdx.x * WITHIN_NT + threadIdx.x;
    if (r >= a.nref) return;
    const uint32_t n = within_row_n(a.ref_n, r, a.ref_s);
    a.ref_last[r] = n ? a.ref[r * a.ref_s + n - 1u] : 0ull;
}

__global__ __launch_bounds__(WITHIN_NT) void within_j_kernel(WithinArgs a)
{
    const uint64_t stride = (uint64_t)gridDim.x * WITHIN_NT;
    for (uint64_t idx = (uint64_t)blockIdx.x * WITHIN_NT + threadIdx.x; idx < a.pairs; idx += stride) {
        const uint64_t q = a.first_q + idx / a.nref, r = idx % a.nref;
        const uint32_t nq = within_row_n(a.qry_n, q, a.qry_s), nr = within_row_n(a.ref_n, r, a.ref_s);
        uint32_t j = 0;
        if (nq != 0 && nr != 0 && nq >= a.j_min && nr >= a.j_min) {
            j = within_rank_le(a.qry + q * a.qry_s, nq, a.ref_last[r]);
            j = j < nr ? j : nr;                                          // (rank <= nq already)
        }
        a.counts[idx] = make_uint2(0u, j);
    }
}

// the wave's count of Q[0 .. j) in R[0 .. nr); uniform arguments, every lane returns the sum
__device__ __forceinline__ uint32_t within_wave_common(const uint64_t *qrow, uint32_t j, const uint64_t *rrow, uint32_t nr, uint32_t lane)
{
    uint32_t common = 0;
    for (uint32_t t0 = 0; t0 < j; t0 += 64u) {                            // (uniform)
        const uint32_t t = t0 + lane;
        const bool hit = t < j && within_member(rrow, nr, qrow[t]);
        common += (uint32_t)__popcll(__ballot(hit));
    }
    return common;
}

template <bool LIST>
__global__ __launch_bounds__(WITHIN_NT) void within_count_kernel(WithinArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t items = LIST ? a.nedges : a.pairs, waves = (uint64_t)gridDim.x * (WITHIN_NT / 64u);
    for (uint64_t it = (uint64_t)blockIdx.x * (WITHIN_NT / 64u) + (threadIdx.x >> 6); it < items; it += waves) {      // (uniform in the wave)
        uint64_t q, r;
        uint32_t j;
        if (LIST) {
            const uint4 e = a.edges[it];
            q = e.x; r = e.y; j = e.w;
        } else {
            q = a.first_q + it / a.nref; r = it % a.nref; j = a.counts[it].y;
        }
        if (j == 0) continue;                                             // (the j pass left {0, 0})
        const uint32_t nq = within_row_n(a.qry_n, q, a.qry_s), nr = within_row_n(a.ref_n, r, a.ref_s);
        if (j > nq) j = nq;                                               // (never: j <= min(nq, nr); keeps every read inside the row)
        const uint32_t common = within_wave_common(a.qry + q * a.qry_s, j, a.ref + r * a.ref_s, nr, lane);
        if (lane == 0) {
            if (LIST) a.edges[it].z = common; else a.counts[it].x = common;
        }
    }
}

static uint32_t within_blocks(uint64_t items, uint64_t per_block)
{
    const uint64_t blocks = (items + per_block - 1u) / per_block;
    return (uint32_t)(blocks < 262144u ? blocks : 262144u);
}

hipError_t launch_within_last(const WithinArgs &a, hipStream_t stream)
{
    if (a.nref == 0) return hipSuccess;
    if (a.nref > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(within_last_kernel, dim3((uint32_t)((a.nref + WITHIN_NT - 1u) / WITHIN_NT)), dim3(WITHIN_NT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_within_j(const WithinArgs &a, hipStream_t stream)
{
    if (a.pairs == 0) return hipSuccess;
    if (a.nref == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(within_j_kernel, dim3(within_blocks(a.pairs, WITHIN_NT)), dim3(WITHIN_NT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_within_count(const WithinArgs &a, hipStream_t stream)
{
    if (a.pairs == 0) return hipSuccess;
    if (a.nref == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(within_count_kernel<false>, dim3(within_blocks(a.pairs, WITHIN_NT / 64u)), dim3(WITHIN_NT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_within_count_list(const WithinArgs &a, hipStream_t stream)
{
    if (a.nedges == 0) return hipSuccess;
    hipLaunchKernelGGL(within_count_kernel<true>, dim3(within_blocks(a.nedges, WITHIN_NT / 64u)), dim3(WITHIN_NT), 0, stream, a);
    return hipGetLastError();
}

}  // namespace mg
