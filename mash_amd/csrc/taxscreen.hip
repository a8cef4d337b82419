// taxscreen.hip — gfx950 kernels for the taxonomy side of `mash taxscreen`
// (CommandTaxScreen.cpp:411-432: the LCA of the references that hold each database hash, the per-taxon histograms).
//
//   lca   : per slot of the screen's key table, the fold of the lowest common ancestor over the nodes of the rows in
//           the slot's run of the rows-by-slot index.  The reference builds one unordered_set per (hash, reference)
//           step (taxdb.hpp:162-196); here a taxonomy is two dense arrays, parent[] and depth[], and an LCA is a
//           depth-aligned walk: dependent 4-byte loads into arrays that stay in the Infinity Cache.
//           Most runs are one row long, a few (a hash shared by a whole clade) thousands: runs of up to
//           TAX_LONG_RUN rows are folded by one work-item, longer ones are listed and folded by a workgroup each.
//   hist  : counts[node] += 1 per hash.  Most hashes of a real database land on a handful of high nodes, so equal
//           nodes are summed inside the wave first, then in a small LDS table per workgroup; global adds are one per
//           distinct node per workgroup (or per wave, for nodes that lose their LDS line to another).
// All integer work, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "taxscreen_internal.h"

namespace mg {

// LCA of two slot_node values.  TAX_NONE is the identity (getLowestCommonAncestor(a, 0) == a), TAX_DISJOINT absorbs;
// so the fold is associative and commutative and may be split over lanes and waves in any order.
__device__ __forceinline__ uint32_t tax_lca(uint32_t a, uint32_t b, const uint32_t *__restrict__ parent, const uint32_t *__restrict__ depth)
{
    if (a == TAX_NONE || a == b) return b;
    if (b == TAX_NONE) return a;
    if (a == TAX_DISJOINT || b == TAX_DISJOINT) return TAX_DISJOINT;
    uint32_t da = depth[a], db = depth[b];
    while (da > db) { a = parent[a]; da--; }
    while (db > da) { b = parent[b]; db--; }
    while (a != b) {
        if (da == 0) return TAX_DISJOINT;                  // two roots
        a = parent[a];
        b = parent[b];
        da--;
    }
    return a;
}

__global__ __launch_bounds__(256) void tax_lca_short_kernel(uint64_t slots, const uint32_t *__restrict__ slot_end, const uint32_t *__restrict__ ent,
                                                            const uint32_t *__restrict__ row_node, const uint32_t *__restrict__ parent,
                                                            const uint32_t *__restrict__ depth, uint32_t *__restrict__ slot_node,
                                                            uint32_t *__restrict__ long_list, unsigned long long *n_long, uint64_t long_cap)
{
    const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= slots) return;
    const uint32_t b = slot ? slot_end[slot - 1] : 0, e = slot_end[slot];
    if (e == b) { slot_node[slot] = TAX_EMPTY; return; }
    if (e - b > TAX_LONG_RUN) {
        const unsigned long long at = atomicAdd(n_long, 1ull);
        if (at < long_cap) long_list[at] = (uint32_t)slot;  // (long_cap = postings / TAX_LONG_RUN + 1: never exceeded)
        return;
    }
    uint32_t acc = TAX_NONE;
    for (uint32_t q = b; q < e; q++) acc = tax_lca(acc, row_node[ent[q]], parent, depth);
    slot_node[slot] = acc;
}

__global__ __launch_bounds__(256) void tax_lca_long_kernel(const uint32_t *__restrict__ slot_end, const uint32_t *__restrict__ ent,
                                                           const uint32_t *__restrict__ row_node, const uint32_t *__restrict__ parent,
                                                           const uint32_t *__restrict__ depth, uint32_t *__restrict__ slot_node,
                                                           const uint32_t *__restrict__ long_list, const unsigned long long *n_long, uint64_t long_cap)
{
    __shared__ uint32_t part[4];
    unsigned long long n = *n_long;
    if (n > long_cap) n = long_cap;
    for (unsigned long long li = blockIdx.x; li < n; li += gridDim.x) {            // (uniform per workgroup)
        const uint32_t slot = long_list[li];
        const uint32_t b = slot ? slot_end[slot - 1] : 0, e = slot_end[slot];
        uint32_t acc = TAX_NONE;
        for (uint32_t q = b + threadIdx.x; q < e; q += 256) acc = tax_lca(acc, row_node[ent[q]], parent, depth);
        for (int off = 32; off > 0; off >>= 1) acc = tax_lca(acc, (uint32_t)__shfl_xor((int)acc, off), parent, depth);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; w++) acc = tax_lca(acc, part[w], parent, depth);
            slot_node[slot] = acc;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ uint32_t tax_bucket(uint32_t node, uint32_t n_nodes)
{
    return node < n_nodes ? node : n_nodes + (node == TAX_NONE ? 1u : 0u);
}

constexpr uint32_t TAX_LDS_LINES = 512;

__global__ __launch_bounds__(256) void tax_hist_kernel(const uint32_t *__restrict__ slot_node, uint64_t n, const uint32_t *__restrict__ touched,
                                                       const uint32_t *__restrict__ obs, uint32_t n_nodes, uint32_t *counts)
{
    // direct-mapped: a line belongs to the first bucket that claims it; others with the same index go to HBM per wave
    __shared__ uint32_t tag[TAX_LDS_LINES], cnt[TAX_LDS_LINES];
    for (uint32_t h = threadIdx.x; h < TAX_LDS_LINES; h += 256) { tag[h] = 0xFFFFFFFFu; cnt[h] = 0; }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256; i0 < n; i0 += stride) {          // (uniform per workgroup: ballots see whole waves)
        const uint64_t i = i0 + threadIdx.x;
        uint32_t bucket = 0;
        bool todo = false;
        if (i < n) {
            const uint64_t slot = touched ? touched[i] : i;
            const uint32_t node = slot_node[slot];
            if (node != TAX_EMPTY && (!touched || obs[slot] >= 1)) { todo = true; bucket = tax_bucket(node, n_nodes); }
        }
        for (;;) {                                         // one round per distinct bucket of the wave
            const unsigned long long left = __ballot(todo);
            if (left == 0) break;
            const int leader = __ffsll((long long)left) - 1;
            const uint32_t v = (uint32_t)__shfl((int)bucket, leader);
            const bool same = todo && bucket == v;
            const uint32_t c = (uint32_t)__popcll(__ballot(same));
            if ((int)lane == leader) {
                const uint32_t h = v & (TAX_LDS_LINES - 1);
                const uint32_t old = atomicCAS(&tag[h], 0xFFFFFFFFu, v);
                if (old == 0xFFFFFFFFu || old == v) atomicAdd(&cnt[h], c);
                else atomicAdd(&counts[v], c);
            }
            if (same) todo = false;
        }
    }
    __syncthreads();
    for (uint32_t h = threadIdx.x; h < TAX_LDS_LINES; h += 256)
        if (cnt[h]) atomicAdd(&counts[tag[h]], cnt[h]);
}

__global__ void tax_clear_kernel(const uint32_t *__restrict__ slot_node, const uint32_t *__restrict__ touched, uint64_t nt, uint32_t n_nodes,
                                 uint32_t *counts)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const uint32_t node = slot_node[touched[t]];
    if (node != TAX_EMPTY) counts[tax_bucket(node, n_nodes)] = 0;
}

__global__ void tax_gather_kernel(const uint32_t *__restrict__ counts, const uint32_t *__restrict__ list, uint64_t m, uint32_t *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) out[i] = counts[list[i]];
}

hipError_t launch_tax_lca(uint64_t slots, const uint32_t *slot_end, const uint32_t *ent, const uint32_t *row_node, const uint32_t *parent,
                          const uint32_t *depth, uint32_t *slot_node, uint32_t *long_list, unsigned long long *n_long, uint64_t long_cap,
                          hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(n_long, 0, 8, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tax_lca_short_kernel, dim3((uint32_t)((slots + 255) / 256)), dim3(256), 0, stream, slots, slot_end, ent, row_node, parent,
                       depth, slot_node, long_list, n_long, long_cap);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (the number of long runs stays on the device: a fixed grid strides over the list)
    hipLaunchKernelGGL(tax_lca_long_kernel, dim3(2048), dim3(256), 0, stream, slot_end, ent, row_node, parent, depth, slot_node, long_list,
                       n_long, long_cap);
    return hipGetLastError();
}

hipError_t launch_tax_hist(const uint32_t *slot_node, uint64_t n, const uint32_t *touched, const uint32_t *obs, uint32_t n_nodes,
                           uint32_t *counts, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    // (at least 16 rounds per workgroup where there is that much work, so that the LDS table earns its flush)
    const uint64_t blocks = std::min<uint64_t>(4096, (n + 256 * 16 - 1) / (256 * 16));
    hipLaunchKernelGGL(tax_hist_kernel, dim3((uint32_t)std::max<uint64_t>(blocks, 1)), dim3(256), 0, stream, slot_node, n, touched, obs, n_nodes, counts);
    return hipGetLastError();
}

hipError_t launch_tax_clear(const uint32_t *slot_node, const uint32_t *touched, uint64_t nt, uint32_t n_nodes, uint32_t *counts, hipStream_t stream)
{
    if (nt == 0) return hipSuccess;
    hipLaunchKernelGGL(tax_clear_kernel, dim3((uint32_t)((nt + 255) / 256)), dim3(256), 0, stream, slot_node, touched, nt, n_nodes, counts);
    return hipGetLastError();
}

hipError_t launch_tax_gather(const uint32_t *counts, const uint32_t *list, uint64_t m, uint32_t *out, hipStream_t stream)
{
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(tax_gather_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, stream, counts, list, m, out);
    return hipGetLastError();
}

}  // namespace mg
