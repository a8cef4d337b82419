// cluster.hip — single-linkage clusters of a thresholded all-vs-all, found on the device: the consumer of pass A's ballots
// (finish_mark_kernel) that needs no distance, no record and no edge list.  The reference has no such command; an EDGE is a
// pair that passes the filters of CommandDistance.cpp:409-422, a CLUSTER a connected component, its LABEL its smallest row.
//
// A lock-free union-find over parent[n] (uint32): a link always hangs the LARGER root under the SMALLER index, so
//   (I1) parent[x] <= x at all times, and parent[x] < x for good once x has stopped being a root;
//   (I2) the rows of a tree only ever change by a successful atomicCAS(&parent[hi], hi, lo), which joins two trees whole;
//   (I3) the root of a tree is its smallest row: every other row of it points strictly downwards.
// With (I3) the result does not depend on the order edges are met in: whatever the schedule, a component ends as one tree
// whose root is the component's smallest row.
//
// Every access to parent[] inside the union launch is an agent-scope atomic (relaxed loads that bypass the CU's L1, atomicMin,
// atomicCAS), never a plain load or store.  Even so a load may return a value that another workgroup has since replaced, and
// that is harmless:
//   * a stale parent is a FORMER parent; by (I2) a former parent (or grandparent) of x is still in x's tree, and by (I1) it is
//     <= x -- a walk over stale values stays inside the component, moves downwards and ends;
//   * path halving writes with atomicMin(&parent[x], g), g such a former grandparent < x: it keeps (I1), moves no row out of its
//     tree, and can never turn a row back into a root or undo a link;
//   * two walks that end at the same row prove the edge redundant whatever was stale on the way (same tree, (I2));
//   * only the CAS decides a link: it succeeds only while `hi` still IS a root (parent[hi] == hi as the memory has it), and on
//     failure hands back the value that beat it, from which the walk goes on.  `lo` may have stopped being a root meanwhile:
//     hi's tree then hangs under a row inside lo's tree, which is the same union.
// Labels are read in a LATER launch (cl_label_kernel): the kernel boundary makes every link visible, its walks end at the true
// roots.
// cl_load, cl_find and cl_unite stand in cluster_internal.h: cluster_forest.hip unites with the same ones.
#include "cluster_internal.h"

namespace mg {

constexpr int CL_NT = 256;

__global__ __launch_bounds__(CL_NT) void cl_init_kernel(uint32_t *parent, uint32_t n)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) parent[i] = i;
}

// An earlier partition as the start: seed[i] <= i (checked by the host), so (I1) holds before the first union, every seeded tree
// is one of (I2)'s whole trees -- a row under its root, the root its smallest row (I3) -- and nothing above has to know that the
// links were not made by a CAS of this call.
__global__ __launch_bounds__(CL_NT) void cl_seed_kernel(uint32_t *parent, const uint32_t *seed, uint32_t n_old, uint32_t n)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) parent[i] = i < n_old ? seed[i] : i;
}

// Pass A's ballots word by word: word w holds pairs [64 w, 64 w + 64) -- finish_mark_kernel's segment / wave / word layout
// ((seg * 4 + wave) * 16 + it) is exactly idx / 64 -- and bits behind a.pairs are zero.  A wave loads 64 words at a time (a word
// that is zero costs that load and nothing else), then takes the words that are not zero one after the other, a lane per bit.
// The grid is sized by the device (launch_cluster_union), not by the pairs.  sp: the job's pairs in parent[]'s index space -- the
// bounds are the job's own, before the bases.
__global__ __launch_bounds__(CL_NT) void cl_union_kernel(FinishArgs a, uint32_t *parent, PairSpace sp)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t words = (a.pairs + 63) / 64;
    const uint64_t nwaves = (uint64_t)gridDim.x * (CL_NT / 64);
    for (uint64_t w0 = ((uint64_t)blockIdx.x * (CL_NT / 64) + (threadIdx.x >> 6)) * 64; w0 < words; w0 += nwaves * 64) {
        const unsigned long long mine = w0 + lane < words ? a.masks[w0 + lane] : 0ull;
        unsigned long long nz = __ballot(mine != 0);
        while (nz) {                                           // (wave-uniform)
            const uint32_t j = (uint32_t)__builtin_ctzll(nz);
            nz &= nz - 1;
            const unsigned long long m = __shfl(mine, j);
            const uint64_t idx = (w0 + j) * 64 + lane;
            if (((m >> lane) & 1) && idx < a.pairs) {
                uint64_t row, col;
                pair_rc(a, idx, row, col);
                if (row < sp.rows && col < sp.cols) cl_unite(parent, sp.row_base + (uint32_t)row, sp.col_base + (uint32_t)col);
            }
        }
    }
}

__global__ __launch_bounds__(CL_NT) void cl_label_kernel(uint32_t *parent, uint32_t n, uint32_t *label, unsigned long long *n_roots)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t roots = 0;
    for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {   // (wave-uniform: the ballot)
        const uint32_t i = i0 + lane;
        uint32_t r = 0xFFFFFFFFu;
        if (i < n) {
            r = cl_find(parent, i);
            label[i] = r;
        }
        roots += (uint32_t)__popcll(__ballot(r == i));
    }
    if (lane == 0 && roots) atomicAdd(n_roots, (unsigned long long)roots);
}

static uint32_t cl_blocks(uint64_t items_per_thread_1, uint32_t cap)
{
    const uint64_t b = (items_per_thread_1 + CL_NT - 1) / CL_NT;
    return (uint32_t)(b < 1 ? 1 : b > cap ? cap : b);
}

hipError_t launch_cluster_init(uint32_t *parent, uint32_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(cl_init_kernel, dim3(cl_blocks(n, 2048)), dim3(CL_NT), 0, stream, parent, n);
    return hipGetLastError();
}

hipError_t launch_cluster_seed(uint32_t *parent, const uint32_t *seed, uint32_t n_old, uint32_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(cl_seed_kernel, dim3(cl_blocks(n, 2048)), dim3(CL_NT), 0, stream, parent, seed, n_old, n);
    return hipGetLastError();
}

hipError_t launch_cluster_union(const FinishArgs &a, uint32_t *parent, const PairSpace &sp, hipStream_t stream)
{
    if (a.pairs == 0 || sp.rows == 0 || sp.cols == 0) return hipSuccess;
    // a work-item per mask word up to 2048 workgroups (8 per CU of an MI355X): beyond that the waves stride
    hipLaunchKernelGGL(cl_union_kernel, dim3(cl_blocks((a.pairs + 63) / 64, 2048)), dim3(CL_NT), 0, stream, a, parent, sp);
    return hipGetLastError();
}

hipError_t launch_cluster_union(const FinishArgs &a, uint32_t *parent, uint32_t n, hipStream_t stream)
{
    return launch_cluster_union(a, parent, PairSpace{n, n, 0u, 0u}, stream);
}

hipError_t launch_cluster_label(uint32_t *parent, uint32_t n, uint32_t *label, unsigned long long *n_roots, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(n_roots, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(cl_label_kernel, dim3(cl_blocks(n, 2048)), dim3(CL_NT), 0, stream, parent, n, label, n_roots);
    return hipGetLastError();
}

}  // namespace mg
