// cluster_medoid.hip — the medoid of every single-linkage cluster (`mash cluster -M`), scored while cl_union_kernel's walk over pass A's
// ballots is under way: the pairs' {numer, denom} stand beside the ballots then, and every edge lies inside one cluster, so a row's
// centrality is a sum over its own edges -- no edge list, no second compare, no labels.
//
//   weight(e) = floor(numer * 2^32 / max(denom, 1))              (medoid_weight, forest_key.h: <= 2^32, 0/0 counts as 0/1)
//   score[i]  = the sum of weight(e) over the edges with an end at i    (64-bit; fewer than 2^31 rows: below 2^63)
//   medoid[i] = among the rows of i's cluster the one with the largest score, equal scores to the smallest row
//
// Everything is an integer and every combining operation commutes -- 64-bit add, max, min --, so score[] and medoid[] are functions
// of the edge set and its counts alone: not of the route (list or matrix blocks), the blocking, the schedule, or whether the
// weights of a word were combined in the wave before they reached memory.
//
// The union launch (cm_union_kernel) is cl_union_kernel with two additions per set bit: the pair's counts are read and its weight is
// added to both ends.  In the flat triangle the 64 pairs of a word lie in one or two rows once row >= 64, and a candidate list is in
// row order, so the row side would send up to 64 atomics to one address: the lanes of a word that hold the SAME row combine their
// weights in the wave (ballot, shuffle) and one atomic per distinct row leaves it.  Which lanes hold the same row is found by
// comparing rows, never assumed from their order: a list may name rows in any order and the same row in lanes far apart.  After
// CM_ROUNDS distinct rows the lanes still waiting add for themselves (the first words of a triangle span up to eleven rows, a sparse
// list up to 64), and in a word with fewer than CM_MIN_EDGES edges every lane does.  The column side is one atomic per edge: the columns of a row's pairs are all different.
// The plain variant (two atomics per edge) is kept for the A/B of tools/cluster_medoid_bench.py: context option MASHGPU_MEDOID_PLAIN.
//
// The pick (launch_medoid_pick) runs behind launch_cluster_label, three launches on the one stream:
//   best[label[i]] = max score[i];   pick[label[i]] = min i among score[i] == best[label[i]];   medoid[i] = pick[label[i]].
// The cluster's smallest row (its label) has a score <= best, some row has exactly best, so pick[] of every label is written.
#include "cluster_internal.h"
#include "forest_key.h"

namespace mg {

constexpr int CM_NT = 256;
constexpr int CM_ROUNDS = 4;          // distinct rows of a word whose lanes are combined; the rest add for themselves
constexpr int CM_MIN_EDGES = 8;       // edges in a word below which every lane adds for itself

template <bool PLAIN>
__global__ __launch_bounds__(CM_NT) void cm_union_kernel(FinishArgs a, uint32_t *parent, unsigned long long *score, PairSpace sp)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t words = (a.pairs + 63) / 64;
    const uint64_t nwaves = (uint64_t)gridDim.x * (CM_NT / 64);
    for (uint64_t w0 = ((uint64_t)blockIdx.x * (CM_NT / 64) + (threadIdx.x >> 6)) * 64; w0 < words; w0 += nwaves * 64) {
        const unsigned long long mine = w0 + lane < words ? a.masks[w0 + lane] : 0ull;
        unsigned long long nz = __ballot(mine != 0);
        while (nz) {                                           // (wave-uniform)
            const uint32_t j = (uint32_t)__builtin_ctzll(nz);
            nz &= nz - 1;
            const unsigned long long m = __shfl(mine, j);
            const uint64_t idx = (w0 + j) * 64 + lane;
            bool in = false;                                   // this lane holds an edge of the job's pair space
            uint32_t row = 0, col = 0;
            unsigned long long wt = 0;
            if (((m >> lane) & 1) && idx < a.pairs) {
                uint64_t r, c;
                pair_rc(a, idx, r, c);
                if (r < sp.rows && c < sp.cols) {
                    in = true;
                    row = sp.row_base + (uint32_t)r;
                    col = sp.col_base + (uint32_t)c;
                    cl_unite(parent, row, col);
                    const uint2 cnt = a.counts[idx];
                    wt = medoid_weight(cnt.x, cnt.y);
                }
            }
            if (PLAIN) {
                if (in) {
                    atomicAdd(score + row, wt);
                    atomicAdd(score + col, wt);
                }
                continue;
            }
            if (in) atomicAdd(score + col, wt);
            unsigned long long todo = __ballot(in);            // (from here on wave-uniform again: every lane takes part in the shuffles)
            const int rounds = __popcll(todo) >= CM_MIN_EDGES ? CM_ROUNDS : 0;       // a word with a few edges: nothing to combine
            for (int round = 0; todo && round < rounds; round++) {
                const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
                const uint32_t r = __shfl(row, lead);
                const bool same = in && row == r;              // (a row leaves `todo` whole: no later leader holds it again)
                const unsigned long long grp = __ballot(same);
                unsigned long long sum = same ? wt : 0ull;
                if (grp & (grp - 1)) {                         // two lanes or more: every lane ends with the group's sum (< 2^38)
                    for (uint32_t o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
                }
                if (lane == lead) atomicAdd(score + r, sum);
                todo &= ~grp;
            }
            if ((todo >> lane) & 1) atomicAdd(score + row, wt);
        }
    }
}

__global__ __launch_bounds__(CM_NT) void cm_best_kernel(const uint32_t *label, const unsigned long long *score, uint32_t n, unsigned long long *best)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const unsigned long long s = score[i];
        if (s) atomicMax(best + label[i], s);                  // (best[] starts at 0)
    }
}

__global__ __launch_bounds__(CM_NT) void cm_pick_kernel(const uint32_t *label, const unsigned long long *score, uint32_t n,
                                                        const unsigned long long *best, uint32_t *pick)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t l = label[i];
        if (score[i] == best[l]) atomicMin(pick + l, i);       // (best: cm_best_kernel's, an earlier launch; pick[] starts at ~0)
    }
}

__global__ __launch_bounds__(CM_NT) void cm_medoid_kernel(const uint32_t *label, const uint32_t *pick, uint32_t n, uint32_t *medoid)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) medoid[i] = pick[label[i]];
}

static uint32_t cm_blocks(uint64_t items_per_thread_1, uint32_t cap)
{
    const uint64_t b = (items_per_thread_1 + CM_NT - 1) / CM_NT;
    return (uint32_t)(b < 1 ? 1 : b > cap ? cap : b);
}

hipError_t launch_medoid_union(const FinishArgs &a, uint32_t *parent, unsigned long long *score, const PairSpace &sp, hipStream_t stream, bool plain)
{
    if (a.pairs == 0 || sp.rows == 0 || sp.cols == 0) return hipSuccess;
    // launch_cluster_union's grid: a work-item per mask word up to 2048 workgroups, beyond that the waves stride
    const dim3 grid(cm_blocks((a.pairs + 63) / 64, 2048));
    if (plain) hipLaunchKernelGGL(cm_union_kernel<true>, grid, dim3(CM_NT), 0, stream, a, parent, score, sp);
    else hipLaunchKernelGGL(cm_union_kernel<false>, grid, dim3(CM_NT), 0, stream, a, parent, score, sp);
    return hipGetLastError();
}

hipError_t launch_medoid_pick(const uint32_t *label, const unsigned long long *score, uint32_t n, unsigned long long *best, uint32_t *pick,
                              uint32_t *medoid, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(best, 0, (size_t)n * sizeof(unsigned long long), stream);
    if (e == hipSuccess) e = hipMemsetAsync(pick, 0xFF, (size_t)n * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const dim3 grid(cm_blocks(n, 2048));
    hipLaunchKernelGGL(cm_best_kernel, grid, dim3(CM_NT), 0, stream, label, score, n, best);
    hipLaunchKernelGGL(cm_pick_kernel, grid, dim3(CM_NT), 0, stream, label, score, n, (const unsigned long long *)best, pick);
    hipLaunchKernelGGL(cm_medoid_kernel, grid, dim3(CM_NT), 0, stream, label, (const uint32_t *)pick, n, medoid);
    return hipGetLastError();
}

}  // namespace mg
