// cluster_density.hip — density clusters (DBSCAN) of a thresholded all-vs-all, found on the device: `mash cluster -D <m>`.  The reference
// has no such command; an EDGE is a pair that passes the filters of CommandDistance.cpp:409-422, with its counts numer/denom.
//   deg(i)  : the number of edges with an end at i;
//   CORE    : deg(i) >= m;
//   clusters: the connected components of the cores under the edges whose BOTH ends are cores;
//   BORDER  : not a core, with an edge to a core; it is filed under its nearest core neighbour via(i) -- the larger numer/denom in the
//             order of forest_key.h, equal fractions (also under different denominators) to the core of smaller row;
//   NOISE   : neither; a cluster of its own;
//   label[i]: the smallest row among ALL members of i's final cluster -- a border can precede every core of its cluster.
// The list is cluster_forest.hip's, {hi, lo, numer, denom}, entries with hi == lo skipped.  Everything is queued behind the last append
// (launch_density), each pass a launch of its own over the whole list or over the rows:
//   K1 cd_degree_kernel   per edge: deg[hi] += 1, deg[lo] += 1
//   K2 cd_union_kernel    per edge with both ends core: cl_unite(parent, hi, lo); then cl_label_kernel: label[core] = its cluster's
//                         smallest core, label[i] = i for every other row (nobody linked it)
//   K3 cd_key_kernel      per edge with exactly one core end: atomicMax(&best_key[member], forest_key(numer, denom))
//   K4 cd_pick_kernel     the same edges whose key == best_key[member]: atomicMin(&via[member], core)
//   K5 cd_file_kernel     per row: a border takes label[via]; a row below its label offers itself: atomicMin(&first[label], row)
//   K6 cd_gather_kernel   per row: label = first[label]; the rows with label == row are counted
// Invariants:
//   (D1) deg[] is final when K2 .. K5 read it (earlier launch, plain loads): "core" means the same to every pass.
//   (D2) cl_unite links the larger root under the smaller (cluster.hip, I1 .. I3) and only cores are ever united: a row that is not a
//        core stays its own root, and cl_label_kernel gives it label[i] = i.
//   (D3) The core can be EITHER end of a border's edge; cd_border_edge names member and core whichever way round they stand.  An edge
//        between two rows that are not cores decides nothing, so a border never links two clusters.
//   (D4) best_key[] starts at 0, which IS a key (numer == 0).  K4 looks at edges only: a border has an edge to a core, so its best_key
//        is the maximum over a set that is not empty and the edge that carries it passes K4's test.  via[] starts at the row itself
//        for a core and at CD_NONE, above every row, otherwise; a row that is not a core and still has CD_NONE behind K4 is noise.
//   (D5) K5 writes label[] of borders only and reads label[] of cores only (via is a core): no word is read and written in one launch.
//        first[i] starts at i.  A cluster's smallest member is its smallest core -- label itself -- or a border below it, so only rows
//        below their label offer; first[] of a row that is nobody's label is never read.  K6 reads first[] of an earlier launch.
//   (D6) The key is the fraction's order exactly for denominators below FOREST_DENOM_LIMIT (forest_key.h); the host refuses larger
//        sketch sizes.
// Why no order of execution can change the result: the racing accesses are adds on deg[], cl_unite on parent[] (the partition it leaves
// is that of the edge set: cluster.hip), one atomicMax per word in K3, one atomicMin per word in K4 and K5, each over a fixed set of
// offers.  Add, max and min commute; the relaxed look in front of an atomic only skips an offer that cannot win (cluster_forest.hip, F2).
// K1 in two forms with the same result: plain, two atomics per edge; or the lanes of a wave that hold the same row side by side -- the
// list route appends a row's pairs next to each other -- add their run's length with one atomic.
#include "cluster_internal.h"
#include "forest_key.h"

namespace mg {

constexpr int CD_NT = 256;
constexpr uint32_t CD_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t cd_load(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// deg[row] += the length of the run of lanes that are `on` and hold `row`, added by the run's first lane.  Called by whole waves.
__device__ __forceinline__ void cd_add_runs(uint32_t *deg, bool on, uint32_t row, uint32_t lane)
{
    const uint32_t prev = __shfl_up(row, 1);
    const bool prev_on = __shfl_up((uint32_t)on, 1) != 0;
    const bool head = on && (lane == 0 || !prev_on || prev != row);
    const unsigned long long stop = __ballot(head || !on);      // a run ends in front of the next head or the next lane that is off
    if (head) {
        const unsigned long long behind = lane == 63 ? 0ull : stop >> (lane + 1);
        atomicAdd(deg + row, behind ? (uint32_t)__builtin_ctzll(behind) + 1u : 64u - lane);
    }
}

__global__ __launch_bounds__(CD_NT) void cd_degree_kernel(const uint4 *edges, unsigned long long m, uint32_t *deg, int plain)
{
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e0 = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); e0 < m; e0 += stride) {   // (wave-uniform)
        const unsigned long long e = e0 + lane;
        const uint2 x = e < m ? *reinterpret_cast<const uint2 *>(edges + e) : make_uint2(0u, 0u);
        const bool on = x.x > x.y;
        if (plain) {                                           // (uniform over the grid)
            if (on) {
                atomicAdd(deg + x.x, 1u);
                atomicAdd(deg + x.y, 1u);
            }
            continue;
        }
        cd_add_runs(deg, on, x.x, lane);
        cd_add_runs(deg, on, x.y, lane);
    }
}

__global__ __launch_bounds__(CD_NT) void cd_union_kernel(const uint4 *edges, unsigned long long m, const uint32_t *deg, uint32_t min_nb, uint32_t *parent)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
        const uint2 x = *reinterpret_cast<const uint2 *>(edges + e);
        if (x.x > x.y && deg[x.x] >= min_nb && deg[x.y] >= min_nb) cl_unite(parent, x.x, x.y);
    }
}

// via[i]: the row itself for a core, CD_NONE otherwise (D4); first[i] = i (D5)
__global__ __launch_bounds__(CD_NT) void cd_rows_init_kernel(const uint32_t *deg, uint32_t n, uint32_t min_nb, uint32_t *via, uint32_t *first)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        via[i] = deg[i] >= min_nb ? i : CD_NONE;
        first[i] = i;
    }
}

// the edge has exactly one core end, whichever way round: `member` and `core` are its ends (D3)
__device__ __forceinline__ bool cd_border_edge(const uint4 &x, const uint32_t *deg, uint32_t min_nb, uint32_t &member, uint32_t &core)
{
    if (x.x <= x.y) return false;                              // (padding)
    const bool ch = deg[x.x] >= min_nb, cl = deg[x.y] >= min_nb;
    if (ch == cl) return false;
    member = ch ? x.y : x.x;
    core = ch ? x.x : x.y;
    return true;
}

__global__ __launch_bounds__(CD_NT) void cd_key_kernel(const uint4 *edges, unsigned long long m, const uint32_t *deg, uint32_t min_nb, unsigned long long *best_key)
{
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e0 = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); e0 < m; e0 += stride) {   // (wave-uniform)
        const unsigned long long e = e0 + lane;
        const uint4 x = e < m ? edges[e] : make_uint4(0u, 0u, 0u, 0u);
        uint32_t member = 0, core = 0;
        const bool on = cd_border_edge(x, deg, min_nb, member, core);
        cf_offer_max(best_key, on, member, on ? forest_key(x.z, x.w) : 0ull);
    }
}

__global__ __launch_bounds__(CD_NT) void cd_pick_kernel(const uint4 *edges, unsigned long long m, const uint32_t *deg, uint32_t min_nb,
                                                       const unsigned long long *best_key, uint32_t *via)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
        const uint4 x = edges[e];
        uint32_t member, core;
        if (!cd_border_edge(x, deg, min_nb, member, core)) continue;
        if (forest_key(x.z, x.w) != best_key[member]) continue;                   // (best_key: K3's, an earlier launch)
        if (core < cd_load(via + member)) atomicMin(via + member, core);
    }
}

// counts: [0] cores, [1] borders, [2] noise
__global__ __launch_bounds__(CD_NT) void cd_file_kernel(const uint32_t *deg, uint32_t n, uint32_t min_nb, uint32_t *via, uint32_t *label, uint32_t *first,
                                                       unsigned long long *counts)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t cores = 0, borders = 0, noise = 0;
    for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {   // (wave-uniform: the ballots)
        const uint32_t i = i0 + lane;
        bool core = false, border = false;
        if (i < n) {
            const uint32_t v = via[i];
            core = deg[i] >= min_nb;
            border = !core && v != CD_NONE;
            uint32_t l = i;
            if (core) l = label[i];
            if (border) label[i] = l = label[v];               // (D5: v is a core, nobody writes its label here)
            if (!core && !border) via[i] = i;
            if (i < l && i < cd_load(first + l)) atomicMin(first + l, i);
        }
        cores += (uint32_t)__popcll(__ballot(core));
        borders += (uint32_t)__popcll(__ballot(border));
        noise += (uint32_t)__popcll(__ballot(i < n && !core && !border));
    }
    if (lane == 0) {
        if (cores) atomicAdd(counts + 0, (unsigned long long)cores);
        if (borders) atomicAdd(counts + 1, (unsigned long long)borders);
        if (noise) atomicAdd(counts + 2, (unsigned long long)noise);
    }
}

__global__ __launch_bounds__(CD_NT) void cd_gather_kernel(uint32_t n, uint32_t *label, const uint32_t *first, unsigned long long *n_clusters)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t heads = 0;
    for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {   // (wave-uniform: the ballot)
        const uint32_t i = i0 + lane;
        uint32_t l = CD_NONE;
        if (i < n) label[i] = l = first[label[i]];
        heads += (uint32_t)__popcll(__ballot(l == i));
    }
    if (lane == 0 && heads) atomicAdd(n_clusters, (unsigned long long)heads);
}

static uint32_t cd_blocks(uint64_t items, uint32_t cap)
{
    const uint64_t b = (items + CD_NT - 1) / CD_NT;
    return (uint32_t)(b < 1 ? 1 : b > cap ? cap : b);
}

hipError_t launch_density(const uint4 *edges, uint64_t m, const DensityBufs &b, uint32_t n, uint32_t min_neighbours, bool plain_degree, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(b.counts, 0, 5 * sizeof(unsigned long long), stream);
    if (e != hipSuccess || n == 0) return e;
    if ((e = hipMemsetAsync(b.deg, 0, (size_t)n * sizeof(uint32_t), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.best_key, 0, (size_t)n * sizeof(unsigned long long), stream)) != hipSuccess) return e;      // (D4)
    // a work-item per edge up to 2048 workgroups (8 per CU of an MI355X): beyond that they stride
    const dim3 ge(cd_blocks(m, 2048)), gr(cd_blocks(n, 2048)), nt(CD_NT);
    const unsigned long long mm = m;
    if (m) hipLaunchKernelGGL(cd_degree_kernel, ge, nt, 0, stream, edges, mm, b.deg, plain_degree ? 1 : 0);
    if ((e = launch_cluster_init(b.parent, n, stream)) != hipSuccess) return e;
    if (m) hipLaunchKernelGGL(cd_union_kernel, ge, nt, 0, stream, edges, mm, (const uint32_t *)b.deg, min_neighbours, b.parent);
    if ((e = launch_cluster_label(b.parent, n, b.label, b.counts + 4, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(cd_rows_init_kernel, gr, nt, 0, stream, (const uint32_t *)b.deg, n, min_neighbours, b.via, b.first);
    if (m) {
        hipLaunchKernelGGL(cd_key_kernel, ge, nt, 0, stream, edges, mm, (const uint32_t *)b.deg, min_neighbours, b.best_key);
        hipLaunchKernelGGL(cd_pick_kernel, ge, nt, 0, stream, edges, mm, (const uint32_t *)b.deg, min_neighbours, (const unsigned long long *)b.best_key, b.via);
    }
    hipLaunchKernelGGL(cd_file_kernel, gr, nt, 0, stream, (const uint32_t *)b.deg, n, min_neighbours, b.via, b.label, b.first, b.counts);
    hipLaunchKernelGGL(cd_gather_kernel, gr, nt, 0, stream, n, b.label, (const uint32_t *)b.first, b.counts + 3);
    return hipGetLastError();
}

}  // namespace mg
