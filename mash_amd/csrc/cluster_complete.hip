// cluster_complete.hip — complete-linkage clusters of a thresholded all-vs-all, cut at the threshold, found on the device: `mash
// cluster -L`.  The reference has no such command (its user pipes `mash triangle -E -d` into hclust or scipy on the host).  An EDGE is
// a pair that passes the filters of CommandDistance.cpp:409-422, with its counts numer/denom.
//
// THE DEFINITION.  A cluster's id is its smallest row; start from singletons.  Two clusters are LINKED iff every pair between them is
// an edge, and the link's WEIGHT is the worst of those edges, the smallest fraction (exactly: forest_key.h).  Links are ORDERED:
// larger weight first, equal weights by ascending larger id, then ascending smaller id (forest_before with forest_rc(hi id, lo id)).
// Merge the first link of all, the new cluster keeps the smaller id; repeat until no link is left.  label[i] = the id of i's cluster.
//
// WHY ROUNDS MAY RUN IN PARALLEL.  Call a link MUTUAL if it is the first link of both its clusters.  Take a mutual link (A, B) and
// let the walk merge another pair (I, J) first.  (I, A) and (J, A), where they exist, rank behind (A, B); the link (I u J, A) exists
// only if both did, its weight is the smaller of theirs and it carries the id of I or of J: it still ranks behind (A, B), and so for
// B.  So a mutual link stays mutual until the walk merges it, the first link of all is always mutual, and the walk performs exactly
// the merges of "merge every mutual link, repeat".
//
// THE LINKS are the appended edge list itself (launch_forest_append: {hi, lo, numer, denom}, 16 bytes) with key[e] = forest_key(numer,
// denom) beside it.  A link's identity {hi id, lo id} never changes: the survivor of a merge keeps its id, so the link between two
// surviving clusters IS the list entry of their ids.  Only a link's weight drops, and links die (key[e] = CC_DEAD); dead links are
// skipped, never compacted.  ONE static lookup from forest_rc(hi, lo) to the entry's place is built behind the last append: open
// addressing, a 64-bit compare-and-swap on the slot's key, 2 m + 1 slots for m entries, so every probe loop ends at an empty slot (and
// is bounded by the table's size besides).  The list holds a pair once; were it to hold one twice, the later entry is marked dead.
//
// A ROUND is five launches over the live links:
//   K1 (cc_key_kernel), per end:   atomicMax(&best_key[id], key[e])
//   K2 (cc_rc_kernel), per end whose best_key == key[e]:   atomicMin(&best_rc[id], hi << 32 | lo)
//   K3 (cc_mate_kernel): a link with hi << 32 | lo == best_rc[hi] == best_rc[lo] is mutual: mate[hi] = lo, mate[lo] = hi, parent[hi] = lo.
//       It is counted into merged[r], every live link into live[r] (one atomic per wave and launch).
//   K4 (cc_decide_kernel), writes next[e] ONLY.  An end is ABSORBED if it is the larger id of a mutual link.  A link with an absorbed
//       end dies.  A link {a, b} between two survivors of which one at least merged survives iff every link of {a, mate a} x {b, mate b}
//       is alive -- 1 or 3 lookups -- and its new key is the smallest of them.  A link whose ends did not merge keeps its key.
//   K5 (cc_commit_kernel), per live link: key[e] = next[e]; per row: best_key / best_rc / mate reset.
// WHY STALE READS CANNOT HURT.
//   (L1) Everything a launch DECIDES ON was finished by an earlier launch: K1 reads key (K5 of the round before, or the begin), K2
//        reads best_key (K1), K3 reads best_rc (K2), K4 reads mate (K3) and key -- its own link's and, through the lookup, other
//        links' -- which no launch between K5 of the round before and K5 of this round writes.  That is why K4 and K5 are two
//        launches: K4 reads the keys and the alive state that K5 writes.  The lookup is written by the begin alone.
//   (L2) Inside a launch the only racing accesses are the monotone atomics on best_key (only raised) and best_rc (only lowered), with
//        the look-before-atomic of cf_offer_* (cluster_internal.h): a stale look is an older value, which can only let through an
//        atomic that changes nothing.  The final value is the max / min over all offers, whatever the order.
//   (L3) K3's stores do not race: best_rc[id] names ONE link, so an id is an end of at most one mutual link, and mate[hi], mate[lo]
//        and parent[hi] have one writer each.  Every other store of a round goes to the work-item's own link (next[e], key[e]) or row.
//   (L4) parent[] only ever gets "larger id under smaller", from ids that were roots (an absorbed id has no live link afterwards and
//        is never an end again), so launch_cluster_label gives label[] and the number of clusters unchanged.
// Termination: a round with a live link merges the first link of all (it is mutual), so merged[r] == 0 iff no link is alive: the
// fixpoint.  Every merge removes a cluster: at most n - 1 rounds merge, and a clique whose fractions all tie needs that many (one
// pair per round).  Every launch of round r first reads merged[r - 1] and returns if it is zero, so the host queues rounds in batches
// and waits once per batch (host_cluster.cpp).
//
// Compiles for tools/hipemu too (MG_HIP_EMU, tests/test_complete_emu.py): wave operations sit in uniform control flow, nothing relies on
// the lock step of a wave, no library call.
#include "cluster_internal.h"
#include "forest_key.h"

namespace mg {

constexpr int CC_NT = 256;
constexpr uint32_t CC_NO_MATE = ~0u;

__device__ __forceinline__ uint64_t cc_slot(const CompleteBufs &b, unsigned long long rc)
{
    unsigned long long h = rc;                                 // (the finalizer of splitmix64)
    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
    h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
    h ^= h >> 31;
    return ((h & b.hash_and) | b.hash_or) % b.slots;
}

// the place of link {x, y} in the list, CC_DEAD if the list has no such entry (written by the begin, an earlier launch)
__device__ __forceinline__ unsigned long long cc_find(const CompleteBufs &b, uint32_t x, uint32_t y)
{
    const unsigned long long rc = x > y ? forest_rc(x, y) : forest_rc(y, x);
    uint64_t at = cc_slot(b, rc);
    for (uint64_t step = 0; step < b.slots; step++) {
        const unsigned long long have = b.slot_rc[at];
        if (have == rc) return b.slot_e[at];
        if (have == CF_NONE) break;
        at = at + 1 == b.slots ? 0 : at + 1;
    }
    return CC_DEAD;
}

// the smaller of key `k` and the key of link {x, y}; CC_DEAD once one of them is dead or absent
__device__ __forceinline__ unsigned long long cc_worst(const CompleteBufs &b, unsigned long long k, uint32_t x, uint32_t y)
{
    if (k == CC_DEAD) return k;
    const unsigned long long e = cc_find(b, x, y);
    if (e == CC_DEAD) return CC_DEAD;
    const unsigned long long o = b.key[e];
    return o == CC_DEAD || o < k ? o : k;
}

__global__ __launch_bounds__(CC_NT) void cc_begin_rows_kernel(CompleteBufs b, uint32_t n)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        b.parent[i] = i;
        b.mate[i] = CC_NO_MATE;
        b.best_key[i] = 0;
        b.best_rc[i] = CF_NONE;
    }
}

// behind the slots' clearing: every link's key, and its place under its {hi, lo}
__global__ __launch_bounds__(CC_NT) void cc_begin_links_kernel(const uint4 *edges, unsigned long long m, CompleteBufs b)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
        const uint4 x = edges[e];
        unsigned long long key = CC_DEAD;
        if (x.x > x.y) {
            const unsigned long long rc = forest_rc(x.x, x.y);
            uint64_t at = cc_slot(b, rc);
            for (uint64_t step = 0; step < b.slots; step++) {
                const unsigned long long was = atomicCAS(b.slot_rc + at, CF_NONE, rc);
                if (was == CF_NONE) {
                    b.slot_e[at] = e;
                    key = forest_key(x.z, x.w);
                    break;
                }
                if (was == rc) break;                          // (the pair a second time: this entry stays dead)
                at = at + 1 == b.slots ? 0 : at + 1;
            }
        }
        b.key[e] = key;
    }
}

// One link per lane of a wave-uniform loop: what K1, K2 and K3 start from
struct CcLink {
    uint32_t hi, lo;
    unsigned long long key;
    bool live;
};

__device__ __forceinline__ CcLink cc_link(const uint4 *edges, const unsigned long long *key, unsigned long long e, unsigned long long m)
{
    CcLink r;
    r.hi = r.lo = 0;
    r.key = e < m ? key[e] : CC_DEAD;
    r.live = r.key != CC_DEAD;
    if (r.live) {                                              // (a dead link costs its key's 8 bytes, not the entry's 16)
        const uint4 x = edges[e];
        r.hi = x.x;
        r.lo = x.y;
    }
    return r;
}

// `go`: the links the round before merged (nullptr: the first round of a batch); a round queued behind the fixpoint does nothing
__global__ __launch_bounds__(CC_NT) void cc_key_kernel(const uint4 *edges, unsigned long long m, CompleteBufs b, const uint32_t *go)
{
    if (go && *go == 0) return;                                // (written by an earlier launch; uniform over the grid)
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e0 = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); e0 < m; e0 += stride) {   // (wave-uniform)
        const CcLink l = cc_link(edges, b.key, e0 + lane, m);
        cf_offer_max(b.best_key, l.live, l.hi, l.key);
        cf_offer_max(b.best_key, l.live, l.lo, l.key);
    }
}

__global__ __launch_bounds__(CC_NT) void cc_rc_kernel(const uint4 *edges, unsigned long long m, CompleteBufs b, const uint32_t *go)
{
    if (go && *go == 0) return;
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e0 = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); e0 < m; e0 += stride) {   // (wave-uniform)
        const CcLink l = cc_link(edges, b.key, e0 + lane, m);
        const unsigned long long rc = forest_rc(l.hi, l.lo);
        cf_offer_min(b.best_rc, l.live && b.best_key[l.hi] == l.key, l.hi, rc);        // (best_key: K1's, an earlier launch)
        cf_offer_min(b.best_rc, l.live && b.best_key[l.lo] == l.key, l.lo, rc);
    }
}

__global__ __launch_bounds__(CC_NT) void cc_mate_kernel(const uint4 *edges, unsigned long long m, CompleteBufs b, const uint32_t *go, uint32_t *merged,
                                                        unsigned long long *live)
{
    if (go && *go == 0) return;
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long n_live = 0;
    uint32_t n_merged = 0;
    for (unsigned long long e0 = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); e0 < m; e0 += stride) {   // (wave-uniform)
        const CcLink l = cc_link(edges, b.key, e0 + lane, m);
        const unsigned long long rc = forest_rc(l.hi, l.lo);
        const bool mutual = l.live && b.best_rc[l.hi] == rc && b.best_rc[l.lo] == rc;          // (best_rc: K2's, an earlier launch)
        n_live += (unsigned long long)__popcll(__ballot(l.live));
        n_merged += (uint32_t)__popcll(__ballot(mutual));
        if (mutual) {                                          // (L3: the one writer of these three words)
            b.mate[l.hi] = l.lo;
            b.mate[l.lo] = l.hi;
            b.parent[l.hi] = l.lo;
        }
    }
    if (lane == 0 && n_live) atomicAdd(live, n_live);
    if (lane == 0 && n_merged) atomicAdd(merged, n_merged);
}

// one work-item per link, no wave operation; writes next[e] and nothing else
__global__ __launch_bounds__(CC_NT) void cc_decide_kernel(const uint4 *edges, unsigned long long m, CompleteBufs b, const uint32_t *go)
{
    if (go && *go == 0) return;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
        const CcLink l = cc_link(edges, b.key, e, m);
        if (!l.live) continue;
        const uint32_t ma = b.mate[l.hi], mb = b.mate[l.lo];   // (K3's, an earlier launch)
        unsigned long long k = l.key;
        if ((ma != CC_NO_MATE && ma < l.hi) || (mb != CC_NO_MATE && mb < l.lo)) {
            k = CC_DEAD;                                       // an absorbed end (the mutual link itself is such a link)
        } else {
            // both ends survive; a partner is larger than the end it joins, so it is neither of the two ends
            if (ma != CC_NO_MATE) k = cc_worst(b, k, ma, l.lo);
            if (mb != CC_NO_MATE) k = cc_worst(b, k, l.hi, mb);
            if (ma != CC_NO_MATE && mb != CC_NO_MATE) k = cc_worst(b, k, ma, mb);
        }
        b.next[e] = k;
    }
}

__global__ __launch_bounds__(CC_NT) void cc_commit_kernel(unsigned long long m, CompleteBufs b, uint32_t n, const uint32_t *go)
{
    if (go && *go == 0) return;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x, first = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned long long e = first; e < m; e += stride)
        if (b.key[e] != CC_DEAD) b.key[e] = b.next[e];         // (next[e]: K4's, an earlier launch; written for every live link)
    for (unsigned long long i = first; i < n; i += stride) {
        b.mate[i] = CC_NO_MATE;
        b.best_key[i] = 0;
        b.best_rc[i] = CF_NONE;
    }
}

static uint32_t cc_blocks(uint64_t items, uint32_t cap)
{
    const uint64_t b = (items + CC_NT - 1) / CC_NT;
    return (uint32_t)(b < 1 ? 1 : b > cap ? cap : b);
}

uint64_t complete_slots(uint64_t m) { return 2 * m + 1; }

hipError_t launch_complete_begin(const uint4 *edges, uint64_t m, const CompleteBufs &b, uint32_t n, hipStream_t stream)
{
    if (n) hipLaunchKernelGGL(cc_begin_rows_kernel, dim3(cc_blocks(n, 2048)), dim3(CC_NT), 0, stream, b, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !m || !n) return e;
    if ((e = hipMemsetAsync(b.slot_rc, 0xFF, (size_t)b.slots * sizeof(unsigned long long), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(cc_begin_links_kernel, dim3(cc_blocks(m, 2048)), dim3(CC_NT), 0, stream, edges, (unsigned long long)m, b);
    return hipGetLastError();
}

hipError_t launch_complete_rounds(const uint4 *edges, uint64_t m, const CompleteBufs &b, uint32_t n, uint32_t rounds, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(b.merged, 0, (size_t)rounds * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(b.live, 0, (size_t)rounds * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    // a work-item per link up to 2048 workgroups (8 per CU of an MI355X): beyond that they stride
    const dim3 grid(cc_blocks(m, 2048)), both(cc_blocks(m > n ? m : n, 2048));
    for (uint32_t r = 0; r < rounds && m && n; r++) {
        const uint32_t *go = r ? b.merged + (r - 1) : nullptr;
        hipLaunchKernelGGL(cc_key_kernel, grid, dim3(CC_NT), 0, stream, edges, (unsigned long long)m, b, go);
        hipLaunchKernelGGL(cc_rc_kernel, grid, dim3(CC_NT), 0, stream, edges, (unsigned long long)m, b, go);
        hipLaunchKernelGGL(cc_mate_kernel, grid, dim3(CC_NT), 0, stream, edges, (unsigned long long)m, b, go, b.merged + r, b.live + r);
        hipLaunchKernelGGL(cc_decide_kernel, grid, dim3(CC_NT), 0, stream, edges, (unsigned long long)m, b, go);
        hipLaunchKernelGGL(cc_commit_kernel, both, dim3(CC_NT), 0, stream, (unsigned long long)m, b, n, go);
    }
    return hipGetLastError();
}

}  // namespace mg
