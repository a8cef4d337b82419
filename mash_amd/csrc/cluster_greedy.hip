// cluster_greedy.hip — greedy representative clusters of a thresholded all-vs-all, found on the device: the second consumer of
// pass A's ballots (finish_mark_kernel).  The reference has no such command; an EDGE is a pair that passes the filters of
// CommandDistance.cpp:409-422.  Walk the rows in index order: row i is a REPRESENTATIVE iff no representative j < i has an edge
// to i (the lexicographically first maximal independent set of the threshold graph), every other row is a MEMBER of the
// smallest representative it has an edge to.  The walk looks sequential; here it is a fixpoint of rounds whose result does not
// depend on the order anything is executed in.
//
// The ballots of a matrix block live until the next block and the fixpoint needs every edge several times, so the edges are
// first appended to a list of {hi, lo} (hi > lo), one atomic on the cursor per wave and 64 ballot words (cg_append_kernel).
//
// One word per row, state[i]:  0 UNDECIDED   1 UNDECIDED and BLOCKED in this round   2 MEMBER   3 REP.   A round is two launches:
//   part A (cg_round_edges_kernel), per edge, only while state[hi] < MEMBER:
//       state[lo] == REP  -> atomicMax(&state[hi], MEMBER)
//       state[lo] <  MEMBER -> atomicMax(&state[hi], BLOCKED)            (a smaller neighbour is still open: hi has to wait)
//   part B (cg_round_rows_kernel), per row: UNDECIDED -> REP;  BLOCKED -> UNDECIDED, counted as still open.
// Invariants:
//   (G1) MEMBER and REP are final: part A only raises a word (atomicMax) and never above MEMBER, part B only touches words
//        below MEMBER, one work-item per row;
//   (G2) REP is written in part B only, so in part A every REP was written by an EARLIER launch: the kernel boundary has made
//        it visible, no read of it can be stale, and no row turns REP while edges are being read;
//   (G3) a row that part B finds UNDECIDED was met by every one of its edges in the part A before it, and each of them saw a
//        smaller neighbour that was neither REP (the row would be MEMBER) nor open (it would be BLOCKED): MEMBER, which by (G1)
//        is what that neighbour really is.  All smaller neighbours decided, none of them REP: the walk makes this row REP too;
//   (G4) a row is made MEMBER only beside a smaller REP, which by induction over the row index is a representative of the walk.
// Accesses to state[] in part A cross workgroups inside a launch and are agent-scope atomics (relaxed loads that bypass the CU's
// L1, atomicMax).  A load may still return a value that another workgroup has since raised, and that can only DELAY a decision:
// the stale value is a smaller one, 0 or 1 where the memory has 2 -- hi is blocked for a round it need not have waited, or an
// edge is looked at whose hi has just been decided and the atomicMax changes nothing.  No stale value can decide a row wrongly:
// deciding needs a REP (never stale, G2) or the absence of any blocker (G3: a word read as MEMBER is MEMBER).
// Termination: the smallest open row has no open smaller neighbour, so nothing blocks it and every round decides it: at most n
// rounds (a path in index order needs them all), and the host stops at the first round that leaves no row open.
// rep[] is written in LATER launches (cg_rep_init_kernel, cg_assign_kernel): rep[i] = i for a REP, and over the edges
// atomicMin(&rep[hi], lo) for a MEMBER hi beside a REP lo -- the smallest representative it has an edge to.  A representative
// with a larger index is never `lo` of an edge of hi, so it never takes hi.
//
// Extending an earlier result (cg_seed_kernel): the first n_old rows start as what the earlier walk made them, REP or MEMBER, the
// rows behind them UNDECIDED, and the rounds run unchanged over all of them.  A seeded word is >= MEMBER before the first round,
// so by (G1) nobody ever writes it again and by (G2) a seeded REP is as visible as one of an earlier launch.  The walk is in index
// order and the seeded rows precede every open one: what they are does not depend on any row behind them, so they ARE the walk's
// decisions on the concatenated table, (G3)'s "a word read as MEMBER is MEMBER" and (G4)'s induction start from them, and the
// edges from an open row to a seeded MEMBER decide nothing -- which is why a caller may leave the members out of the table.
// Every edge of such a call has an open row as hi; the assignment writes rep[] for those rows only (`first`).
//
// NEAREST representative (launch_nearest_assign, `mash cluster -B`): the same representatives, but a member joins, among ALL the
// representatives it has an edge to, the one whose edge is best in the order of forest_key.h -- the larger shared fraction by
// exact cross-multiplication, equal fractions (also under different denominators) to the smaller representative.  The list is
// cluster_forest.hip's, {hi, lo, numer, denom}; the rounds read its first two words (cg_ends) and are otherwise the same kernel.
// Behind the fixpoint, each in a launch of its own and over the whole list:
//   pass 1 (cn_key_kernel): an edge with one end REP and the other MEMBER: atomicMax(&best_key[member], forest_key(numer, denom))
//   pass 2 (cn_rep_kernel): the same edges whose key == best_key[member]:   atomicMin(&rep[member], representative)
// Invariants:
//   (N1) state[] is final (G1) and was written by earlier launches: plain loads, and "an edge between a REP and a MEMBER" means the
//        same to both passes.  best_key[] is final when pass 2 reads it, for the same reason.
//   (N2) The representative can be EITHER end of the edge: a member below a representative is `lo` and the representative `hi`
//        (cg_assign_kernel only ever looks at `lo`).  Both passes go through cn_ends, which names the member and the
//        representative whichever way round they stand.  An edge between two members decides nothing; no edge joins two
//        representatives (the walk).
//   (N3) best_key[] starts at 0, which IS a key: an edge may carry numer == 0 (only the p-value filter on) and be a member's only
//        edge.  That is harmless because pass 2 looks at edges only, never at "no edge yet": every member has an edge to a
//        representative (G4), so best_key[member] is the maximum over a set that is not empty, 0 included, and the edge that
//        carries it passes pass 2's test.  rep[member] starts at ~0 (cg_rep_init_kernel), above every row.
//   (N4) Padding entries hi == lo (a pair outside the table) are skipped by cn_ends as by every other reader.
//   (N5) The key is the fraction's order exactly for denominators below FOREST_DENOM_LIMIT (forest_key.h): equal fractions have
//        equal keys whatever their denominators, 0/0 is 0/1.  The host refuses larger sketch sizes.
// Why no order of execution can change the result: the only racing accesses are one atomicMax per word in pass 1 and one
// atomicMin per word in pass 2, each over a fixed set of offers, and max and min do not depend on the order of their operands.
// The relaxed look in front of the atomic only skips an offer that cannot win: a stale value is an older one, smaller for
// best_key, larger for rep (cluster_forest.hip, F2).  So rep[] is a function of the edge set and its counts alone.
// Contention is low (a member has a handful of representatives within the threshold, spread over the list), so the offers are
// per lane: no wave-level reduction.
#include "cluster_internal.h"
#include "forest_key.h"

namespace mg {

constexpr int CG_NT = 256;
constexpr uint32_t CG_UNDECIDED = 0, CG_BLOCKED = 1, CG_MEMBER = 2, CG_REP = 3;

__device__ __forceinline__ uint32_t cg_load(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Pass A's ballots as cl_union_kernel reads them: a wave loads 64 words, counts their bits, takes room for all of them with ONE
// atomicAdd on the cursor, then writes the words that are not zero one after the other, a lane per bit.  An entry whose place
// is at or behind `cap` is not written (the cursor still counts it: the host reads how much room the block needed).
// sp: the job's pairs in the index space of state[] (cluster_internal.h), bounds before bases.
__global__ __launch_bounds__(CG_NT) void cg_append_kernel(FinishArgs a, PairSpace sp, uint2 *edges, unsigned long long cap,
                                                         unsigned long long *cursor, uint32_t *overflow)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t words = (a.pairs + 63) / 64;
    const uint64_t nwaves = (uint64_t)gridDim.x * (CG_NT / 64);
    for (uint64_t w0 = ((uint64_t)blockIdx.x * (CG_NT / 64) + (threadIdx.x >> 6)) * 64; w0 < words; w0 += nwaves * 64) {   // (wave-uniform)
        unsigned long long mine = w0 + lane < words ? a.masks[w0 + lane] : 0ull;
        if (w0 + lane + 1 == words && (a.pairs & 63)) mine &= (1ull << (a.pairs & 63)) - 1;      // (bits behind a.pairs are zero anyway)
        unsigned long long nz = __ballot(mine != 0);
        if (!nz) continue;
        const uint32_t cnt = (uint32_t)__popcll(mine);
        uint32_t incl = cnt;                                   // inclusive scan of the words' bit counts over the wave
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const uint32_t total = __shfl(incl, 63);
        unsigned long long base = 0;
        if (lane == 0) {
            base = atomicAdd(cursor, (unsigned long long)total);
            if (base + total > cap) atomicOr(overflow, 1u);
        }
        base = __shfl(base, 0);
        const uint32_t excl = incl - cnt;
        while (nz) {                                           // (wave-uniform)
            const uint32_t j = (uint32_t)__builtin_ctzll(nz);
            nz &= nz - 1;
            const unsigned long long m = __shfl(mine, j);
            const uint32_t off = __shfl(excl, j);
            if ((m >> lane) & 1) {
                const unsigned long long at = base + off + (uint32_t)__popcll(m & ((1ull << lane) - 1));
                if (at < cap) {
                    uint64_t row, col;
                    pair_rc(a, (w0 + j) * 64 + lane, row, col);
                    uint2 e = make_uint2(0u, 0u);              // (a pair outside the table: an entry every reader skips, hi == lo)
                    if (row < sp.rows && col < sp.cols) {
                        const uint32_t r = sp.row_base + (uint32_t)row, c = sp.col_base + (uint32_t)col;
                        e = make_uint2(r > c ? r : c, r > c ? c : r);
                    }
                    edges[at] = e;
                }
            }
        }
    }
}

__global__ __launch_bounds__(CG_NT) void cg_seed_kernel(uint32_t *state, const uint32_t *seed, uint32_t n_old, uint32_t n)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        state[i] = i >= n_old ? CG_UNDECIDED : (!seed || seed[i] == i) ? CG_REP : CG_MEMBER;
}

// `go`: the number of rows the round before left open (nullptr: the first round of a batch, the host has looked); a round
// queued behind the fixpoint does nothing
// E: uint2 {hi, lo}, or uint4 {hi, lo, numer, denom} of which the rounds read the first two words
__device__ __forceinline__ uint2 cg_ends(const uint2 *edges, uint64_t e) { return edges[e]; }
__device__ __forceinline__ uint2 cg_ends(const uint4 *edges, uint64_t e) { return *reinterpret_cast<const uint2 *>(edges + e); }

template <class E>
__global__ __launch_bounds__(CG_NT) void cg_round_edges_kernel(const E *edges, unsigned long long m, uint32_t *state, const uint32_t *go)
{
    if (go && *go == 0) return;                                // (written by an earlier launch; uniform over the grid)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
        const uint2 x = cg_ends(edges, e);
        if (x.x <= x.y) continue;
        const uint32_t sh = cg_load(state + x.x);
        if (sh >= CG_MEMBER) continue;
        const uint32_t sl = cg_load(state + x.y);
        if (sl == CG_REP) atomicMax(state + x.x, CG_MEMBER);
        else if (sl < CG_MEMBER && sh == CG_UNDECIDED) atomicMax(state + x.x, CG_BLOCKED);
    }
}

// one work-item per row, nobody else touches state[] in this launch; *left += rows still open behind this round
__global__ __launch_bounds__(CG_NT) void cg_round_rows_kernel(uint32_t *state, uint32_t n, const uint32_t *go, uint32_t *left)
{
    if (go && *go == 0) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t open = 0;
    for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {   // (wave-uniform: the ballot)
        const uint32_t i = i0 + lane;
        const uint32_t s = i < n ? state[i] : CG_MEMBER;
        if (s == CG_UNDECIDED) state[i] = CG_REP;
        else if (s == CG_BLOCKED) state[i] = CG_UNDECIDED;
        open += (uint32_t)__popcll(__ballot(s == CG_BLOCKED));
    }
    if (lane == 0 && open) atomicAdd(left, open);
}

// rep[] holds rows first .. n - 1; the representatives are counted over all n rows
__global__ __launch_bounds__(CG_NT) void cg_rep_init_kernel(const uint32_t *state, uint32_t n, uint32_t first, uint32_t *rep, unsigned long long *n_reps)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t reps = 0;
    for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {   // (wave-uniform: the ballot)
        const uint32_t i = i0 + lane;
        const bool is_rep = i < n && state[i] == CG_REP;
        if (i < n && i >= first) rep[i - first] = is_rep ? i : 0xFFFFFFFFu;
        reps += (uint32_t)__popcll(__ballot(is_rep));
    }
    if (lane == 0 && reps) atomicAdd(n_reps, (unsigned long long)reps);
}

__global__ __launch_bounds__(CG_NT) void cg_assign_kernel(const uint2 *edges, unsigned long long m, const uint32_t *state, uint32_t first, uint32_t *rep)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
        const uint2 x = edges[e];
        if (x.x > x.y && x.x >= first && state[x.y] == CG_REP && state[x.x] == CG_MEMBER) atomicMin(rep + (x.x - first), x.y);
    }
}

// ---- the nearest representative (N1 .. N5 at the head of the file)

__device__ __forceinline__ unsigned long long cn_load(unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the edge joins a REP and a MEMBER, whichever way round: `member` and `rep` are its ends
__device__ __forceinline__ bool cn_ends(const uint4 &x, const uint32_t *state, uint32_t &member, uint32_t &rep)
{
    if (x.x <= x.y) return false;                              // (padding)
    const uint32_t sh = state[x.x], sl = state[x.y];
    if (sh == CG_MEMBER && sl == CG_REP) { member = x.x; rep = x.y; return true; }
    if (sh == CG_REP && sl == CG_MEMBER) { member = x.y; rep = x.x; return true; }
    return false;
}

__global__ __launch_bounds__(CG_NT) void cn_key_kernel(const uint4 *edges, unsigned long long m, const uint32_t *state, unsigned long long *best_key)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
        const uint4 x = edges[e];
        uint32_t member, rep;
        if (!cn_ends(x, state, member, rep)) continue;
        const unsigned long long key = forest_key(x.z, x.w);
        if (key > cn_load(best_key + member)) atomicMax(best_key + member, key);
    }
}

__global__ __launch_bounds__(CG_NT) void cn_rep_kernel(const uint4 *edges, unsigned long long m, const uint32_t *state, const unsigned long long *best_key,
                                                      uint32_t *rep_of)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += stride) {
        const uint4 x = edges[e];
        uint32_t member, rep;
        if (!cn_ends(x, state, member, rep)) continue;
        if (forest_key(x.z, x.w) != best_key[member]) continue;                   // (best_key: pass 1's, an earlier launch)
        if (rep < cg_load(rep_of + member)) atomicMin(rep_of + member, rep);
    }
}

static uint32_t cg_blocks(uint64_t items, uint32_t cap)
{
    const uint64_t b = (items + CG_NT - 1) / CG_NT;
    return (uint32_t)(b < 1 ? 1 : b > cap ? cap : b);
}

hipError_t launch_greedy_append(const FinishArgs &a, const PairSpace &sp, uint2 *edges, uint64_t cap, unsigned long long *cursor,
                                uint32_t *overflow, hipStream_t stream)
{
    if (a.pairs == 0 || sp.rows == 0 || sp.cols == 0) return hipSuccess;
    // a work-item per mask word up to 2048 workgroups (8 per CU of an MI355X): beyond that the waves stride
    hipLaunchKernelGGL(cg_append_kernel, dim3(cg_blocks((a.pairs + 63) / 64, 2048)), dim3(CG_NT), 0, stream, a, sp, edges, (unsigned long long)cap,
                       cursor, overflow);
    return hipGetLastError();
}

hipError_t launch_greedy_append(const FinishArgs &a, uint32_t n, uint2 *edges, uint64_t cap, unsigned long long *cursor, uint32_t *overflow,
                                hipStream_t stream)
{
    return launch_greedy_append(a, PairSpace{n, n, 0u, 0u}, edges, cap, cursor, overflow, stream);
}

hipError_t launch_greedy_seed(uint32_t *state, const uint32_t *seed, uint32_t n_old, uint32_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(cg_seed_kernel, dim3(cg_blocks(n, 2048)), dim3(CG_NT), 0, stream, state, seed, n_old, n);
    return hipGetLastError();
}

template <class E>
static hipError_t cg_rounds(const E *edges, uint64_t m, uint32_t *state, uint32_t n, uint32_t *left, uint32_t rounds, hipStream_t stream)
{
    if (n == 0 || rounds == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(left, 0, (size_t)rounds * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t *go = r ? left + (r - 1) : nullptr;
        if (m) hipLaunchKernelGGL(cg_round_edges_kernel<E>, dim3(cg_blocks(m, 2048)), dim3(CG_NT), 0, stream, edges, (unsigned long long)m, state, go);
        hipLaunchKernelGGL(cg_round_rows_kernel, dim3(cg_blocks(n, 2048)), dim3(CG_NT), 0, stream, state, n, go, left + r);
    }
    return hipGetLastError();
}

hipError_t launch_greedy_rounds(const uint2 *edges, uint64_t m, uint32_t *state, uint32_t n, uint32_t *left, uint32_t rounds, hipStream_t stream)
{
    return cg_rounds(edges, m, state, n, left, rounds, stream);
}

hipError_t launch_greedy_rounds(const uint4 *edges, uint64_t m, uint32_t *state, uint32_t n, uint32_t *left, uint32_t rounds, hipStream_t stream)
{
    return cg_rounds(edges, m, state, n, left, rounds, stream);
}

hipError_t launch_greedy_assign(const uint2 *edges, uint64_t m, const uint32_t *state, uint32_t n, uint32_t *rep, unsigned long long *n_reps,
                                hipStream_t stream, uint32_t first)
{
    hipError_t e = hipMemsetAsync(n_reps, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess || n == 0) return e;
    hipLaunchKernelGGL(cg_rep_init_kernel, dim3(cg_blocks(n, 2048)), dim3(CG_NT), 0, stream, state, n, first, rep, n_reps);
    if (m && first < n) hipLaunchKernelGGL(cg_assign_kernel, dim3(cg_blocks(m, 2048)), dim3(CG_NT), 0, stream, edges, (unsigned long long)m, state, first, rep);
    return hipGetLastError();
}

hipError_t launch_nearest_assign(const uint4 *edges, uint64_t m, const uint32_t *state, uint32_t n, unsigned long long *best_key, uint32_t *rep,
                                 unsigned long long *n_reps, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(n_reps, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess || n == 0) return e;
    if ((e = hipMemsetAsync(best_key, 0, (size_t)n * sizeof(unsigned long long), stream)) != hipSuccess) return e;      // (N3)
    hipLaunchKernelGGL(cg_rep_init_kernel, dim3(cg_blocks(n, 2048)), dim3(CG_NT), 0, stream, state, n, 0u, rep, n_reps);
    if (m) {
        hipLaunchKernelGGL(cn_key_kernel, dim3(cg_blocks(m, 2048)), dim3(CG_NT), 0, stream, edges, (unsigned long long)m, state, best_key);
        hipLaunchKernelGGL(cn_rep_kernel, dim3(cg_blocks(m, 2048)), dim3(CG_NT), 0, stream, edges, (unsigned long long)m, state, best_key, rep);
    }
    return hipGetLastError();
}

}  // namespace mg
