// spectrum.hip — the distance spectrum of a job (`mash triangle -H`, `mash dist -H`): for every {numer, denom} that occurs among the
// job's pairs, how many pairs have it.  A histogram with two homes for a key (spectrum_internal.h: SpectrumBins):
//
//   denom == s       full[numer], 64-bit counts in global memory -- nearly every pair of a real collection.  Where 4 (s + 1) bytes
//                    fit in 64 KiB (s <= 16 383) a workgroup counts in 32-bit bins in DYNAMIC LDS sized by s (s = 1000: 4 KB, the
//                    occupancy stays) and sends its non-zero bins to memory at its end, one 64-bit add each; above that s the adds
//                    go to memory directly;
//   any other denom  (short sketches) one open-addressing table in global memory keyed by numer << 32 | denom: a slot is claimed by
//                    a 64-bit compare-and-swap on its key (CF_NONE: empty) and its count bumped by a 64-bit add -- the idiom of
//                    cc_begin_links_kernel.  An entry that finds no slot raises a flag; the host enlarges the table, clears every
//                    bin and runs the call again.
//
// Everything is an integer and the only combining operation is the add, which commutes: the bins are a function of the job alone --
// not of the route (ballots over a list or over matrix blocks, the list with the rule, the whole matrix), the blocking, the schedule,
// the size of the table, or whether equal keys were combined in the wave before they reached memory.
//
// Two shapes put nearly every pair into ONE bin -- all rows identical (s/s), and the whole matrix of an unrelated collection (0/s) --
// and must not queue 64 adds of a wave behind one address: the lanes of a wave that hold the same key as the wave's first waiting lane
// leave as one add of their number (ballot, popcount), for SP_ROUNDS such keys; the lanes still waiting add for themselves, and a
// wave with fewer than SP_MIN_ENTRIES entries skips the rounds.  Which lanes hold the same key is found by comparing keys.  On the
// whole-matrix form {0, s} does not even reach the rounds: a lane counts its own in a register and the wave sends one add at its end.
// The plain variant (one add per entry, straight to memory, no LDS) is kept for the A/B of tools/spectrum_bench.py: context option
// MASHGPU_SPECTRUM_PLAIN.
//
// Wave operations stand in wave-uniform control flow and nothing relies on lock step: the file compiles for tools/hipemu (MG_HIP_EMU).
#include "spectrum_internal.h"

#ifndef MG_HIP_EMU
#define MG_DYN_SHARED(T, name)                                   \
    extern __shared__ __align__(16) unsigned char name##_raw[]; \
    T *name = reinterpret_cast<T *>(name##_raw)
#endif

namespace mg {

constexpr int SP_NT = 256;
constexpr int SP_ROUNDS = 2;          // distinct keys of a wave whose lanes are combined; the rest add for themselves
constexpr int SP_MIN_ENTRIES = 8;     // entries in a wave below which every lane adds for itself
// A launch with LDS bins counts fewer than 2^32 entries IN ALL (launchers: spectrum_lds), so a workgroup's share, and with it any
// 32-bit bin, stays below 2^32 and cannot wrap.
constexpr uint64_t SP_LDS_MAX_ENTRIES = 0xFFFFFFFFull;

__device__ __forceinline__ uint64_t spectrum_slot(unsigned long long key, uint64_t slots)
{
    return (uint64_t)(((key ^ (key >> 32)) * 0x9E3779B97F4A7C15ull) >> 24) & (slots - 1);
}

// n entries of one key that has no place in full[]
__device__ __forceinline__ void sp_table_add(const SpectrumBins &b, unsigned long long key, unsigned long long n)
{
    uint64_t at = spectrum_slot(key, b.slots);
    for (uint64_t step = 0; step < b.slots; step++) {
        unsigned long long was = cf_load(b.keys + at);
        if (was == CF_NONE) was = atomicCAS(b.keys + at, CF_NONE, key);
        if (was == CF_NONE || was == key) {
            atomicAdd(b.vals + at, n);
            return;
        }
        at = (at + 1) & (b.slots - 1);
    }
    atomicOr(b.overflow, 1u);                                  // (not counted: the host runs the call again with a larger table)
}

// n entries of {numer, denom} to their home (numer <= s is checked, not assumed: nothing is ever added past full[s] or lds[s])
template <bool LDS>
__device__ __forceinline__ void sp_put(const SpectrumBins &b, uint32_t *lds, uint32_t numer, uint32_t denom, uint32_t n)
{
    if (denom == b.s && numer <= b.s) {
        if (LDS) atomicAdd(lds + numer, n);
        else atomicAdd(b.full + numer, (unsigned long long)n);
    } else {
        sp_table_add(b, (unsigned long long)numer << 32 | denom, n);
    }
}

// One entry per lane with `on`.  Called by whole waves.
template <bool LDS, bool PLAIN>
__device__ __forceinline__ void sp_add_wave(const SpectrumBins &b, uint32_t *lds, bool on, uint32_t numer, uint32_t denom)
{
    if (PLAIN) {
        if (on) sp_put<false>(b, nullptr, numer, denom, 1u);
        return;
    }
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long key = (unsigned long long)numer << 32 | denom;
    unsigned long long todo = __ballot(on);                    // (wave-uniform from here on: every lane takes part in the shuffles)
    const int rounds = __popcll(todo) >= SP_MIN_ENTRIES ? SP_ROUNDS : 0;
    for (int round = 0; todo && round < rounds; round++) {
        const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
        const unsigned long long k0 = __shfl(key, lead);
        const unsigned long long grp = __ballot(on && key == k0);      // (a key leaves `todo` whole: no later leader holds it again)
        if (lane == lead) sp_put<LDS>(b, lds, (uint32_t)(k0 >> 32), (uint32_t)k0, (uint32_t)__popcll(grp));
        todo &= ~grp;
    }
    if ((todo >> lane) & 1) sp_put<LDS>(b, lds, numer, denom, 1u);
}

template <bool LDS>
__device__ __forceinline__ void sp_lds_begin(const SpectrumBins &b, uint32_t *lds)
{
    if (!LDS) return;
    for (uint32_t i = threadIdx.x; i <= b.s; i += SP_NT) lds[i] = 0;
    __syncthreads();
}

template <bool LDS>
__device__ __forceinline__ void sp_lds_end(const SpectrumBins &b, uint32_t *lds)
{
    if (!LDS) return;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= b.s; i += SP_NT) {
        const uint32_t n = lds[i];
        if (n) atomicAdd(b.full + i, (unsigned long long)n);
    }
}

template <bool LDS, bool PLAIN>
__global__ __launch_bounds__(SP_NT) void sp_marked_kernel(FinishArgs a, PairSpace sp, SpectrumBins b)
{
    MG_DYN_SHARED(uint32_t, lds);
    sp_lds_begin<LDS>(b, lds);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t words = (a.pairs + 63) / 64;
    const uint64_t nwaves = (uint64_t)gridDim.x * (SP_NT / 64);
    const bool clip = sp.rows != 0xFFFFFFFFu || sp.cols != 0xFFFFFFFFu;      // (the whole job: no pair_rc, no square root per set bit)
    for (uint64_t w0 = ((uint64_t)blockIdx.x * (SP_NT / 64) + (threadIdx.x >> 6)) * 64; w0 < words; w0 += nwaves * 64) {
        const unsigned long long mine = w0 + lane < words ? a.masks[w0 + lane] : 0ull;
        unsigned long long nz = __ballot(mine != 0);
        while (nz) {                                           // (wave-uniform)
            const uint32_t j = (uint32_t)__builtin_ctzll(nz);
            nz &= nz - 1;
            const unsigned long long m = __shfl(mine, j);
            const uint64_t idx = (w0 + j) * 64 + lane;
            bool in = ((m >> lane) & 1) && idx < a.pairs;
            if (in && clip) {
                uint64_t r, c;
                pair_rc(a, idx, r, c);
                in = r < sp.rows && c < sp.cols;
            }
            uint2 cnt = make_uint2(0u, 0u);
            if (in) cnt = a.counts[idx];
            sp_add_wave<LDS, PLAIN>(b, lds, in, cnt.x, cnt.y);
        }
    }
    sp_lds_end<LDS>(b, lds);
}

template <bool LDS, bool PLAIN>
__global__ __launch_bounds__(SP_NT) void sp_all_kernel(const uint2 *counts, uint64_t pairs, SpectrumBins b)
{
    MG_DYN_SHARED(uint32_t, lds);
    sp_lds_begin<LDS>(b, lds);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * (SP_NT / 64);
    unsigned long long zeros = 0;                              // this lane's {0, s}
    for (uint64_t base = ((uint64_t)blockIdx.x * (SP_NT / 64) + (threadIdx.x >> 6)) * 64; base < pairs; base += nwaves * 64) {
        const uint64_t idx = base + lane;
        bool on = idx < pairs;
        uint2 cnt = make_uint2(0u, 0u);
        if (on) cnt = counts[idx];
        if (!PLAIN && on && cnt.x == 0 && cnt.y == b.s) {
            zeros++;
            on = false;
        }
        sp_add_wave<LDS, PLAIN>(b, lds, on, cnt.x, cnt.y);
    }
    if (!PLAIN) {                                              // (every wave gets here: its loop bound is wave-uniform)
        for (uint32_t o = 32; o; o >>= 1) zeros += __shfl_xor(zeros, o);
        if (lane == 0 && zeros) atomicAdd(b.full, zeros);
    }
    sp_lds_end<LDS>(b, lds);
}

template <bool LDS, bool PLAIN>
__global__ __launch_bounds__(SP_NT) void sp_list_kernel(const uint2 *cnt, const uint2 *rc, uint64_t K, const uint32_t *nh_row, const uint32_t *nh_col,
                                                        SpectrumBins b, unsigned long long *rule, unsigned long long *listed_zero)
{
    MG_DYN_SHARED(uint32_t, lds);
    sp_lds_begin<LDS>(b, lds);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * (SP_NT / 64);
    unsigned long long zeros = 0;                              // entries with numer == 0 this wave has seen (wave-uniform)
    for (uint64_t base = ((uint64_t)blockIdx.x * (SP_NT / 64) + (threadIdx.x >> 6)) * 64; base < K; base += nwaves * 64) {
        const uint64_t idx = base + lane;
        const bool on = idx < K;
        uint2 c = make_uint2(0u, 0u);
        uint32_t d = 0;
        if (on) {
            c = cnt[idx];
            const uint2 p = rc[idx];
            const uint32_t na = nh_row[p.x], nb = nh_col[p.y];
            const uint64_t sum = (uint64_t)(na < b.s ? na : b.s) + (nb < b.s ? nb : b.s);
            d = sum < b.s ? (uint32_t)sum : b.s;               // the rule denominator: what the pair would be if it were not listed
        }
        sp_add_wave<LDS, PLAIN>(b, lds, on, c.x, c.y);
        // the second binning: nearly every entry has two full sketches, those leave as one add
        const unsigned long long at_s = __ballot(on && d == b.s);
        if (at_s && lane == (uint32_t)__builtin_ctzll(at_s)) atomicAdd(rule + b.s, (unsigned long long)__popcll(at_s));
        if (on && d != b.s) atomicAdd(rule + d, 1ull);
        zeros += (unsigned long long)__popcll(__ballot(on && c.x == 0));
    }
    if (lane == 0 && zeros) atomicAdd(listed_zero, zeros);
    sp_lds_end<LDS>(b, lds);
}

static uint32_t sp_blocks(uint64_t items)
{
    // a work-item per entry (mask word) up to 2048 workgroups (8 per CU of an MI355X): beyond that the waves stride
    const uint64_t n = (items + SP_NT - 1) / SP_NT;
    return (uint32_t)(n < 1 ? 1 : n > 2048 ? 2048 : n);
}

// LDS bins: they fit, and the launch's entries cannot wrap a 32-bit bin
static bool spectrum_lds(const SpectrumBins &b, uint64_t entries, bool plain)
{
    return !plain && b.s <= SPECTRUM_LDS_MAX_S && entries <= SP_LDS_MAX_ENTRIES;
}

#define SP_LAUNCH(kernel, grid, lds, plain, ...)                                                                                      \
    do {                                                                                                                              \
        const size_t shm__ = (lds) ? ((size_t)b.s + 1) * sizeof(uint32_t) : 0;                                                        \
        if (plain) hipLaunchKernelGGL((kernel<false, true>), grid, dim3(SP_NT), 0, stream, __VA_ARGS__);                              \
        else if (lds) hipLaunchKernelGGL((kernel<true, false>), grid, dim3(SP_NT), shm__, stream, __VA_ARGS__);                       \
        else hipLaunchKernelGGL((kernel<false, false>), grid, dim3(SP_NT), 0, stream, __VA_ARGS__);                                   \
    } while (0)

hipError_t launch_spectrum_marked(const FinishArgs &a, const PairSpace &sp, const SpectrumBins &b, hipStream_t stream, bool plain)
{
    if (a.pairs == 0 || sp.rows == 0 || sp.cols == 0) return hipSuccess;
    if (b.slots == 0 || (b.slots & (b.slots - 1))) return hipErrorInvalidValue;
    const bool lds = spectrum_lds(b, a.pairs, plain);
    const dim3 grid(sp_blocks((a.pairs + 63) / 64));
    SP_LAUNCH(sp_marked_kernel, grid, lds, plain, a, sp, b);
    return hipGetLastError();
}

hipError_t launch_spectrum_all(const uint2 *counts, uint64_t pairs, const SpectrumBins &b, hipStream_t stream, bool plain)
{
    if (pairs == 0) return hipSuccess;
    if (b.slots == 0 || (b.slots & (b.slots - 1))) return hipErrorInvalidValue;
    const bool lds = spectrum_lds(b, pairs, plain);
    const dim3 grid(sp_blocks(pairs));
    SP_LAUNCH(sp_all_kernel, grid, lds, plain, counts, pairs, b);
    return hipGetLastError();
}

hipError_t launch_spectrum_list(const uint2 *cnt, const uint2 *rc, uint64_t K, const uint32_t *nh_row, const uint32_t *nh_col, const SpectrumBins &b,
                                unsigned long long *rule, unsigned long long *listed_zero, hipStream_t stream, bool plain)
{
    if (K == 0) return hipSuccess;
    if (b.slots == 0 || (b.slots & (b.slots - 1))) return hipErrorInvalidValue;
    const bool lds = spectrum_lds(b, K, plain);
    const dim3 grid(sp_blocks(K));
    SP_LAUNCH(sp_list_kernel, grid, lds, plain, cnt, rc, K, nh_row, nh_col, b, rule, listed_zero);
    return hipGetLastError();
}

#undef SP_LAUNCH

}  // namespace mg
