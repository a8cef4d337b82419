// screen_finish.hip — gfx950 kernels for the tail of `mash screen` (CommandScreen.cpp:331-455): from the observation
// counters of the slots a mixture touched to the rows the command prints.
//
//   shared  : per observed slot, +1 for every row that holds its key (:338-355); a row's 0 -> 1 transition puts it on the
//             touched-rows list, so that everything per row below (and the clearing) is proportional to that list;
//   winners : (-w, :357-407) per observed slot the holder with the highest (score, length) and the lowest row among
//             equals.  Scores are mg_identity of the counts above, read from a table the host's libm filled (the device's
//             pow is not libm's; the scheme of finish.hip's distance table);
//   group   : the observation counts by row: exclusive scan of the rows' counts, then a scatter through a per-row cursor.
//             The order inside a row is whatever the atomics give; the selection does not depend on it;
//   median  : the count of rank shared / 2 (:409-414) by a radix select, four 8-bit digits from the top, histogram in LDS,
//             straight from global memory: a wave per row, a workgroup for rows above SRF_LONG_ROW counts;
//   rows    : identity from the table, the exact binomial tail of pvalue.h, both filters (:420-434), ordered compaction
//             (ballots, per-segment counts, scan, write) over the per-row counts, so rows come out in row order.
// Holder runs are short for unrelated genomes and hundreds long inside a clade: a lane walks a run of up to SRF_LONG_RUN
// entries itself, longer ones are handed to the whole wave one after the other.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>

#include "pvalue.h"
#include "screen_finish_internal.h"

namespace mg {

constexpr int SRF_NT = 256;
constexpr int SRF_PER = 4;
constexpr int SRF_SEG = SRF_NT * SRF_PER;    // rows per workgroup of the mark / write passes

// the observed slot of work item t: its run [b, e) in ent and its counter; false when there is nothing to walk
__device__ __forceinline__ bool srf_slot(const ScreenFinishArgs &a, uint64_t t, uint32_t &slot, uint32_t &b, uint32_t &e, uint32_t &c)
{
    slot = b = e = c = 0;
    if (t >= a.nt) return false;
    slot = a.touched[t];
    c = a.obs[slot];
    if (c == 0) return false;
    b = slot ? a.slot_end[slot - 1] : 0;
    e = a.slot_end[slot];
    return e > b;
}

// f(row, count) for every holder of every observed slot of this wave's 64 work items (all 64 lanes must arrive)
template <class F>
__device__ __forceinline__ void srf_walk(const ScreenFinishArgs &a, bool live, uint32_t b, uint32_t e, uint32_t c, F f)
{
    const uint32_t lane = threadIdx.x & 63;
    const bool lng = live && e - b > SRF_LONG_RUN;
    if (live && !lng)
        for (uint32_t q = b; q < e; q++) f(a.ent[q], c);
    unsigned long long m = __ballot(lng);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const uint32_t bb = __shfl(b, src), ee = __shfl(e, src), cc = __shfl(c, src);
        for (uint32_t q = bb + lane; q < ee; q += 64) f(a.ent[q], cc);
    }
}

__global__ __launch_bounds__(256) void srf_shared_kernel(ScreenFinishArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t slot, b, e, c;
    const bool live = srf_slot(a, t, slot, b, e, c);
    srf_walk(a, live, b, e, c, [&](uint32_t row, uint32_t) {
        if (row >= a.n) return;
        if (atomicAdd(&a.shared[row], 1u) == 0) {
            const unsigned long long at = atomicAdd(&a.ctr[SRF_CTR_ROWS], 1ull);
            if (at < a.n) a.rows[at] = row;
        }
    });
    unsigned long long len = live ? e - b : 0;                 // the hit total: one add per wave
    for (int d = 32; d > 0; d >>= 1) len += __shfl_xor(len, d);
    if ((threadIdx.x & 63) == 0 && len) atomicAdd(&a.ctr[SRF_CTR_HITS], len);
}

__device__ __forceinline__ uint32_t srf_denom(const ScreenFinishArgs &a, uint32_t row)
{
    const uint32_t d = a.nhash[row];
    return d > a.s ? a.s : d;
}

__device__ __forceinline__ double srf_identity(const ScreenFinishArgs &a, uint32_t x, uint32_t denom)
{
    return a.lut[(uint64_t)a.lut_start[denom] + x];
}

__global__ __launch_bounds__(256) void srf_score_kernel(ScreenFinishArgs a, uint64_t nrows)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    const uint32_t row = a.rows[i];
    a.score[row] = srf_identity(a, a.shared[row], srf_denom(a, row));
}

// the holder that takes a hash: highest score, then larger length, then lower row (scores are positive doubles: their bits
// order as they do)
struct SrfBest {
    unsigned long long score, len;
    uint32_t row;
};

__device__ __forceinline__ bool srf_better(const SrfBest &x, const SrfBest &y)
{
    if (x.score != y.score) return x.score > y.score;
    if (x.len != y.len) return x.len > y.len;
    return x.row < y.row;
}

__global__ __launch_bounds__(256) void srf_winner_kernel(ScreenFinishArgs a)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t slot, b, e, c;
    const bool live = srf_slot(a, t, slot, b, e, c);
    const bool lng = live && e - b > SRF_LONG_RUN;
    auto holder = [&](uint32_t q) {
        SrfBest h;
        h.row = a.ent[q];
        h.score = (unsigned long long)__double_as_longlong(a.score[h.row]);
        h.len = a.lengths[h.row];
        return h;
    };
    uint32_t win = 0xFFFFFFFFu;
    if (live && !lng) {
        SrfBest best = holder(b);
        for (uint32_t q = b + 1; q < e; q++) {
            const SrfBest h = holder(q);
            if (srf_better(h, best)) best = h;
        }
        win = best.row;
    }
    unsigned long long m = __ballot(lng);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const uint32_t bb = __shfl(b, src), ee = __shfl(e, src);
        SrfBest best{0ull, 0ull, 0xFFFFFFFFu};                  // (loses to every holder: a holder of an observed hash scores > 0)
        for (uint32_t q = bb + lane; q < ee; q += 64) {
            const SrfBest h = holder(q);
            if (srf_better(h, best)) best = h;
        }
        for (int d = 32; d > 0; d >>= 1) {
            SrfBest o;
            o.score = __shfl_xor(best.score, d);
            o.len = __shfl_xor(best.len, d);
            o.row = __shfl_xor(best.row, d);
            if (srf_better(o, best)) best = o;
        }
        if ((int)lane == src) win = best.row;
    }
    if (t < a.nt) a.winner_row[t] = win;
    if (win < a.n) atomicAdd(&a.shared_w[win], 1u);
}

__global__ __launch_bounds__(256) void srf_scatter_kernel(ScreenFinishArgs a, uint64_t vals_cap)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t slot, b, e, c;
    const bool live = srf_slot(a, t, slot, b, e, c);
    srf_walk(a, live, b, e, c, [&](uint32_t row, uint32_t count) {
        if (row >= a.n) return;
        const uint64_t at = (uint64_t)a.row_off[row] + atomicAdd(&a.fill[row], 1u);
        if (at < vals_cap) a.vals[at] = count;
    });
}

__global__ __launch_bounds__(256) void srf_scatter_winner_kernel(ScreenFinishArgs a, uint64_t vals_cap)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.nt) return;
    const uint32_t row = a.winner_row[t];
    if (row >= a.n) return;
    const uint64_t at = (uint64_t)a.row_off[row] + atomicAdd(&a.fill[row], 1u);
    if (at < vals_cap) a.vals[at] = a.obs[a.touched[t]];
}

// The element of rank k (0-based, ascending) of v[0 .. cnt), k < cnt, by NT threads: digits of 8 bits from the top; per digit
// a histogram of the elements that match the digits fixed so far, then the first wave finds the bin that holds rank k.
// A digit that is zero in every element (the OR of all says so: counts rarely leave the lowest byte) needs no pass.
template <int NT>
__device__ uint32_t srf_select(const uint32_t *v, uint32_t cnt, uint32_t k, uint32_t *hist, uint32_t *box)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) box[2] = 0;
    __syncthreads();
    uint32_t any = 0;
    for (uint32_t i = tid; i < cnt; i += NT) any |= v[i];
    for (int d = 32; d > 0; d >>= 1) any |= __shfl_xor(any, d);
    if (lane == 0) atomicOr(&box[2], any);
    __syncthreads();
    any = box[2];
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (((any >> shift) & 255u) != 0) {
            for (uint32_t q = tid; q < 256; q += NT) hist[q] = 0;
            __syncthreads();
            for (uint32_t i = tid; i < cnt; i += NT) {
                const uint32_t x = v[i];
                if ((x & mask) == prefix) atomicAdd(&hist[(x >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < 64) {
                uint32_t c[4], sum = 0;
                for (int j = 0; j < 4; j++) { c[j] = hist[lane * 4 + j]; sum += c[j]; }
                uint32_t incl = sum;
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = __shfl_up(incl, d);
                    if ((int)lane >= d) incl += up;
                }
                const uint32_t excl = incl - sum;
                if (k >= excl && k < incl) {
                    uint32_t kk = k - excl, digit = lane * 4;
                    for (int j = 0; j < 3; j++) {
                        if (kk < c[j]) break;
                        kk -= c[j];
                        digit++;
                    }
                    box[0] = digit;
                    box[1] = kk;
                }
            }
            __syncthreads();
            prefix |= box[0] << shift;
            k = box[1];
        }
        mask |= 255u << shift;
    }
    __syncthreads();                                               // (box and hist are free for the caller's next row)
    return prefix;
}

template <int NT, bool LONG>
__global__ __launch_bounds__(NT) void srf_median_kernel(ScreenFinishArgs a, const uint32_t *cnt_of, uint64_t nrows)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t box[4];
    uint64_t todo = nrows;
    if (LONG) { todo = a.ctr[SRF_CTR_LONG]; if (todo > a.n) todo = a.n; }
    for (uint64_t i = blockIdx.x; i < todo; i += gridDim.x) {
        const uint32_t row = LONG ? a.long_rows[i] : a.rows[i];
        const uint32_t cnt = cnt_of[row];
        if (cnt == 0) continue;                                    // (with winner: a touched row that won nothing)
        if (!LONG && cnt > SRF_LONG_ROW) {
            if (threadIdx.x == 0) {
                const unsigned long long at = atomicAdd(&a.ctr[SRF_CTR_LONG], 1ull);
                if (at < a.n) a.long_rows[at] = row;
            }
            continue;
        }
        const uint32_t m = srf_select<NT>(a.vals + a.row_off[row], cnt, cnt / 2, hist, box);
        if (threadIdx.x == 0) a.median[row] = m;
    }
}

// a row's place in the output: candidate, identity filter, p-value filter (CommandScreen.cpp:420-434)
__device__ __forceinline__ bool srf_row_passes(const ScreenFinishArgs &a, const uint32_t *cnt_of, uint64_t row)
{
    const uint32_t x = cnt_of[row];
    if (x == 0 && !a.all_rows) return false;
    const uint32_t denom = srf_denom(a, (uint32_t)row);
    if (srf_identity(a, x, denom) < a.min_identity) return false;
    if (x == 0 || !(a.max_p < 1.0)) return !(1.0 > a.max_p);    // p-values are at most 1; that of x == 0 is 1
    return !(binomial_q((uint64_t)x - 1, a.r, denom) > a.max_p);
}

__global__ __launch_bounds__(SRF_NT) void srf_mark_kernel(ScreenFinishArgs a, const uint32_t *cnt_of)
{
    __shared__ uint32_t wtot[SRF_NT / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t seg = blockIdx.x;
    const uint64_t base = seg * SRF_SEG + (uint64_t)wave * (SRF_PER * 64);
    uint32_t total = 0;
    for (int it = 0; it < SRF_PER; it++) {
        const uint64_t row = base + (uint64_t)it * 64 + lane;
        const bool pass = row < a.n && srf_row_passes(a, cnt_of, row);
        const unsigned long long m = __ballot(pass);
        if (lane == 0) a.masks[(seg * (SRF_NT / 64) + wave) * SRF_PER + it] = m;
        total += (uint32_t)__popcll(m);
    }
    if (lane == 0) wtot[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < SRF_NT / 64; w++) t += wtot[w];
        a.seg_count[seg] = t;
    }
}

__global__ __launch_bounds__(1024) void srf_scan_kernel(const uint32_t *seg_count, unsigned long long *seg_off, uint64_t nseg,
                                                        unsigned long long *total)
{
    __shared__ unsigned long long part[1024];
    const uint64_t per = (nseg + 1023) / 1024;
    const uint64_t b = threadIdx.x * per < nseg ? threadIdx.x * per : nseg, e = b + per < nseg ? b + per : nseg;
    unsigned long long sum = 0;
    for (uint64_t i = b; i < e; i++) sum += seg_count[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned long long x = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += x;
        __syncthreads();
    }
    unsigned long long run = part[threadIdx.x] - sum;
    for (uint64_t i = b; i < e; i++) { seg_off[i] = run; run += seg_count[i]; }
    if (threadIdx.x == 1023) *total = part[1023];
}

__global__ __launch_bounds__(SRF_NT) void srf_write_kernel(ScreenFinishArgs a, const uint32_t *cnt_of)
{
    __shared__ uint32_t wtot[SRF_NT / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t seg = blockIdx.x;
    const uint64_t base = seg * SRF_SEG + (uint64_t)wave * (SRF_PER * 64);
    const unsigned long long *mk = a.masks + (seg * (SRF_NT / 64) + wave) * SRF_PER;
    uint32_t total = 0;
    for (int it = 0; it < SRF_PER; it++) total += (uint32_t)__popcll(mk[it]);
    if (lane == 0) wtot[wave] = total;
    __syncthreads();
    uint64_t pos = a.seg_off[seg];
    for (uint32_t w = 0; w < wave; w++) pos += wtot[w];
    if (pos >= a.out_cap) return;
    for (int it = 0; it < SRF_PER; it++) {
        const unsigned long long mm = mk[it];
        if ((mm >> lane) & 1) {
            const uint64_t at = pos + __popcll(mm & ((1ull << lane) - 1));
            if (at < a.out_cap) {
                const uint64_t row = base + (uint64_t)it * 64 + lane;
                ScreenResult o;
                o.row = (uint32_t)row;
                o.shared = cnt_of[row];
                o.denom = srf_denom(a, (uint32_t)row);
                o.median = o.shared ? a.median[row] : 0;
                o.identity = srf_identity(a, o.shared, o.denom);
                o.p_value = o.shared ? binomial_q((uint64_t)o.shared - 1, a.r, o.denom) : 1.0;
                a.out[at] = o;
            }
        }
        pos += __popcll(mm);
    }
}

__global__ __launch_bounds__(256) void srf_clear_kernel(ScreenFinishArgs a, uint64_t nrows)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    const uint32_t row = a.rows[i];
    a.shared[row] = 0;
    a.shared_w[row] = 0;
    a.fill[row] = 0;
}

uint64_t screen_finish_segments(uint64_t n) { return (n + SRF_SEG - 1) / SRF_SEG; }
uint64_t screen_finish_mask_words(uint64_t n) { return screen_finish_segments(n) * (SRF_NT / 64) * SRF_PER; }

size_t screen_finish_scan_temp_bytes(uint64_t n)
{
    size_t bytes = 0;
    uint32_t *p = nullptr;
    (void)rocprim::exclusive_scan(nullptr, bytes, p, p, 0u, (size_t)n, rocprim::plus<uint32_t>(), (hipStream_t)0);
    return bytes;
}

static dim3 srf_grid(uint64_t items) { return dim3((uint32_t)((items + 255) / 256)); }

hipError_t launch_srf_shared(const ScreenFinishArgs &a, hipStream_t stream)
{
    if (a.nt == 0) return hipSuccess;
    hipLaunchKernelGGL(srf_shared_kernel, srf_grid(a.nt), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_srf_winners(const ScreenFinishArgs &a, uint64_t nrows, hipStream_t stream)
{
    if (a.nt == 0 || nrows == 0) return hipSuccess;
    hipLaunchKernelGGL(srf_score_kernel, srf_grid(nrows), dim3(256), 0, stream, a, nrows);
    hipLaunchKernelGGL(srf_winner_kernel, srf_grid(a.nt), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_srf_offsets(const ScreenFinishArgs &a, bool winner, void *temp, size_t temp_bytes, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    return rocprim::exclusive_scan(temp, temp_bytes, winner ? a.shared_w : a.shared, a.row_off, 0u, (size_t)a.n, rocprim::plus<uint32_t>(), stream);
}

hipError_t launch_srf_scatter(const ScreenFinishArgs &a, bool winner, uint64_t vals_cap, hipStream_t stream)
{
    if (a.nt == 0) return hipSuccess;
    if (winner) hipLaunchKernelGGL(srf_scatter_winner_kernel, srf_grid(a.nt), dim3(256), 0, stream, a, vals_cap);
    else hipLaunchKernelGGL(srf_scatter_kernel, srf_grid(a.nt), dim3(256), 0, stream, a, vals_cap);
    return hipGetLastError();
}

hipError_t launch_srf_medians(const ScreenFinishArgs &a, bool winner, uint64_t nrows, hipStream_t stream)
{
    if (nrows == 0) return hipSuccess;
    const uint32_t *cnt_of = winner ? a.shared_w : a.shared;
    const uint32_t blocks = (uint32_t)(nrows < 16384 ? nrows : 16384);
    hipLaunchKernelGGL((srf_median_kernel<64, false>), dim3(blocks), dim3(64), 0, stream, a, cnt_of, nrows);
    if (a.s > SRF_LONG_ROW)                                        // (a row has at most s counts)
        hipLaunchKernelGGL((srf_median_kernel<256, true>), dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, stream, a, cnt_of, nrows);
    return hipGetLastError();
}

hipError_t launch_srf_rows(const ScreenFinishArgs &a, bool winner, hipStream_t stream)
{
    const uint64_t nseg = screen_finish_segments(a.n);
    if (nseg == 0 || nseg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint32_t *cnt_of = winner ? a.shared_w : a.shared;
    hipLaunchKernelGGL(srf_mark_kernel, dim3((uint32_t)nseg), dim3(SRF_NT), 0, stream, a, cnt_of);
    hipLaunchKernelGGL(srf_scan_kernel, dim3(1), dim3(1024), 0, stream, a.seg_count, a.seg_off, nseg, a.ctr + SRF_CTR_OUT);
    if (a.out_cap) hipLaunchKernelGGL(srf_write_kernel, dim3((uint32_t)nseg), dim3(SRF_NT), 0, stream, a, cnt_of);
    return hipGetLastError();
}

hipError_t launch_srf_clear(const ScreenFinishArgs &a, uint64_t nrows, hipStream_t stream)
{
    if (nrows == 0) return hipSuccess;
    hipLaunchKernelGGL(srf_clear_kernel, srf_grid(nrows), dim3(256), 0, stream, a, nrows);
    return hipGetLastError();
}

}  // namespace mg
