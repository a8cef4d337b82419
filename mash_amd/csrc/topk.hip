// topk.hip — `mash dist -N`: the k nearest references of every query, chosen on the device.
//
// The reference has no such option; every record is still the reference's record of that pair (CommandDistance.cpp:387-424,
// the tail of compareSketches) and the order is defined on the exact fraction it prints in column 5 (:289, "numer/denom"):
//   pair a ranks before pair b  iff  numer_a * denom_b > numer_b * denom_a   (64-bit integers),
//   equal fractions by ascending reference index.
//
// THE KEY.  No scalar key is used.  A float32 of numer / denom merges 4999/9999 with 5000/10001 (they differ by 2e-8 of
// their value, a float32 resolves 6e-8), a 32-bit fixed-point quotient fails as soon as two fractions are closer than 2^-32,
// which denominators beyond 65 535 allow (1/(d(d-1)) < 2^-32).  Every comparison here is the cross-multiplication itself:
// numer <= denom <= s < 2^32, so both products fit 64 bits without overflow and the comparison is exact for every s the
// library accepts.  denom == 0 (two empty sketches) implies numer == 0; such a pair is compared as 0/1, which makes "a zero
// numerator ranks as zero whatever its denominator" hold against every other pair and keeps the order total and transitive
// (the bare products would tie 0/0 with everything).  The second key is the pair's position in its row segment: both layouts
// (a matrix row, a row of the candidate lists) hold a row's pairs in column order, so position order IS reference-index order,
// and it is unique -- the order is strict, any sorting network realises it, and a tie across the k-th place is cut in column
// order by the same comparison, not by a separate pass.
// THE KEYED FORM (template parameter KEYED, launch_topk_select_keyed; knn.hip's mirrored triangle): the second key is key[idx],
// unique within a row, read beside the counts -- a segment may then hold its pairs in ANY order and the answer is the same.  The
// long kernel keeps the position beside the key (one more uint32_t[TOPK_BUF] of LDS, 32 KB in all) to report `sel`.  KEYED = false
// is the code above and below unchanged: no key array is declared or touched.
//
// SELECTION, short segments (topk_select_short_kernel, a wave per row of up to 64 pairs): see the kernel.
// SELECTION, long segments (topk_select_kernel, one workgroup of 256 per row).  The row is streamed once, coalesced, 1024 pairs at a time.
// LDS holds up to 2048 entries {numer, denom, position}: the best <= k seen so far and what the chunks appended since the last
// prune.  A pair is appended iff its eligibility bit is set and -- once k pairs are known -- it ranks before the k-th of them
// (the bound); ballots and one LDS atomic per wave give the places.  When fewer than 1024 places are left (or the first k
// pairs have arrived and no bound is known yet) the buffer is sorted by a bitonic network over the next power of two, cut to
// k, and the bound is renewed.  On rows whose pairs mostly share nothing -- the serving shape -- nearly all pairs fail the
// bound: a pair 0/x never ranks before an earlier 0/y.  The end of the row sorts once more and writes the row's list.
//
// FINISH (topk_finish_kernel).  Distance (the host-libm table of finish.hip) and p-value (pvalue.h) for the selected records
// only, by the very device functions the other outputs use: the doubles are bit-equal to mg_compare_rect_pairs_host's.
//
// Compiles for tools/hipemu too (MG_HIP_EMU, tests/test_topk_emu.py): a workgroup that uses barriers leaves as a whole, wave operations sit in
// uniform control flow, nothing relies on the lock step of a wave.
#include "topk_internal.h"
#ifndef MG_HIP_EMU
#include "pvalue.h"
#endif

namespace mg {

struct TopkEnt { uint32_t numer, denom, pos; };

// a ranks strictly before b (see THE KEY)
__device__ __forceinline__ bool topk_before(const TopkEnt &a, const TopkEnt &b)
{
    const unsigned long long l = (unsigned long long)a.numer * (b.denom ? b.denom : 1u);
    const unsigned long long r = (unsigned long long)b.numer * (a.denom ? a.denom : 1u);
    return l > r || (l == r && a.pos < b.pos);
}

// buf[0 .. n) -> sorted best first, by a bitonic network over P = the power of two >= n (places n .. P filled with an entry that
// ranks after every real one).  Uniform: every work-item calls it with the same n.  Ends behind a barrier.
template <bool KEYED>
__device__ void topk_sort(uint32_t *bn, uint32_t *bd, uint32_t *bp, uint32_t *bq, uint32_t n)
{
    uint32_t P = 2;
    while (P < n) P <<= 1;
    for (uint32_t i = n + threadIdx.x; i < P; i += TOPK_NT) { bn[i] = 0; bd[i] = 1; bp[i] = 0xFFFFFFFFu; }
    __syncthreads();
    for (uint32_t size = 2; size <= P; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = threadIdx.x; t < P / 2; t += TOPK_NT) {
                const uint32_t i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i + stride;
                const TopkEnt x{bn[i], bd[i], bp[i]}, y{bn[j], bd[j], bp[j]};
                const bool up = (i & size) == 0;                       // this run ends best first
                if (up ? topk_before(y, x) : topk_before(x, y)) {
                    bn[i] = y.numer; bd[i] = y.denom; bp[i] = y.pos;
                    bn[j] = x.numer; bd[j] = x.denom; bp[j] = x.pos;
                    if constexpr (KEYED) { const uint32_t q = bq[i]; bq[i] = bq[j]; bq[j] = q; }
                }
            }
            __syncthreads();
        }
}

// Short segments (n <= TOPK_SHORT = 64, most rows of a candidate list): a wave per row, a lane per pair, no LDS and no barrier.
// A pair's place in the row's list is the number of eligible pairs that rank before it -- the order is strict, so the places of
// the eligible pairs are 0, 1, 2, ... without a gap -- and the pairs with a place below k are the answer.
template <bool KEYED>
__global__ __launch_bounds__(TOPK_NT) void topk_select_short_kernel(TopkArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * (TOPK_NT / 64u) + (threadIdx.x >> 6);
    const bool live = row < a.nrows;                                      // (uniform in the wave, as all that depends on the row)
    const uint32_t n = !live ? 0u : a.seg_cnt ? a.seg_cnt[row] : a.ncols;
    if (n > TOPK_SHORT) return;                                           // a long row: topk_select_kernel's
    const unsigned long long begin = !live ? 0ull : a.seg_base ? a.seg_base[row] : (unsigned long long)row * a.ncols;
    TopkEnt e{0, 1, lane};
    bool elig = lane < n;
    if (elig) {
        const unsigned long long idx = begin + lane;
        const uint2 c = a.counts[idx];
        e.numer = c.x;
        e.denom = c.y;
        if (a.masks) elig = (a.masks[idx >> 6] >> (idx & 63u)) & 1ull;
        if constexpr (KEYED) e.pos = a.key[idx];
    }
    uint32_t place = 0;
    for (uint32_t l = 0; l < n; l++) {
        const TopkEnt o{__shfl(e.numer, l), __shfl(e.denom, l), KEYED ? __shfl(e.pos, l) : l};
        const uint32_t oe = __shfl((uint32_t)elig, l);
        if (oe && topk_before(o, e)) place++;
    }
    const unsigned long long m = __ballot(elig);
    if (elig && place < a.k) {
        a.sel[(unsigned long long)row * a.k + place] = (uint32_t)(begin + lane);
        if (a.denom_seen && e.denom <= a.s) a.denom_seen[e.denom] = 1u;
    }
    if (live && lane == 0) {
        const uint32_t c = (uint32_t)__popcll(m);
        a.row_n[row] = c < a.k ? c : a.k;
    }
}

template <bool KEYED>
__global__ __launch_bounds__(TOPK_NT) void topk_select_kernel(TopkArgs a)
{
    __shared__ uint32_t bn[TOPK_BUF], bd[TOPK_BUF], bp[TOPK_BUF];
    __shared__ uint32_t bq[KEYED ? TOPK_BUF : 1];                         // KEYED: bp holds the key, bq the position
    __shared__ uint32_t fill;                                             // entries in the buffer
    const uint32_t row = blockIdx.x, lane = threadIdx.x & 63u;
    const unsigned long long begin = a.seg_base ? a.seg_base[row] : (unsigned long long)row * a.ncols;
    const uint32_t n = a.seg_cnt ? a.seg_cnt[row] : a.ncols;
    if (n <= TOPK_SHORT) return;                                          // (uniform) a short row: topk_select_short_kernel's
    if (threadIdx.x == 0) fill = 0;
    __syncthreads();
    bool bounded = false;
    TopkEnt bound{0, 1, 0};
    for (uint32_t c0 = 0; c0 < n; c0 += TOPK_CHUNK) {                     // (uniform)
        uint2 c[4];
        uint32_t key[KEYED ? 4 : 1];
        bool take[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {                                     // four loads in flight per lane
            const uint32_t pos = c0 + (uint32_t)j * TOPK_NT + threadIdx.x;
            take[j] = pos < n;
            c[j] = make_uint2(0, 1);
            if (take[j]) {
                const unsigned long long idx = begin + pos;
                c[j] = a.counts[idx];
                if (a.masks) take[j] = (a.masks[idx >> 6] >> (idx & 63u)) & 1ull;
                if constexpr (KEYED) key[j] = a.key[idx];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t pos = c0 + (uint32_t)j * TOPK_NT + threadIdx.x;
            TopkEnt e{c[j].x, c[j].y, pos};
            if constexpr (KEYED) e.pos = take[j] ? key[j] : 0u;
            const bool t = take[j] && (!bounded || topk_before(e, bound));
            const unsigned long long m = __ballot(t);
            uint32_t at = 0;
            if (lane == 0 && m) at = atomicAdd(&fill, (uint32_t)__popcll(m));
            at = __shfl(at, 0u);
            if (t) {
                at += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                bn[at] = e.numer; bd[at] = e.denom; bp[at] = e.pos;
                if constexpr (KEYED) bq[at] = pos;
            }
        }
        __syncthreads();
        const uint32_t f = fill;
        __syncthreads();                                                  // (nobody adds to `fill` before all have read it)
        if (f > TOPK_BUF - TOPK_CHUNK || (!bounded && f >= a.k)) {        // (uniform) prune: sort, keep k, renew the bound
            topk_sort<KEYED>(bn, bd, bp, bq, f);
            if (f >= a.k) {
                bounded = true;
                bound = TopkEnt{bn[a.k - 1], bd[a.k - 1], bp[a.k - 1]};
            }
            __syncthreads();                                              // (the bound is read before the buffer changes)
            if (threadIdx.x == 0) fill = f < a.k ? f : a.k;
            __syncthreads();
        }
    }
    const uint32_t f = fill;
    __syncthreads();
    if (f > 1) topk_sort<KEYED>(bn, bd, bp, bq, f);
    const uint32_t keep = f < a.k ? f : a.k;
    for (uint32_t j = threadIdx.x; j < keep; j += TOPK_NT) {
        a.sel[(unsigned long long)row * a.k + j] = (uint32_t)(begin + (KEYED ? bq[j] : bp[j]));
        if (a.denom_seen && bd[j] <= a.s) a.denom_seen[bd[j]] = 1u;
    }
    if (threadIdx.x == 0) a.row_n[row] = keep;
}

template <bool KEYED>
static hipError_t topk_select_launch(const TopkArgs &a, hipStream_t stream)
{
    if (a.nrows == 0) return hipSuccess;
    if (a.k == 0 || a.k > TOPK_MAX || a.nrows > 0x7FFFFFFFu) return hipErrorInvalidValue;
    // a matrix block has rows of one length; a candidate list has both kinds, and each kernel leaves the other's rows alone
    if (a.seg_cnt || a.ncols <= TOPK_SHORT)
        hipLaunchKernelGGL(topk_select_short_kernel<KEYED>, dim3((a.nrows + TOPK_NT / 64u - 1u) / (TOPK_NT / 64u)), dim3(TOPK_NT), 0, stream, a);
    if (a.seg_cnt || a.ncols > TOPK_SHORT)
        hipLaunchKernelGGL(topk_select_kernel<KEYED>, dim3(a.nrows), dim3(TOPK_NT), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_topk_select(const TopkArgs &a, hipStream_t stream) { return topk_select_launch<false>(a, stream); }

hipError_t launch_topk_select_keyed(const TopkArgs &a, hipStream_t stream)
{
    if (!a.key || !a.seg_base || !a.seg_cnt) return hipErrorInvalidValue;
    return topk_select_launch<true>(a, stream);
}

#ifndef MG_HIP_EMU
__global__ __launch_bounds__(1024) void topk_scan_kernel(const uint32_t *row_n, unsigned long long *row_off, uint32_t nrows, unsigned long long *total)
{
    __shared__ unsigned long long part[1024];
    const uint32_t per = (nrows + 1023u) / 1024u;
    const uint32_t b = threadIdx.x * per < nrows ? threadIdx.x * per : nrows, e = b + per < nrows ? b + per : nrows;
    unsigned long long sum = 0;
    for (uint32_t i = b; i < e; i++) sum += row_n[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned long long x = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += x;
        __syncthreads();
    }
    unsigned long long run = part[threadIdx.x] - sum;
    for (uint32_t i = b; i < e; i++) { row_off[i] = run; run += row_n[i]; }
    if (threadIdx.x == 1023) *total = part[1023];
}

// one work-item per slot (row, j) of the selection
__global__ __launch_bounds__(256) void topk_finish_kernel(FinishArgs f, TopkArgs a, const unsigned long long *row_off, FinishEdge *out)
{
    const unsigned long long slots = (unsigned long long)a.nrows * a.k, stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < slots; t += stride) {
        const uint32_t r = (uint32_t)(t / a.k), j = (uint32_t)(t % a.k);
        if (j >= a.row_n[r]) continue;
        const uint32_t idx = a.sel[t];
        const uint2 c = f.counts[idx];
        uint64_t row, col;
        if (f.list_rc) {
            const uint2 rc = f.list_rc[idx];
            row = rc.x;
            col = rc.y;
        } else {
            row = f.first_row + r;
            col = idx - (uint64_t)r * a.ncols;
        }
        FinishEdge e;
        e.row = (uint32_t)row;
        e.col = (uint32_t)col;
        e.numer = c.x;
        e.denom = c.y;
        e.distance = lut_distance(f, c.x, c.y);
        e.p_value = p_value(c.x, f.len_row[row], f.len_col[col], f.kmer_space, c.y);
        out[row_off[r] + j] = e;
    }
}

hipError_t launch_topk_scan(const uint32_t *row_n, unsigned long long *row_off, uint32_t nrows, unsigned long long *total, hipStream_t stream)
{
    hipLaunchKernelGGL(topk_scan_kernel, dim3(1), dim3(1024), 0, stream, row_n, row_off, nrows, total);
    return hipGetLastError();
}

hipError_t launch_topk_finish(const FinishArgs &f, const TopkArgs &a, const unsigned long long *row_off, FinishEdge *out, hipStream_t stream)
{
    const unsigned long long slots = (unsigned long long)a.nrows * a.k;
    if (slots == 0) return hipSuccess;
    unsigned long long blocks = (slots + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(topk_finish_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, f, a, row_off, out);
    return hipGetLastError();
}
#endif  // !MG_HIP_EMU

}  // namespace mg
