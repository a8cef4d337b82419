// knn.hip — `mash triangle -N`: the k nearest neighbours of every sketch of one table, chosen on the device.
//
// The reference has no such option; a record is the reference's record of the unordered pair (CommandTriangle.cpp:159-198 prints
// pair {i, j}, j < i, once) given to both its rows, and the order is topk.hip's on the exact fraction with the NEIGHBOUR INDEX
// as the second key: one order across both sides of the diagonal.
//
// THE MIRROR.  A triangle compares pair {i, j} once; its thresholded candidate list (cand_lists + finish_mark_kernel) holds the
// pair in row i's run only.  Three passes make it symmetric, eligible entries only:
//   degree   deg[row]++ and deg[col]++ per set ballot bit.  The list is row major, so the lanes of a wave mostly share their row:
//            the row side is one atomic per distinct row of the wave (ballot of the lanes that agree with the first one left,
//            until none is left), the column side one atomic per lane -- those go to 64 different rows.
//   scan     exclusive, over n + 1 entries (the last one 0, so base[n] is the total), many workgroups: sums of tiles of 2048, one
//            workgroup over the tile sums, then every tile again with its offset.  32-bit: the host has checked the total.
//   scatter  the degree pass again, an atomic cursor per row instead of the counter: {numer, denom} and the neighbour go to
//            base[row] + place and base[col] + place.
// The order inside a segment is therefore whatever the atomics made it.  Nothing reads it: the selection (topk.hip, KEYED) ranks
// by {fraction, neighbour}, the neighbour is unique within a row, so the order is strict and the k best are one set in one
// order however the segment is laid out; `sel` then names places in the segment, and the finish reads the record there.
//
// Compiles for tools/hipemu too (MG_HIP_EMU, tests/test_knn_emu.py): wave operations sit in wave-uniform control flow.
#include "knn_internal.h"
#ifndef MG_HIP_EMU
#include "pvalue.h"
#endif

namespace mg {

// One wave per ballot word w (entries 64 w .. 64 w + 63), a lane per entry: calls row_side(row, lanes of the wave that share it,
// leader lane) once per distinct row of the word's eligible entries -- every lane of the wave calls it, uniformly -- and
// leaves {row, col} of this lane's entry in rc.  Returns whether this lane's entry is eligible.
template <class RowSide>
__device__ __forceinline__ bool knn_word(const KnnMirror &m, uint64_t w, uint32_t lane, uint2 &rc, RowSide row_side)
{
    const uint64_t idx = w * 64u + lane;
    const bool on = idx < m.K && ((m.masks[w] >> lane) & 1ull);
    rc = on ? m.rc[idx] : make_uint2(0u, 0u);
    unsigned long long left = __ballot(on);                               // (uniform)
    while (left) {
        const uint32_t lead = (uint32_t)__builtin_ctzll(left);
        const uint32_t row = __shfl(rc.x, lead);
        const unsigned long long same = __ballot(on && rc.x == row);
        row_side(row, same, lead);
        left &= ~same;
    }
    return on;
}

__global__ __launch_bounds__(KNN_NT) void knn_degree_kernel(KnnMirror m, uint64_t words)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (KNN_NT / 64u);
    for (uint64_t w = (uint64_t)blockIdx.x * (KNN_NT / 64u) + (threadIdx.x >> 6); w < words; w += waves) {      // (uniform in the wave)
        uint2 rc;
        const bool on = knn_word(m, w, lane, rc, [&](uint32_t row, unsigned long long same, uint32_t lead) {
            if (lane == lead) atomicAdd(&m.deg[row], (uint32_t)__popcll(same));
        });
        if (on) atomicAdd(&m.deg[rc.y], 1u);
    }
}

__global__ __launch_bounds__(KNN_NT) void knn_scatter_kernel(KnnMirror m, uint64_t words)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (KNN_NT / 64u);
    for (uint64_t w = (uint64_t)blockIdx.x * (KNN_NT / 64u) + (threadIdx.x >> 6); w < words; w += waves) {
        uint2 rc;
        uint32_t at_row = 0;
        const bool on = knn_word(m, w, lane, rc, [&](uint32_t row, unsigned long long same, uint32_t lead) {
            uint32_t first = 0;
            if (lane == lead) first = atomicAdd(&m.cur[row], (uint32_t)__popcll(same));
            first = __shfl(first, lead);
            if ((same >> lane) & 1ull) at_row = first + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        });
        if (on) {
            const uint2 c = m.cnt[w * 64u + lane];
            const uint32_t a = m.base[rc.x] + at_row, b = m.base[rc.y] + atomicAdd(&m.cur[rc.y], 1u);
            m.sym_counts[a] = c;
            m.sym_nbr[a] = rc.y;
            m.sym_counts[b] = c;
            m.sym_nbr[b] = rc.x;
        }
    }
}

// ---- the scan of deg[0 .. n] (KNN_SCAN_TILE entries a workgroup, 8 consecutive ones a work-item)

__device__ __forceinline__ uint32_t knn_tile_load(const KnnMirror &m, uint32_t v[8])
{
    const uint64_t first = (uint64_t)blockIdx.x * KNN_SCAN_TILE + threadIdx.x * 8u;
    uint32_t sum = 0;
    for (uint32_t j = 0; j < 8; j++) {
        v[j] = first + j <= m.n ? m.deg[first + j] : 0u;
        sum += v[j];
    }
    return sum;
}

// part[t] -> the sum of part[0 .. t] (inclusive); ends behind a barrier
__device__ __forceinline__ void knn_block_scan(uint32_t *part)
{
    for (uint32_t d = 1; d < KNN_NT; d <<= 1) {
        const uint32_t x = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += x;
        __syncthreads();
    }
}

__global__ __launch_bounds__(KNN_NT) void knn_scan_sums_kernel(KnnMirror m)
{
    __shared__ uint32_t part[KNN_NT];
    uint32_t v[8];
    part[threadIdx.x] = knn_tile_load(m, v);
    __syncthreads();
    knn_block_scan(part);
    if (threadIdx.x == KNN_NT - 1) m.block_sum[blockIdx.x] = part[KNN_NT - 1];
}

// block_sum[0 .. nb) -> its exclusive scan, in place (one workgroup: nb = n / 2048, a few hundred for a million rows)
__global__ __launch_bounds__(KNN_NT) void knn_scan_top_kernel(uint32_t *block_sum, uint32_t nb)
{
    __shared__ uint32_t part[KNN_NT];
    const uint32_t per = (nb + KNN_NT - 1u) / KNN_NT;
    const uint32_t b = threadIdx.x * per < nb ? threadIdx.x * per : nb, e = b + per < nb ? b + per : nb;
    uint32_t sum = 0;
    for (uint32_t i = b; i < e; i++) sum += block_sum[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    knn_block_scan(part);
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t i = b; i < e; i++) { const uint32_t x = block_sum[i]; block_sum[i] = run; run += x; }
}

__global__ __launch_bounds__(KNN_NT) void knn_scan_write_kernel(KnnMirror m)
{
    __shared__ uint32_t part[KNN_NT];
    uint32_t v[8];
    const uint32_t sum = knn_tile_load(m, v);
    part[threadIdx.x] = sum;
    __syncthreads();
    knn_block_scan(part);
    const uint64_t first = (uint64_t)blockIdx.x * KNN_SCAN_TILE + threadIdx.x * 8u;
    uint32_t run = m.block_sum[blockIdx.x] + part[threadIdx.x] - sum;
    for (uint32_t j = 0; j < 8 && first + j <= m.n; j++) { m.base[first + j] = run; run += v[j]; }
}

uint64_t knn_scan_blocks(uint32_t n) { return ((uint64_t)n + 1u + KNN_SCAN_TILE - 1u) / KNN_SCAN_TILE; }

static uint32_t knn_word_blocks(uint64_t words)
{
    const uint64_t blocks = (words + KNN_NT / 64u - 1u) / (KNN_NT / 64u);
    return (uint32_t)(blocks < 16384u ? blocks : 16384u);
}

hipError_t launch_knn_degree(const KnnMirror &m, hipStream_t stream)
{
    if (m.n == 0 || m.n > 0x7FFFFFFFu) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(m.deg, 0, ((size_t)m.n + 1u) * 4u, stream);
    if (e != hipSuccess || m.K == 0) return e;
    const uint64_t words = (m.K + 63u) / 64u;
    hipLaunchKernelGGL(knn_degree_kernel, dim3(knn_word_blocks(words)), dim3(KNN_NT), 0, stream, m, words);
    return hipGetLastError();
}

hipError_t launch_knn_scan(const KnnMirror &m, hipStream_t stream)
{
    if (m.n == 0 || m.n > 0x7FFFFFFFu) return hipErrorInvalidValue;
    const uint32_t nb = (uint32_t)knn_scan_blocks(m.n);
    hipLaunchKernelGGL(knn_scan_sums_kernel, dim3(nb), dim3(KNN_NT), 0, stream, m);
    hipLaunchKernelGGL(knn_scan_top_kernel, dim3(1), dim3(KNN_NT), 0, stream, m.block_sum, nb);
    hipLaunchKernelGGL(knn_scan_write_kernel, dim3(nb), dim3(KNN_NT), 0, stream, m);
    return hipGetLastError();
}

hipError_t launch_knn_scatter(const KnnMirror &m, hipStream_t stream)
{
    if (m.n == 0 || m.n > 0x7FFFFFFFu) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(m.cur, 0, (size_t)m.n * 4u, stream);
    if (e != hipSuccess || m.K == 0) return e;
    const uint64_t words = (m.K + 63u) / 64u;
    hipLaunchKernelGGL(knn_scatter_kernel, dim3(knn_word_blocks(words)), dim3(KNN_NT), 0, stream, m, words);
    return hipGetLastError();
}

#ifndef MG_HIP_EMU
__global__ __launch_bounds__(256) void knn_clear_self_kernel(unsigned long long *masks, uint32_t nrows, uint64_t ncols, uint64_t first_row)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const uint64_t idx = (uint64_t)r * ncols + first_row + r;
    atomicAnd(&masks[idx >> 6], ~(1ull << (idx & 63u)));                  // (two rows' bits can share a word)
}

// one work-item per slot (row, j) of the selection
__global__ __launch_bounds__(256) void knn_finish_kernel(FinishArgs f, TopkArgs a, const uint32_t *sym_nbr, const unsigned long long *row_off, FinishEdge *out)
{
    const unsigned long long slots = (unsigned long long)a.nrows * a.k, stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < slots; t += stride) {
        const uint32_t r = (uint32_t)(t / a.k), j = (uint32_t)(t % a.k);
        if (j >= a.row_n[r]) continue;
        const uint32_t idx = a.sel[t];
        const uint2 c = a.counts[idx];
        const uint64_t row = f.first_row + r, col = sym_nbr[idx];
        const uint64_t hi = row > col ? row : col, lo = row > col ? col : row;      // the triangle's own order of the pair
        FinishEdge e;
        e.row = (uint32_t)row;
        e.col = (uint32_t)col;
        e.numer = c.x;
        e.denom = c.y;
        e.distance = lut_distance(f, c.x, c.y);
        e.p_value = p_value(c.x, f.len_row[hi], f.len_col[lo], f.kmer_space, c.y);
        out[row_off[r] + j] = e;
    }
}

hipError_t launch_knn_clear_self(unsigned long long *masks, uint32_t nrows, uint64_t ncols, uint64_t first_row, hipStream_t stream)
{
    if (nrows == 0) return hipSuccess;
    if (first_row + nrows > ncols) return hipErrorInvalidValue;           // (a row's own column lies inside its row)
    hipLaunchKernelGGL(knn_clear_self_kernel, dim3((nrows + 255u) / 256u), dim3(256), 0, stream, masks, nrows, ncols, first_row);
    return hipGetLastError();
}

hipError_t launch_knn_finish(const FinishArgs &f, const TopkArgs &a, const uint32_t *sym_nbr, const unsigned long long *row_off, FinishEdge *out,
                             hipStream_t stream)
{
    const unsigned long long slots = (unsigned long long)a.nrows * a.k;
    if (slots == 0) return hipSuccess;
    unsigned long long blocks = (slots + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(knn_finish_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, f, a, sym_nbr, row_off, out);
    return hipGetLastError();
}
#endif  // !MG_HIP_EMU

}  // namespace mg
