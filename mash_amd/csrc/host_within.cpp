// host_within.cpp -- `mash within` on the device: the two entry points over within.hip.  The matrix is cut in row blocks as for
// the compare outputs (cut_internal.h), and the thresholded call compacts its survivors with the filter passes of compare.hip:
// the j pass leaves {0, j} per pair, the filter's integer table says which j pass.
#include "cut_internal.h"
#include "within_internal.h"

// The smallest j >= 1 whose error bound 1 / sqrt(j) (CommandContain.cpp:260) is at most max_error; 0: no j passes.  The bound
// falls as j grows, so the device's `j >= j_min` keeps exactly the pairs writeOutput's `error <= threshold` keeps (:188).
static uint64_t within_j_min(double max_error)
{
    if (!(max_error > 0.0)) return 0;                                     // (NaN too)
    if (max_error >= 1.0) return 1;
    const double guess = std::ceil(1.0 / (max_error * max_error));
    if (!(guess < 1.8e19)) return 0;                                      // (beyond any sketch)
    uint64_t j = std::max<uint64_t>((uint64_t)guess, 1);
    auto pass = [&](uint64_t x) { return 1.0 / std::sqrt((double)x) <= max_error; };
    while (j > 1 && pass(j - 1)) j--;
    while (!pass(j)) j++;
    return j;
}

static mg::WithinArgs within_args(const OutRange &R, const RowBlock &b, const unsigned long long *last, uint32_t j_min, mg_counts *counts)
{
    mg::WithinArgs a{};
    a.ref = R.cols->hashes;
    a.qry = R.rows->hashes;
    a.ref_n = R.cols->nhash;
    a.qry_n = R.rows->nhash;
    a.ref_s = R.cols->s;
    a.qry_s = R.rows->s;
    a.nref = R.cols->n;
    a.first_q = b.r;
    a.pairs = b.pairs;
    a.ref_last = const_cast<unsigned long long *>(last);
    a.j_min = j_min;
    a.counts = reinterpret_cast<uint2 *>(counts);
    return a;
}

// What both calls do first: the range (rows = queries, cols = references), its blocks, the references' largest hashes
struct WithinJob {
    OutRange R;
    std::vector<RowBlock> blocks;
    uint64_t largest = 0;
    DevBuf<unsigned long long> last;
    DevBuf<mg_counts> counts;
    explicit WithinJob(mg_ctx *ctx) : last(ctx), counts(nullptr) {}       // (a block's counts, up to 8 GiB, stay out of the context's cache)
};

static int within_open(mg_ctx *ctx, const mg_table *ref, const mg_table *qry, uint64_t qb, uint64_t qe, uint64_t block_pairs, WithinJob &J)
{
    int rc = out_range(ctx, qry, ref, qb, qe, false, &J.R);
    if (rc != MG_OK || !J.R.pairs) return rc;
    if (ref->n > 0x7FFFFFFFull) return fail(ctx, MG_ERR_UNSUPPORTED, "within: too many references");
    if (const char *o = ctx_opt(ctx, "MASHGPU_OUT_BLOCK_PAIRS")) block_pairs = std::min(std::max<uint64_t>(1, strtoull(o, nullptr, 10)), block_pairs);
    J.blocks = row_blocks(J.R, block_pairs, &J.largest);
    if (J.last.alloc(ref->n) != hipSuccess || J.counts.alloc(J.largest) != hipSuccess)
        return fail(ctx, MG_ERR_NOMEM, "within: device allocation failed");
    mg::WithinArgs a = within_args(J.R, J.blocks[0], J.last, 0, J.counts);
    HIP_TRY(ctx, mg::launch_within_last(a, ctx->stream));
    return MG_OK;
}

int mg_within_rect_host(mg_ctx *ctx, const mg_table *ref, const mg_table *qry, uint64_t q_begin, uint64_t q_end, mg_counts *out_host)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!ref || !qry || !out_host) return fail(ctx, MG_ERR_INVALID, "mg_within_rect_host: NULL argument");
    WithinJob J(ctx);
    const int rc = within_open(ctx, ref, qry, q_begin, q_end, 1ull << 27, J);      // 1 GiB of {common, j}
    if (rc != MG_OK || !J.R.pairs) return rc;
    for (const RowBlock &b : J.blocks) {
        const mg::WithinArgs a = within_args(J.R, b, J.last, 0, J.counts);
        HIP_TRY(ctx, mg::launch_within_j(a, ctx->stream));
        HIP_TRY(ctx, mg::launch_within_count(a, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(out_host + b.before, J.counts, b.pairs * sizeof(mg_counts), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MG_OK;
}

int mg_within_rect_results_host(mg_ctx *ctx, const mg_table *ref, const mg_table *qry, uint64_t q_begin, uint64_t q_end, double max_error,
                                mg_edge *out_host, uint64_t capacity, uint64_t *count_out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!ref || !qry || !count_out || (!out_host && capacity)) return fail(ctx, MG_ERR_INVALID, "mg_within_rect_results_host: NULL argument");
    *count_out = 0;
    const uint64_t j_min = within_j_min(max_error);
    if (j_min == 0 || j_min > std::min(ref->s, qry->s)) return MG_OK;    // no pair can pass: j <= min(|R|, |Q|)
    WithinJob J(ctx);
    int rc = within_open(ctx, ref, qry, q_begin, q_end, 1ull << 30, J);
    if (rc != MG_OK || !J.R.pairs) return rc;

    // the filter's table by j (its `denom`): the j pass leaves numer = 0, so 0 passes and anything above it fails
    std::vector<uint32_t> min_numer((size_t)J.R.s + 1, 0xFFFFFFFFu);
    std::fill(min_numer.begin() + j_min, min_numer.end(), 0u);
    const uint64_t window = 1ull << 26, nseg_max = mg::filter_segments(J.largest);
    DevBuf<uint32_t> d_min(ctx), d_segc(ctx);
    DevBuf<unsigned long long> d_sego(ctx), d_n(ctx);
    DevBuf<uint4> d_edges;
    if (d_min.alloc(min_numer.size()) != hipSuccess || d_n.alloc(1) != hipSuccess || d_segc.alloc(nseg_max) != hipSuccess ||
        d_sego.alloc(nseg_max) != hipSuccess || d_edges.alloc(std::min(J.largest, window)) != hipSuccess)
        return fail(ctx, MG_ERR_NOMEM, "within: device allocation failed");
    HIP_TRY(ctx, hipMemcpyAsync(d_min, min_numer.data(), min_numer.size() * 4, hipMemcpyHostToDevice, ctx->stream));

    Room room{capacity};
    for (const RowBlock &b : J.blocks) {
        mg::WithinArgs a = within_args(J.R, b, J.last, (uint32_t)j_min, J.counts);
        mg::FilterArgs f;
        f.counts = a.counts;
        f.min_numer = d_min;
        f.seg_count = d_segc;
        f.seg_off = d_sego;
        f.edges = d_edges;
        f.pairs = b.pairs;
        f.first_row = b.r;
        f.ncols = J.R.cols->n;
        f.win_lo = 0; f.win_n = 0;
        f.s = J.R.s;
        f.triangle = 0;
        unsigned long long n_blk = 0;
        HIP_TRY(ctx, mg::launch_within_j(a, ctx->stream));
        HIP_TRY(ctx, mg::launch_filter_count(f, d_n, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&n_blk, d_n, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        // survivors rank in reference order; nothing more is counted or copied once `capacity` is exceeded
        for (uint64_t lo = 0; lo < n_blk && n_blk <= room.left(); lo += window) {
            f.win_lo = lo;
            f.win_n = std::min<uint64_t>(window, n_blk - lo);
            a.edges = d_edges;
            a.nedges = f.win_n;
            HIP_TRY(ctx, mg::launch_filter_write(f, ctx->stream));
            HIP_TRY(ctx, mg::launch_within_count_list(a, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(room.at(out_host) + lo, d_edges, f.win_n * sizeof(mg_edge), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        room.total += n_blk;
    }
    *count_out = room.total;
    if (room.total > capacity) return fail(ctx, MG_ERR_NOMEM, "within: more passing pairs than `capacity` (see *count_out)");
    return MG_OK;
}
