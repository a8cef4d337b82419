// host_spectrum.cpp -- the distance spectrum of a job (include/mashgpu.h: mg_compare_tri_spectrum_host): the distinct {numer, denom}
// of its passing pairs with the number of pairs that have each, binned on the device (spectrum.hip).  Three routes:
//   1  a filter is on: the thresholded counts of cut_counts (lists, or the matrix in row blocks), pass A per piece, one launch that
//      walks its ballots and bins the counts beside the set bits;
//   2  filters off, lists: every list entry binned by its own key and, a second time, by its rule denominator; the pairs NOT on the
//      list are {0, rule denominator} and are counted here, by arithmetic on the rows' hash counts -- no matrix, no fill;
//   3  filters off, no lists: the matrix in row blocks, every count binned.
// The bins live across the pieces of a call.  A key whose denominator is not s goes to a table that starts small; when an entry
// finds no slot the table is enlarged, every bin cleared and the call run again from its first piece.
#include "cut_internal.h"

namespace {

const mg::PairSpace kWholeJob{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};

// the device side of one attempt
struct SpectrumDev {
    DevBuf<unsigned long long> full, keys, vals, rule, ctl;   // ctl: [0] list entries with numer 0, [1] the overflow flag (its low word)
    PassABufs pa;
    DevBuf<unsigned long long> d_count;
    uint64_t slots = 0;
    uint32_t s = 0;
    explicit SpectrumDev(mg_ctx *ctx) : full(ctx), keys(ctx), vals(ctx), rule(ctx), ctl(ctx), pa(ctx), d_count(ctx) {}
    int begin(mg_ctx *ctx, uint32_t s_, uint64_t slots_)
    {
        s = s_;
        slots = slots_;
        if (full.alloc((uint64_t)s + 1) != hipSuccess || rule.alloc((uint64_t)s + 1) != hipSuccess || keys.alloc(slots) != hipSuccess ||
            vals.alloc(slots) != hipSuccess || ctl.alloc(2) != hipSuccess || d_count.alloc(1) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, MG_ERR_NOMEM, "spectrum: device allocation failed");
        }
        HIP_TRY(ctx, hipMemsetAsync(full, 0, ((size_t)s + 1) * 8, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(rule, 0, ((size_t)s + 1) * 8, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(keys, 0xFF, (size_t)slots * 8, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(vals, 0, (size_t)slots * 8, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctl, 0, 16, ctx->stream));
        return MG_OK;
    }
    mg::SpectrumBins bins() const { return mg::SpectrumBins{full, keys, vals, slots, reinterpret_cast<uint32_t *>(ctl.p + 1), s}; }
};

uint64_t pow2_at_least(uint64_t v)
{
    uint64_t p = 4;
    while (p < v) p <<= 1;
    return p;
}

// the distinct values of c[0 .. m) (the rows' clamped hash counts, each <= s) with the number of rows that have each, ascending
std::vector<std::pair<uint32_t, uint64_t>> size_histogram(const uint32_t *c, uint64_t m, uint32_t s)
{
    std::vector<uint64_t> h((size_t)s + 1, 0);
    for (uint64_t i = 0; i < m; i++) h[c[i]]++;
    std::vector<std::pair<uint32_t, uint64_t>> out;
    for (uint32_t v = 0; v <= s; v++)
        if (h[v]) out.push_back({v, h[v]});
    return out;
}

// acc[min(s, a + b)] +/-= the unordered pairs {a, b} of two different rows among the first m of c[]
void add_pairs_within(const std::vector<uint32_t> &c, uint64_t m, uint32_t s, bool subtract, std::vector<uint64_t> &acc)
{
    const auto h = size_histogram(c.data(), m, s);
    for (size_t a = 0; a < h.size(); a++) {
        for (size_t b = a; b < h.size(); b++) {
            const uint64_t n = a == b ? h[a].second * (h[a].second - 1) / 2 : h[a].second * h[b].second;
            const uint64_t d = std::min<uint64_t>(s, (uint64_t)h[a].first + h[b].first);
            if (subtract) acc[d] -= n; else acc[d] += n;     // (what is subtracted is a subset of what was added: no wrap at the end)
        }
    }
}

// Route 2's arithmetic: the pairs of R per rule denominator min(s, |A| + |B|), |X| = min(nhash, s)
int rule_pairs(mg_ctx *ctx, const OutRange &R, std::vector<uint64_t> &acc)
{
    acc.assign((size_t)R.s + 1, 0);
    std::vector<uint32_t> nr(R.re), nc;
    HIP_TRY(ctx, hipMemcpyAsync(nr.data(), R.rows->nhash, (size_t)R.re * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (!R.triangle) {
        nc.resize(R.cols->n);
        HIP_TRY(ctx, hipMemcpyAsync(nc.data(), R.cols->nhash, (size_t)R.cols->n * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t &v : nr) v = std::min(v, R.s);
    for (uint32_t &v : nc) v = std::min(v, R.s);
    if (R.triangle) {
        // rows [rb, re) against everything below them: the pairs inside the first re rows minus those inside the first rb
        add_pairs_within(nr, R.re, R.s, false, acc);
        add_pairs_within(nr, R.rb, R.s, true, acc);
        return MG_OK;
    }
    const auto hq = size_histogram(nr.data() + R.rb, R.re - R.rb, R.s), hr = size_histogram(nc.data(), nc.size(), R.s);
    for (const auto &a : hq)
        for (const auto &b : hr) acc[std::min<uint64_t>(R.s, (uint64_t)a.first + b.first)] += a.second * b.second;
    return MG_OK;
}

// bins in the order of the definition: descending fraction exactly (0/0 as 1/1), equal fractions by ascending denominator
bool bin_before(const mg_spectrum_bin &a, const mg_spectrum_bin &b)
{
    const uint64_t an = a.denom ? a.numer : 1, ad = a.denom ? a.denom : 1, bn = b.denom ? b.numer : 1, bd = b.denom ? b.denom : 1;
    const uint64_t l = an * bd, r = bn * ad;
    return l != r ? l > r : a.denom < b.denom;
}

// One attempt with a table of `slots`: the job's pieces binned into D.  *route as the stats report it.
int spectrum_attempt(mg_ctx *ctx, const OutRange &R, const Cut &cut, SpectrumDev &D, bool plain, uint64_t *route, uint64_t *listed, bool *by_rule)
{
    const mg::SpectrumBins bins = D.bins();
    const Blocks how{1ull << 30, "MASHGPU_SPECTRUM_BLOCK_PAIRS", "spectrum"};
    *by_rule = false;
    *listed = 0;
    if (cut.filtered()) {
        *route = 1;
        CutBufs bufs(ctx, ctx);
        bool cleared = false;
        const int rc = cut_counts(ctx, R, cut, true, how, bufs,
                          [&](uint64_t pairs, uint64_t, uint64_t, bool) { return D.pa.alloc(pairs, R.s) ? MG_OK : kAllocFailed; },
                          [&] { D.pa.release(); },
                          [&](mg::FinishArgs f, const RowBlock &, const CandLists *) -> int {
            if (!cleared) HIP_TRY(ctx, hipMemsetAsync(D.pa.seen, 0, ((size_t)R.s + 1) * 4, ctx->stream));
            cleared = true;
            D.pa.bind(f);
            HIP_TRY(ctx, mg::launch_finish_mark(f, D.d_count, ctx->stream));
            HIP_TRY(ctx, mg::launch_spectrum_marked(f, kWholeJob, bins, ctx->stream, plain));
            return MG_OK;
        });
        if (rc != MG_OK) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // (the pieces' buffers go back to the context behind this wait)
        return MG_OK;
    }
    {
        CandLists L(ctx);
        bool lists = false;
        const int rc = job_cand_lists(ctx, R, L, &lists, [](uint64_t) { return true; });
        if (rc != MG_OK) return rc;
        if (lists) {
            *route = 2;
            *by_rule = true;
            *listed = L.K;
            HIP_TRY(ctx, mg::launch_spectrum_list(L.cnt, L.rc, L.K, R.rows->nhash, R.cols->nhash, bins, D.rule, D.ctl, ctx->stream, plain));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the lists go back to the context behind this wait)
            return MG_OK;
        }
    }
    *route = 3;
    CutBufs bufs(ctx, ctx);
    const int rc = cut_counts(ctx, R, cut, false, how, bufs, [](uint64_t, uint64_t, uint64_t, bool) { return MG_OK; }, [] {},
                      [&](const mg::FinishArgs &f, const RowBlock &, const CandLists *) -> int {
        HIP_TRY(ctx, mg::launch_spectrum_all(f.counts, f.pairs, bins, ctx->stream, plain));
        return MG_OK;
    });
    if (rc != MG_OK) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MG_OK;
}

int spectrum(mg_ctx *ctx, const mg_table *rows, const mg_table *cols, uint64_t rb, uint64_t re, bool triangle, const Cut &cut,
             mg_spectrum_bin *out_host, uint64_t capacity, uint64_t *count_out)
{
    *count_out = 0;
    ctx->spectrum_route = ctx->spectrum_listed = ctx->spectrum_listed_zero = ctx->spectrum_other_keys = ctx->spectrum_regrows = 0;
    OutRange R;
    int rc = out_range(ctx, rows, cols, rb, re, triangle, &R);
    if (rc != MG_OK || R.empty() || !R.pairs) return rc;
    if (cut.k < 1) return fail(ctx, MG_ERR_INVALID, "compare: bad k-mer size");
    const bool plain = ctx_opt(ctx, "MASHGPU_SPECTRUM_PLAIN") != nullptr;
    // the table of the other denominators: 1024 slots to begin with (a test starts it at 4), at most a size that the s (s + 1) / 2 + s
    // keys there can be cannot fill
    const uint64_t max_slots = pow2_at_least((uint64_t)R.s * ((uint64_t)R.s + 1) / 2 + R.s + 1);
    uint64_t slots = 1024;
    if (const char *o = ctx_opt(ctx, "MASHGPU_SPECTRUM_SLOTS")) slots = pow2_at_least(strtoull(o, nullptr, 10));
    slots = std::min(slots, max_slots);
    std::vector<unsigned long long> full((size_t)R.s + 1), rule, keys, vals;
    std::vector<uint64_t> by_denom;
    unsigned long long ctl[2] = {0, 0};
    uint64_t route = 0, listed = 0, regrows = 0;
    for (;;) {
        SpectrumDev D(ctx);
        bool by_rule = false;
        if ((rc = D.begin(ctx, R.s, slots)) != MG_OK) return rc;
        if ((rc = spectrum_attempt(ctx, R, cut, D, plain, &route, &listed, &by_rule)) != MG_OK) return rc;
        keys.resize(slots);
        vals.resize(slots);
        rule.assign(by_rule ? (size_t)R.s + 1 : 0, 0);
        HIP_TRY(ctx, hipMemcpyAsync(ctl, D.ctl, 16, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(full.data(), D.full, full.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(keys.data(), D.keys, slots * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(vals.data(), D.vals, slots * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (by_rule) HIP_TRY(ctx, hipMemcpyAsync(rule.data(), D.rule, rule.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (!(uint32_t)ctl[1]) {
            if (by_rule && (rc = rule_pairs(ctx, R, by_denom)) != MG_OK) return rc;
            break;
        }
        if (slots >= max_slots) return fail(ctx, MG_ERR_HIP, "spectrum: the table of denominators overflowed at its largest size");
        slots = std::min(slots * 4, max_slots);
        regrows++;
    }
    // the bins of equal key from the three sources, added on the host
    std::map<unsigned long long, uint64_t> sum;
    for (uint64_t x = 0; x <= R.s; x++)
        if (full[x]) sum[(unsigned long long)x << 32 | R.s] += full[x];
    for (uint64_t i = 0; i < slots; i++)
        if (keys[i] != mg::CF_NONE && vals[i]) sum[keys[i]] += vals[i];
    for (uint64_t d = 0; d < rule.size(); d++) {
        if (by_denom[d] < rule[d]) return fail(ctx, MG_ERR_HIP, "spectrum: more list entries than pairs at a denominator (the table changed since its index was built?)");
        if (by_denom[d] > rule[d]) sum[(unsigned long long)d] += by_denom[d] - rule[d];
    }
    ctx->spectrum_route = route;
    ctx->spectrum_listed = listed;
    ctx->spectrum_listed_zero = ctl[0];
    ctx->spectrum_regrows = regrows;
    for (const auto &kv : sum) ctx->spectrum_other_keys += (uint32_t)kv.first != R.s;
    *count_out = sum.size();
    if (sum.size() > capacity) return fail(ctx, MG_ERR_NOMEM, "spectrum: more bins than `capacity` (see *count_out)");
    uint64_t n = 0;
    for (const auto &kv : sum) out_host[n++] = mg_spectrum_bin{(uint32_t)(kv.first >> 32), (uint32_t)kv.first, kv.second};
    std::sort(out_host, out_host + n, bin_before);
    return MG_OK;
}

}  // namespace

int mg_compare_tri_spectrum_host(mg_ctx *ctx, const mg_table *t, uint64_t row_begin, uint64_t row_end, int kmer_size, double kmer_space,
                                 double max_distance, double max_p_value, mg_spectrum_bin *out_host, uint64_t capacity, uint64_t *count_out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!t || !count_out || (!out_host && capacity)) return fail(ctx, MG_ERR_INVALID, "mg_compare_tri_spectrum_host: NULL argument");
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    if (cut.max_p >= 0.0 && cut.max_p < 1.0 && (!t->lengths || !t->has_lengths))
        return fail(ctx, MG_ERR_INVALID, "mg_compare_tri_spectrum_host: a p-value filter, and the table carries no lengths");
    return spectrum(ctx, t, t, row_begin, row_end, true, cut, out_host, capacity, count_out);
}

int mg_compare_rect_spectrum_host(mg_ctx *ctx, const mg_table *ref, const mg_table *qry, uint64_t q_begin, uint64_t q_end, int kmer_size,
                                  double kmer_space, double max_distance, double max_p_value, mg_spectrum_bin *out_host, uint64_t capacity,
                                  uint64_t *count_out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!ref || !qry || !count_out || (!out_host && capacity)) return fail(ctx, MG_ERR_INVALID, "mg_compare_rect_spectrum_host: NULL argument");
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    if (cut.max_p >= 0.0 && cut.max_p < 1.0 && (!ref->lengths || !ref->has_lengths || !qry->lengths || !qry->has_lengths))
        return fail(ctx, MG_ERR_INVALID, "mg_compare_rect_spectrum_host: a p-value filter, and the tables carry no lengths");
    return spectrum(ctx, qry, ref, q_begin, q_end, false, cut, out_host, capacity, count_out);
}

int mg_spectrum_stats(mg_ctx *ctx, uint64_t *route_out, uint64_t *listed_out, uint64_t *listed_zero_out, uint64_t *other_keys_out, uint64_t *regrows_out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (route_out) *route_out = ctx->spectrum_route;
    if (listed_out) *listed_out = ctx->spectrum_listed;
    if (listed_zero_out) *listed_zero_out = ctx->spectrum_listed_zero;
    if (other_keys_out) *other_keys_out = ctx->spectrum_other_keys;
    if (regrows_out) *regrows_out = ctx->spectrum_regrows;
    return MG_OK;
}
