// host_reads.cpp -- reads mode (-r with -m, -c, -b): the event kernel on the device, the reference's heap on the host;
// sessions fed chunk by chunk, and mg_sketch_reads_host over one
#include "host_internal.h"

namespace {

// MinHashHeap::tryInsert (MinHashHeap.cpp:68-145) over explicit containers: kept hashes with
// counts, pending hashes (multiplicityMinimum > 1) and the pending max-queue that may hold hashes
// already erased from the pending set; with -b, the Bloom filter in front of the kept set.
//
// The filter (MinHashHeap.cpp:19-41: vendored bloom_filter.hpp with projected_element_count 1e9,
// false_positive_probability 0, maximum_size = bytes * 8): probability 0 makes
// compute_optimal_parameters (bloom_filter.hpp:107-155) pick one hash function and cast -inf to
// the table size, which x86-64 builds turn into 2^63 and the clamp into maximum_size -- ONE hash
// over bytes * 8 bits.  Salt :449-508 (salt_count 1), hash_ap :526-568 over the hash's 8 or 4
// bytes, bit = hash % table_size :443-447.
struct ReadsBloom {
    std::vector<uint8_t> bits;
    uint64_t nbits = 0;
    bool use64 = true;
    void init(uint64_t bytes, bool u64)
    {
        nbits = bytes * 8;
        use64 = u64;
        bits.assign((size_t)std::min<uint64_t>(bytes, 1ull << 29), 0);   // a 32-bit hash stays below bit 2^32
    }
    uint64_t bit_of(uint64_t hash) const
    {
        const uint64_t seed = 0xA5A5A5A55A5A5A5Aull * 0xA5A5A5A5ull + 1ull;     // random_seed_
        uint32_t h = 0xAAAAAAAAu * 0xAAAAAAAAu + (uint32_t)seed;                // the filter's only salt
        if (use64) {
            const uint32_t w0 = (uint32_t)hash, w1 = (uint32_t)(hash >> 32);
            h ^= (h << 7) ^ (w0 * (h >> 3)) ^ (~((h << 11) + (w1 ^ (h >> 5))));
        } else {
            h ^= ~((h << 11) + ((uint32_t)hash ^ (h >> 5)));
        }
        return (uint64_t)h % nbits;
    }
    bool test_and_set(uint64_t hash)                        // contains ? true : (insert, false)
    {
        const uint64_t b = bit_of(hash);
        const uint8_t m = (uint8_t)(1u << (b & 7));
        if (bits[b >> 3] & m) return true;
        bits[b >> 3] |= m;
        return false;
    }
};

struct ReadsHeap {
    uint64_t cap, mmin;
    std::map<uint64_t, uint32_t> kept;
    std::map<uint64_t, uint32_t> pending;
    std::priority_queue<uint64_t> pending_q;
    uint64_t msum = 0;                                       // multiplicitySum
    ReadsBloom bloom;                                        // nbits == 0: none

    ReadsHeap(uint64_t s, uint64_t m) : cap(s), mmin(m < 1 ? 1 : m) {}
    bool full() const { return kept.size() >= cap; }
    uint64_t top() const { return kept.rbegin()->first; }
    double multiplicity() const { return kept.empty() ? 0.0 : (double)msum / (double)kept.size(); }   // MinHashHeap.h:44

    void try_insert(uint64_t h)
    {
        if (!(kept.size() < cap || h < top())) return;       // :70-74
        auto it = kept.find(h);
        if (it != kept.end()) {                              // :120-124
            it->second++;
            msum++;
        } else if (bloom.nbits) {                            // :78-94
            if (bloom.test_and_set(h)) {
                kept.emplace(h, 2u);
                msum += 2;
            }
        } else {
            auto pit = pending.find(h);
            const uint64_t pc = pit == pending.end() ? 0 : pit->second;
            if (mmin == 1 || pc == mmin - 1) {               // :96-109
                kept.emplace(h, (uint32_t)mmin);
                msum += mmin;
                if (mmin > 1 && pit != pending.end()) pending.erase(pit);
            } else {                                         // :110-118
                if (pit == pending.end()) { pending_q.push(h); pending.emplace(h, 1u); }
                else pit->second++;
            }
        }
        if (kept.size() > cap) {                             // :126-144
            auto last = std::prev(kept.end());
            const uint64_t tv = last->first;
            msum -= last->second;
            kept.erase(last);
            while (!pending_q.empty() && tv < pending_q.top()) {
                pending.erase(pending_q.top());
                pending_q.pop();
            }
        }
    }
};

}  // namespace

// Reads mode as a SESSION: chunks of whole records in reading order; the heap (incl. the -m pending
// set) lives on the host between chunks, the device sees one chunk at a time, and with -c the caller
// stops reading its files the moment a chunk reports the target coverage.  Host and device memory are
// bounded by one chunk for EVERY reads option (-r, -m, -c, -b): what the reference's reader loop does
// (Sketch.cpp:1196-1270), where mg_sketch_host / mg_sketch_begin keep the whole read set in HBM.
struct mg_reads_session {
    mg_ctx *ctx = nullptr;
    mg_params p;
    int mode = 0;
    ReadsHeap heap;
    bool stopped = false;
    uint64_t used = 0;                  // records consumed when the stop occurred
    uint64_t records = 0;               // records (>= k) seen so far
    double shrink = 1.0;
    DevBuf<uint8_t> d_bases, d_alpha;   // (no pool: the event buffer outlives calls)
    uint64_t d_cap = 0;
    DevBuf<mg::HashEvent> d_ev;
    DevBuf<unsigned long long> d_cnt;
    std::vector<mg::HashEvent> ev;
    mg_reads_session(uint64_t s, uint64_t m) : heap(s, m) {}
};

static const uint64_t kReadsEventCap = 1ull << 23;           // events per pass (128 MiB)

int mg_reads_begin(mg_ctx *ctx, const mg_params *p, mg_reads_session **out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!p || !out) return fail(ctx, MG_ERR_INVALID, "mg_reads_begin: NULL argument");
    int mode = 0;
    const int rc = sketch_check_params(ctx, p, "mg_reads_begin", true, &mode);
    if (rc != MG_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    mg_reads_session *rs = new mg_reads_session(p->sketch_size, p->min_copies);
    rs->ctx = ctx;
    rs->p = *p;
    rs->mode = mode;
    if (p->bloom_bytes) {
        try { rs->heap.bloom.init(p->bloom_bytes, p->use64 != 0); }
        catch (const std::bad_alloc &) { delete rs; return fail(ctx, MG_ERR_NOMEM, "mg_reads_begin: the Bloom filter does not fit in host memory"); }
    }
    if (rs->d_alpha.alloc(256) != hipSuccess || rs->d_ev.alloc(kReadsEventCap) != hipSuccess || rs->d_cnt.alloc(1) != hipSuccess ||
        hipMemcpyAsync(rs->d_alpha, p->alphabet, 256, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        mg_reads_free(rs);
        return fail(ctx, MG_ERR_NOMEM, "mg_reads_begin: device allocation failed");
    }
    *out = rs;
    return MG_OK;
}

namespace {

struct Record { uint64_t b, e; };

// Records of a batch (kseq drops nothing inside a record, so separators are record ends) of at least k bases -- shorter
// ones are skipped (Sketch.cpp:1222-1226): their number, and with `out` their [b, e).
static uint64_t scan_records(const uint8_t *bases, uint64_t nbases, uint64_t k, std::vector<Record> *out)
{
    uint64_t n = 0;
    for (uint64_t b = 0; b < nbases;) {
        const void *q = memchr(bases + b, MG_RECORD_SEP, nbases - b);
        const uint64_t e = q ? (uint64_t)((const uint8_t *)q - bases) : nbases;
        if (e - b >= k) { n++; if (out) out->push_back({b, e}); }
        b = e + 1;
    }
    return n;
}

// The unit of a launch is a PIECE: a range of k-mer start positions inside one record.  A record of any length (a
// chromosome under -r, Sketch.cpp:1196-1270 has no limit) is cut into pieces of at most kPiece positions -- every
// position yields at most one event, so a piece always fits the event buffer -- and the stop test of -c still
// follows whole records only (Sketch.cpp:1258).
struct Piece { uint64_t pb, pe; uint32_t rec; bool last; };

static std::vector<Piece> cut_pieces(const std::vector<Record> &rec, uint64_t k)
{
    constexpr uint64_t kPiece = kReadsEventCap / 4;
    std::vector<Piece> pieces;
    for (size_t r = 0; r < rec.size(); r++) {
        const uint64_t p0 = rec[r].b, p1 = rec[r].e - k + 1;             // k-mer starts [p0, p1)
        for (uint64_t o = p0; o < p1; o += kPiece) pieces.push_back({o, std::min(p1, o + kPiece), (uint32_t)r, o + kPiece >= p1});
    }
    return pieces;
}

// pieces [r0, r1) of one pass: as many as are expected to stay within the event capacity
static size_t size_pass(const mg_reads_session *rs, const std::vector<Piece> &pieces, size_t r0)
{
    const ReadsHeap &heap = rs->heap;
    const double hash_space = rs->p.use64 ? 18446744073709551616.0 : 4294967296.0;
    const uint64_t want_bytes = 2ull << 20;                  // while the heap is not full everything is an event
    const double pass = heap.full() ? std::min(1.0, ((double)heap.top() + 1.0) / hash_space) : 1.0;
    uint64_t budget = (uint64_t)std::min<double>((double)(1ull << 40), (double)(kReadsEventCap / 2) / std::max(pass, 1e-12));
    if (budget < want_bytes || !heap.full()) budget = want_bytes;
    budget = (uint64_t)std::max(1.0, (double)budget * rs->shrink);
    size_t r1 = r0;
    uint64_t bytes = 0;
    while (r1 < pieces.size() && (r1 == r0 || bytes + (pieces[r1].pe - pieces[r1].pb) <= budget)) {
        bytes += pieces[r1].pe - pieces[r1].pb;
        r1++;
    }
    return r1;
}

// One pass of the event kernel over k-mer starts [b0, b0 + npos), none reading past `limit`: the events that can enter the
// heap, in reading order, in rs->ev -- or *overflow: more of them than the buffer holds, nothing read back.
static int run_pass(mg_reads_session *rs, uint64_t b0, uint64_t npos, uint64_t limit, bool *overflow)
{
    mg_ctx *ctx = rs->ctx;
    const mg_params *p = &rs->p;
    const uint64_t tile = mg::sketch_tile(256);
    std::vector<mg::SketchWork> work;
    append_chunk_work(work, b0, npos, sketch_chunk_size(npos, 4096, 2 * tile, tile), limit, 0, nullptr);
    DevBuf<mg::SketchWork> d_work(ctx);
    if (d_work.alloc(work.size()) != hipSuccess) return fail(ctx, MG_ERR_NOMEM, "mg_reads_add_host: device allocation failed");
    mg::EventArgs ea;
    ea.bases = rs->d_bases; ea.work = d_work; ea.alphabet = rs->d_alpha; ea.out = rs->d_ev; ea.count = rs->d_cnt;
    ea.capacity = kReadsEventCap; ea.bound = rs->heap.full() ? rs->heap.top() : 0xFFFFFFFFFFFFFFFFull; ea.seed = p->seed; ea.use64 = p->use64;
    ea.fold_case = p->preserve_case ? 0 : 1;
    unsigned long long n_ev = 0;
    HIP_TRY(ctx, hipMemcpyAsync(d_work, work.data(), work.size() * sizeof(mg::SketchWork), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(rs->d_cnt, 0, 8, ctx->stream));
    HIP_TRY(ctx, mg::launch_hash_events(p->kmer_size, rs->mode, ea, (uint32_t)work.size(), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&n_ev, rs->d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *overflow = n_ev > kReadsEventCap;
    if (*overflow) return MG_OK;
    rs->ev.resize(n_ev);
    if (n_ev) HIP_TRY(ctx, hipMemcpy(rs->ev.data(), rs->d_ev, n_ev * sizeof(mg::HashEvent), hipMemcpyDeviceToHost));
    std::sort(rs->ev.begin(), rs->ev.end(), [](const mg::HashEvent &x, const mg::HashEvent &y) { return x.pos < y.pos; });
    return MG_OK;
}

// Replay of a chunk's events into the heap, record by record; the stop test follows every record that changed the heap.
struct Replay {
    mg_reads_session *rs;
    const std::vector<Record> &rec;
    size_t at = 0;                                           // record the replay is in
    bool touched = false;                                    // ... and whether it changed the heap
    void close(size_t upto)                                  // records [at, upto) are complete
    {
        if (at >= upto) return;
        // (without -c, a -b session, nothing stops the reading)
        if (rs->p.target_cov > 0 && touched && rs->heap.multiplicity() >= rs->p.target_cov) { rs->stopped = true; rs->used = rs->records + at + 1; }
        touched = false;
        at = upto;
    }
    void pass(const Piece &last)                             // the events of a pass that ended with piece `last`
    {
        for (size_t i = 0; i < rs->ev.size(); i++) {
            size_t r = at;
            while (rs->ev[i].pos >= rec[r].e) r++;           // the event's record
            close(r);
            if (rs->stopped) return;
            rs->heap.try_insert(rs->ev[i].hash);
            touched = true;
        }
        close(last.last ? (size_t)last.rec + 1 : (size_t)last.rec);
    }
};

}  // namespace

int mg_reads_add_host(mg_reads_session *rs, const uint8_t *bases, uint64_t nbases, int *stopped_out)
{
    if (!rs) return MG_ERR_INVALID;
    mg_ctx *ctx = rs->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (stopped_out) *stopped_out = rs->stopped ? 1 : 0;
    if (!bases && nbases) return fail(ctx, MG_ERR_INVALID, "mg_reads_add_host: NULL bases");
    if (rs->stopped || nbases == 0) return MG_OK;
    const uint64_t k = (uint64_t)rs->p.kmer_size;
    std::vector<Record> rec;
    if (scan_records(bases, nbases, k, &rec) == 0) return MG_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (nbases + 64 > rs->d_cap) {                           // the session's block grows to the largest chunk seen
        if (rs->d_bases) hipStreamSynchronize(ctx->stream);
        rs->d_cap = 0;
        const uint64_t cap = std::max<uint64_t>(nbases + 64, 1ull << 20);
        if (rs->d_bases.alloc(cap) != hipSuccess) return fail(ctx, MG_ERR_NOMEM, "mg_reads_add_host: device allocation failed");
        rs->d_cap = cap;
    }
    HIP_TRY(ctx, hipMemcpyAsync(rs->d_bases, bases, nbases, hipMemcpyHostToDevice, ctx->stream));
    const std::vector<Piece> pieces = cut_pieces(rec, k);
    Replay replay{rs, rec};
    for (size_t r0 = 0; r0 < pieces.size() && !rs->stopped;) {
        const size_t r1 = size_pass(rs, pieces, r0);
        const Piece &last = pieces[r1 - 1];
        bool overflow = false;
        const int rc = run_pass(rs, pieces[r0].pb, last.pe - pieces[r0].pb, rec[last.rec].e, &overflow);
        if (rc != MG_OK) return rc;
        if (overflow) {                                      // denser than expected: take fewer pieces
            if (r1 - r0 == 1) return fail(ctx, MG_ERR_HIP, "mg_reads_add_host: more events than k-mer positions in a piece");
            rs->shrink /= 4;
            continue;
        }
        rs->shrink = 1.0;
        replay.pass(last);
        r0 = r1;
    }
    rs->records += rec.size();
    if (stopped_out) *stopped_out = rs->stopped ? 1 : 0;
    return MG_OK;
}

int mg_reads_finish(mg_reads_session *rs, uint64_t *hashes_out, uint32_t *nhash_out, uint32_t *counts_out, uint64_t *records_used_out)
{
    if (!rs) return MG_ERR_INVALID;
    if (!hashes_out || !nhash_out) return fail(rs->ctx, MG_ERR_INVALID, "mg_reads_finish: NULL argument");
    const uint64_t s = rs->p.sketch_size;
    for (uint64_t i = 0; i < s; i++) hashes_out[i] = MG_HASH_PAD;
    if (counts_out) memset(counts_out, 0, s * 4);
    uint32_t n = 0;
    for (const auto &kv : rs->heap.kept) {
        hashes_out[n] = kv.first;
        if (counts_out) counts_out[n] = kv.second;
        n++;
    }
    *nhash_out = n;
    if (records_used_out) *records_used_out = rs->stopped ? rs->used : rs->records;
    return MG_OK;
}

int mg_reads_reset(mg_reads_session *rs)
{
    if (!rs) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(rs->ctx->mu);
    ReadsBloom bloom;
    std::swap(bloom, rs->heap.bloom);                       // keep the filter's memory, clear its bits
    std::fill(bloom.bits.begin(), bloom.bits.end(), 0);
    rs->heap = ReadsHeap(rs->p.sketch_size, rs->p.min_copies);
    std::swap(bloom, rs->heap.bloom);
    rs->stopped = false;
    rs->used = rs->records = 0;
    rs->shrink = 1.0;
    return MG_OK;
}

void mg_reads_free(mg_reads_session *rs)
{
    if (!rs) return;
    hipSetDevice(rs->ctx->device);
    hipStreamSynchronize(rs->ctx->stream);
    delete rs;
}

int mg_sketch_reads_host(mg_ctx *ctx, const mg_params *p, const uint8_t *bases, uint64_t nbases, uint64_t *hashes_out,
                         uint32_t *nhash_out, uint32_t *counts_out, uint64_t *records_used_out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!p || !hashes_out || !nhash_out || (!bases && nbases)) return fail(ctx, MG_ERR_INVALID, "mg_sketch_reads_host: NULL argument");
    if (!(p->target_cov > 0) && p->bloom_bytes == 0) {
        // the records of the batch: the "reads used" of a run without -c (a k out of range is refused by the sketching call)
        if (records_used_out) *records_used_out = scan_records(bases, nbases, (uint64_t)p->kmer_size, nullptr);
        mg_params q = *p;
        q.target_cov = 0;
        const uint64_t off[2] = {0, nbases};
        return mg_sketch_host(ctx, &q, bases, nbases, off, 1, hashes_out, nhash_out, counts_out);
    }
    // one chunk through the session
    mg_reads_session *rs = nullptr;
    int rc = mg_reads_begin(ctx, p, &rs);
    if (rc != MG_OK) return rc;
    rc = mg_reads_add_host(rs, bases, nbases, nullptr);
    if (rc == MG_OK) rc = mg_reads_finish(rs, hashes_out, nhash_out, counts_out, records_used_out);
    mg_reads_free(rs);
    return rc;
}

