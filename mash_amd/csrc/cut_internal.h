// cut_internal.h -- what a consumer of thresholded counts needs from host_compare.cpp: the range of a host-output call, the
// thresholds, the device buffers of pass A and of the two routes to the counts, and cut_counts, which walks one of the routes and
// hands every piece of it to the consumer.  Host only: for host_compare.cpp (survivors, the nearest k) and host_cluster.cpp (unions,
// edge lists).  The engines behind the routes stay inside host_compare.cpp.
#pragma once
#include "host_internal.h"

// What every host-output call starts from: [rb, re) clamped to the rows, the view a triangle of one table is served from
// (tri_view: the first re rows are all such a call looks at), s, and the pairs of the range.
struct OutRange {
    const mg_table *rows, *cols;
    uint64_t rb, re, pairs;
    uint32_t s;
    bool triangle;
    bool empty() const { return rb >= re; }
};

int out_range(mg_ctx *ctx, const mg_table *rows, const mg_table *cols, uint64_t rb, uint64_t re, bool triangle, OutRange *o,
              uint64_t max_s = 0xFFFFFFFEull);

// rows [r, r2): `pairs` pairs, `before` pairs of the range ahead of them
struct RowBlock { uint64_t r, r2, pairs, before; };

// The range in blocks of whole rows of at most max_pairs pairs (a block always takes its first row); *largest: the pairs of the
// largest block, which the caller's device buffers hold
std::vector<RowBlock> row_blocks(const OutRange &R, uint64_t max_pairs, uint64_t *largest);

// A caller's buffer of `capacity` records while blocks fill it: `total` counts on past the capacity (the caller is told the true
// count), nothing is written past it
struct Room {
    uint64_t capacity, total = 0;
    uint64_t left() const { return total <= capacity ? capacity - total : 0; }
    template <class T> T *at(T *out) const { return out + std::min(total, capacity); }
};

// How a caller has its matrix cut: row blocks of at most `pairs` pairs -- or of what the option `knob` says (the tests' way to many
// blocks): below `pairs`, or up to `ceiling` where a caller sets one -- and the caller's name in the allocation error
struct Blocks { uint64_t pairs; const char *knob, *who; uint64_t ceiling = 0; };

// what a caller's allocation callback answers when the device has no room: its driver words the error
static const int kAllocFailed = -1001;

// What a finish is given: k and the k-mer space of the distance and p-value formulas, and the two thresholds.  A threshold
// is on when it lies in [0, 1): one of 1 or more lets every pair through, a negative one means none was asked for.
struct Cut {
    int k;
    double kspace, max_d, max_p;
    bool d_on() const { return max_d >= 0.0 && max_d < 1.0; }
    bool filtered() const { return d_on() || (max_p >= 0.0 && max_p < 1.0); }
};

// What the device finish needs besides the counts: the distance table (host libm, one row per
// denominator flagged in `seen`, row s always) and the integer form of the distance filter.
struct FinishTables {
    DevBuf<uint32_t> d_start, d_min;
    DevBuf<double> d_lut;
    bool complete = true;                   // false: some flagged denominator did not fit the budget (device yields NaN)
    explicit FinishTables(mg_ctx *c) : d_start(c), d_min(c), d_lut(c) {}
};

int build_finish_tables(mg_ctx *ctx, uint32_t s, const Cut &cut, const std::vector<uint32_t> &seen, FinishTables &ft);

// The FinishArgs fields every device finish fills: `pairs` counts from row first_row on, the tables' lengths, the distance
// table and filters of `ft`
mg::FinishArgs finish_args(const mg_table *rows, const mg_table *cols, uint32_t s, bool triangle, const void *counts, uint64_t pairs,
                           uint64_t first_row, const FinishTables &ft, const Cut &cut);

// a denominator beyond the distance table's budget left NaN distances (FinishTables::complete): those are computed here
void patch_nan_distances(mg_result *r, uint64_t n, int k);

// The lists of a finished list job in REFERENCE order (host_compare.cpp: job_lists): K entries, {row, col} and {common, denom}
struct CandLists {
    uint64_t K = 0;
    DevBuf<uint2> rc, cnt;
    DevBuf<uint32_t> byrow, base;
    DevBuf<unsigned char> temp;
    size_t tb = 0;
    explicit CandLists(mg_ctx *c) : rc(c), cnt(c), byrow(c), base(c), temp(c) {}
    void release() { rc.free(); cnt.free(); byrow.free(); base.free(); temp.free(); }
};

// The inverted-index engine's job over R as lists, for a consumer that takes them whole (host_spectrum.cpp: with the filters off the
// lists are every pair that is not {0, rule denominator}).  *ok false: no lists -- the engine is forced off or leaves the job to the
// matrix (copies of rows, empty rows, nearly every pair related), or they do not fit; that is no error, and L is released then.
// *ok with L.K == 0: no pair of R shares a hash.  extra(K) allocates the consumer's buffers for K entries (false: they do not fit).
int job_cand_lists(mg_ctx *ctx, const OutRange &R, CandLists &L, bool *ok, const std::function<bool(uint64_t K)> &extra);

// Pass A of a finish (finish_mark_kernel) over up to `pairs` entries: its ballots and segments, the denominators it flags
struct PassABufs {
    DevBuf<unsigned long long> masks, seg_off;
    DevBuf<uint32_t> seg_count, seen;
    explicit PassABufs(mg_ctx *owner) : masks(owner), seg_off(owner), seg_count(owner), seen(owner) {}
    bool alloc(uint64_t pairs, uint32_t s)
    {
        return masks.alloc(mg::finish_mask_words(pairs)) == hipSuccess && seg_count.alloc(mg::finish_segments(pairs)) == hipSuccess &&
               seg_off.alloc(mg::finish_segments(pairs)) == hipSuccess && seen.alloc((uint64_t)s + 1) == hipSuccess;
    }
    void release() { masks.free(); seg_off.free(); seg_count.free(); seen.free(); }
    void bind(mg::FinishArgs &f) const
    {
        f.masks = masks;
        f.seg_count = seg_count;
        f.seg_off = seg_off;
        f.denom_seen = seen;
    }
};

// What a thresholded call keeps on the device for as long as it runs, whichever route serves it: the candidate lists, the finish
// tables of pass A, the counts of a matrix block (their owner is the caller's choice)
struct CutBufs {
    CandLists L;
    FinishTables fa;
    DevBuf<mg_counts> counts;
    CutBufs(mg_ctx *ctx, mg_ctx *counts_owner) : L(ctx), fa(ctx), counts(counts_owner) {}
};

// The counts of R for a consumer that thresholds them (survivors, unions, edges, the nearest k), by one of two routes:
//  * lists, if asked for and the index engine gives them: a filter is on, so only pairs that share a hash can pass (numer = 0 means
//    distance 1 and p-value 1), and those are the engine's candidates -- no matrix is filled, no 8 B per pair read back.  use() is
//    called once, f over the list (f.list_rc) and L the lists, b the whole range -- or not at all: no candidates.
//  * the matrix in row blocks otherwise: use() is called per block, L == nullptr.  Every block has pairs.
// f carries pass A's tables (no extra denominator row), built once: behind the first compare, for building waits.
// alloc(pairs, rows, blocks, lists) allocates the consumer's buffers for the list or the largest block and answers MG_OK,
// kAllocFailed, or an error it has worded itself; on the matrix route it may also queue what has to precede the first compare, on the
// lists route anything but MG_OK only means no lists.  Lists that fall through leave nothing behind on the device -- the fallback is
// there for the device that is short of memory --: give_back() frees what alloc(.., true) took.
// The callbacks run once per call or row block, beside a compare and several launches.
using CutAlloc = std::function<int(uint64_t pairs, uint64_t rows, uint64_t blocks, bool lists)>;
using CutUse = std::function<int(const mg::FinishArgs &f, const RowBlock &b, const CandLists *L)>;
int cut_counts(mg_ctx *ctx, const OutRange &R, const Cut &cut, bool try_lists, const Blocks &how, CutBufs &B, const CutAlloc &alloc,
               const std::function<void()> &give_back, const CutUse &use);
