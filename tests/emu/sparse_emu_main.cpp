// sparse_emu_main.cpp -- runs the inverted-index engine of mash_amd/csrc/compare_sparse.hip on host fibers (tools/hipemu):
// sp_locate, sp_discover (count-only and listing, with and without classes of copies), the SIX merge forms -- one lane per
// candidate (sp_merge_kernel), the whole row in LDS (sp_merge_rows_kernel), the row a window at a time
// (sp_merge_rows_win_kernel), several rows per item (sp_merge_pack_kernel<32 | 43 | 64>) --, sp_scatter, sp_class_pairs and
// sp_fill_short, all through the library's own launchers, on index arrays made here by a std::stable_sort, and compares EVERY
// pair of the output with the loop of compareSketches (CommandDistance.cpp:347-385, restated below on the rows' 64-bit
// values).  The six forms' `res` arrays must also be byte-equal to each other; a form its launcher declines is reported.
// The discover stage is checked on its own: counters[0] = the candidates listed, counters[1] = the shared hashes the table
// gives, the candidate set = the pairs that share a value among their first s (pairs of one class left out), every row's
// segment in column order, count-only = listing, and a list too small raises counters[2] without a write behind cand_cap.
// TEST INFRASTRUCTURE (tests/test_sparse_emu.py); built with g++.
//
//   sparse_emu <case> [seed [cases]]      cases: see main(); exit status 0 = every pair agrees
//
// Arrays the kernels only read stand in front of a page without access (Fenced): a read past an image is a fault here, not
// a guess.  The table's code image has the library's slack (n * rs + 64 words: every lane loads 24 column codes before it
// looks at anything, and the refill reads up to code ib + 32 of its column); the query images of a rect job have none, as
// in host_compare.cpp -- the row side is never read beyond (nA >> 2) * 4 + 3 < rs.
//
// Edges, where the code gives another one than the issue named:
//   * with s = 200 and rounds of 8 steps the union reaches s on step 8 of round 25, whatever the rows hold; the steps 1, 7, 8
//     and 9 of a round are met by the OTHER two bounds (a side exhausted at union size 17, 23, 24, 25; both roles) in `ring`,
//     and by s = 1, 7, 8, 9, 15, 16, 17 in `sizes`;
//   * a segment with classes is in the order of the classes' representatives, a class's rows ascending behind each other --
//     in column order only where the table holds no copies;
//   * the bitmap's words per thread go from 1 to 2 between a row of 8192 columns and one of 8193, so the table has 8194 rows;
//   * the library gives a rect job's query images the TABLE's stride; the kernels take any, so `rect` also runs a query
//     sketch size of 20 at stride 24 against the table's 36.
//
// Mutations of compare_sparse.hip (each alone, on a scratch copy of the file; the harness rebuilt and every case run) and the
// cases that fail under it -- the case named first is the one the mutation was aimed at:
//   refill test `loaded + 8u - ib <= SPM_RING` -> `< SPM_RING + 8u`, in each of the three ring kernels in turn:
//       ring (a chunk lands on codes not yet consumed: 27 common instead of 65), sizes from s = 31, windows, copies, rect
//   staging `nvec = (nA >> 2) + 1u` without the `+ 1u` (whole-row kernel; `(n >> 2) + 1u` of the pack kernel):
//       sizes from s = 3 (the row's last chunk is never staged) and every other case
//   `room < 8u` -> `room < 7u`, in each of the three kernels in turn:
//       sizes at s = 15 ({9, 16} for {9, 15}: the unchecked round steps past a bound), copies; the windowed form also in
//       `windows` (on the sizes tables)
//   the window's `aend` from `a0 + SPM_AWIN - 1`:
//       windows at s = 2048 (a lane waits at code 2047, the next window starts at 2048: A[ia - a0] leaves the LDS -- here a
//       fault at a fence); no other case has a row of more than one window
//   `SHORT = 7` without the matching change in the long-run ballot, i.e. `__ballot(len > SHORT + 1)`: runs of 7 are marked by
//   neither path:
//       discover (20139 of 20146 candidates), sizes, ring, chunks, windows, copies
//     (the other half -- `len <= SHORT + 1` in the short loop with the ballot unchanged -- marks runs of 7 twice, which is the
//      same program: no case can fail, none does)
//   pack: `u >= a.chunk_inc[sB - 1u]` -> `>`:
//       pack (the first candidate of a row that starts inside an item is nobody's: its result slot keeps the harness's
//       poison) and every other case
//   rect: the `| 1u` of the column codes dropped -- lanes (both places, and the one in the loop alone), whole rows (both rounds,
//   and the checked round alone), windowed, pack:
//       rect, and only rect.  The lane kernel's `| 1u` in the loop alone survived the first version of the table, whose
//       values of a single row all stood first in their rows: ref row r now holds V(1001 + 2 r) in its middle.
#include "../../tools/hipemu/hipemu.h"

#include <signal.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../mash_amd/csrc/compare_sparse.hip"

using namespace mg;

typedef std::vector<uint64_t> Row;
typedef std::vector<Row> Rows;

// ------------------------------------------------------------------------------------------------ fenced arrays
template <class T> struct Fenced {
    T *p = nullptr;
    size_t n = 0;
    void *map = nullptr;
    size_t map_bytes = 0;
    Fenced() {}
    Fenced(const Fenced &) = delete;
    Fenced &operator=(const Fenced &) = delete;
    ~Fenced() { if (map) munmap(map, map_bytes); }
    void make(size_t count, T fill)
    {
        if (map) munmap(map, map_bytes);
        const size_t page = 4096, bytes = count * sizeof(T);
        map_bytes = ((bytes + page - 1) / page + 1) * page;
        map = mmap(nullptr, map_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (map == MAP_FAILED) { fprintf(stderr, "mmap failed\n"); exit(2); }
        mprotect((char *)map + map_bytes - page, page, PROT_NONE);
        p = reinterpret_cast<T *>((char *)map + map_bytes - page - bytes);      // the array ends where the fence starts
        n = count;
        for (size_t i = 0; i < count; i++) p[i] = fill;
    }
    void from(const std::vector<T> &v) { make(v.size(), T()); for (size_t i = 0; i < v.size(); i++) p[i] = v[i]; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
};

static const char *g_what = "";
static void on_fault(int)
{
    static const char msg[] = "sparse_emu: access past the end of a fenced array in: ";
    (void)!write(2, msg, sizeof msg - 1);
    (void)!write(2, g_what, strlen(g_what));
    (void)!write(2, "\n", 1);
    _exit(3);
}

// ------------------------------------------------------------------------------------------------ the reference
// the loop of compareSketches on two rows (CommandDistance.cpp:347-385)
static uint2 reference_pair(const Row &A, const Row &B, uint32_t s)
{
    size_t i = 0, j = 0;
    uint64_t c = 0, d = 0;
    while (d < s && i < A.size() && j < B.size()) {
        if (A[i] < B[j]) i++;
        else if (B[j] < A[i]) j++;
        else { i++; j++; c++; }
        d++;
    }
    if (d < s) {
        d += (A.size() - i) + (B.size() - j);
        if (d > s) d = s;
    }
    return make_uint2((uint32_t)c, (uint32_t)d);
}

static bool share_a_value(const Row &A, const Row &B)
{
    size_t i = 0, j = 0;
    while (i < A.size() && j < B.size()) {
        if (A[i] < B[j]) i++;
        else if (B[j] < A[i]) j++;
        else return true;
    }
    return false;
}

static Row finish_row(Row v, uint32_t keep)
{
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    if (v.size() > keep) v.resize(keep);
    return v;
}

static Rows clipped(const Rows &t, uint32_t s)
{
    Rows r;
    for (const Row &x : t) r.push_back(finish_row(x, s));
    return r;
}

// value number k of the tables below: ascending in k, above 2^32, low bits that do not follow k
static uint64_t V(uint64_t k) { return ((k + 1) << 34) + ((k * 2654435761ull) & 0xFFFFFFFFull); }

// ------------------------------------------------------------------------------------------------ the index
// every array of the column side as host_index.cpp lays it out: entries (value, row) in value order, rows ascending inside
// a value (std::stable_sort); code = 2 x first sorted position of the value's group + (another row holds it too); copies of
// an earlier row stay out and form classes
struct Index {
    uint32_t n = 0, rs = 0, E = 0, nshort = 0, cls_members = 0;
    bool copies = false;
    std::vector<uint32_t> rep_h, short_h;
    Fenced<uint32_t> off, code, pos, sorted_rows, gend, rep, cls_of, cls_off, cls_rows, cls_first, short_rows, short_cnt;
    Fenced<uint64_t> keys_sorted;
};

static void build_index(Index &ix, const Rows &rows, uint32_t s, bool dedup)
{
    const uint32_t n = ix.n = (uint32_t)rows.size();
    ix.rs = sparse_img_stride(s);
    ix.rep_h.resize(n);
    ix.copies = false;
    std::map<Row, uint32_t> firsts;
    for (uint32_t i = 0; i < n; i++) {
        ix.rep_h[i] = i;
        if (!dedup || rows[i].empty()) continue;
        auto it = firsts.find(rows[i]);
        if (it == firsts.end()) firsts[rows[i]] = i;
        else { ix.rep_h[i] = it->second; ix.copies = true; }
    }
    std::vector<uint32_t> off(n + 1, 0), short_cnt;
    std::vector<std::pair<uint64_t, uint32_t>> ent;         // (value, image index)
    ix.short_h.clear();
    for (uint32_t i = 0; i < n; i++) {
        off[i] = (uint32_t)ent.size();
        if (ix.rep_h[i] == i)
            for (uint32_t p = 0; p < rows[i].size(); p++) ent.push_back({rows[i][p], i * ix.rs + p});
        if (rows[i].size() < s) { ix.short_h.push_back(i); short_cnt.push_back((uint32_t)rows[i].size()); }
    }
    off[n] = ix.E = (uint32_t)ent.size();
    std::stable_sort(ent.begin(), ent.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    ix.off.from(off);
    ix.code.make((size_t)n * ix.rs + 64, 0xFFFFFFFFu);       // (the library's slack)
    ix.pos.make((size_t)n * ix.rs, 0u);
    ix.sorted_rows.make(ix.E, 0u);
    ix.gend.make(ix.E, 0xFFFFFFFFu);                        // (defined at the first position of a value's group only)
    ix.keys_sorted.make(ix.E, 0ull);
    for (uint32_t e = 0; e < ix.E;) {
        uint32_t f = e;
        while (f < ix.E && ent[f].first == ent[e].first) f++;
        ix.gend[e] = f;
        for (uint32_t g = e; g < f; g++) {
            ix.code[ent[g].second] = 2u * e + (f - e >= 2 ? 1u : 0u);
            ix.pos[ent[g].second] = g;
            ix.keys_sorted[g] = ent[g].first;
            ix.sorted_rows[g] = ent[g].second / ix.rs;
        }
        e = f;
    }
    ix.nshort = (uint32_t)ix.short_h.size();
    ix.short_rows.from(ix.short_h);
    ix.short_cnt.from(short_cnt);
    ix.cls_members = 0;
    if (ix.copies) {
        std::vector<uint32_t> cls_of(n, 0xFFFFFFFFu), size(n, 0), cls_off, cls_rows, cls_first;
        for (uint32_t i = 0; i < n; i++) size[ix.rep_h[i]]++;
        uint32_t ncls = 0, tot = 0;
        for (uint32_t i = 0; i < n; i++)
            if (size[i] >= 2) { cls_of[i] = ncls++; cls_off.push_back(tot); tot += size[i]; }
        cls_off.push_back(tot);
        cls_rows.resize(tot);
        cls_first.resize(tot);
        std::vector<uint32_t> at(cls_off.begin(), cls_off.end() - 1);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t k = cls_of[ix.rep_h[i]];
            if (k != 0xFFFFFFFFu) { cls_first[at[k]] = cls_off[k]; cls_rows[at[k]++] = i; }
        }
        ix.rep.from(ix.rep_h); ix.cls_of.from(cls_of); ix.cls_off.from(cls_off); ix.cls_rows.from(cls_rows); ix.cls_first.from(cls_first);
        ix.cls_members = tot;
    }
}

static void column_side(SparseArgs &a, const Index &ix, uint32_t s)
{
    memset(&a, 0, sizeof a);
    a.sorted_rows = ix.sorted_rows.p;
    a.col_img = ix.code.p;
    a.col_cnt_off = ix.off.p;
    a.rs_col = ix.rs;
    a.ncols = ix.n;
    a.s = s;
    a.gend = ix.gend.p;
    if (ix.copies) { a.rep = ix.rep.p; a.cls_of = ix.cls_of.p; a.cls_off = ix.cls_off.p; a.cls_rows = ix.cls_rows.p; }
}

// ------------------------------------------------------------------------------------------------ a job
enum { F_LANES = 1, F_ROWS = 2, F_WIN = 4, F_P32 = 8, F_P43 = 16, F_P64 = 32, F_ALL = 63 };
static const char *form_name[6] = {"lanes", "rows", "rows windowed", "pack 32", "pack 43", "pack 64"};

struct Want {                                               // what the table says the job must give
    std::set<std::pair<uint32_t, uint32_t>> cand;           // {row, col} in the index's rows
    unsigned long long shared = 0;
    std::vector<uint2> out;                                 // every pair of the output
};

struct Tally { uint64_t pairs = 0, cands = 0, forms_run = 0, declined = 0; uint32_t max_pack_rows[3] = {0, 0, 0}; };
static Tally g_t;

static const uint2 POISON = {0xDEADBEEFu, 0xDEADBEEFu};
static bool is_poison(const uint2 &v) { return v.x == POISON.x && v.y == POISON.y; }

// rows of one item of the pack kernel, from the segments (a check of the TABLE: does it stage as many rows as the case wants)
static uint32_t most_rows_per_item(const uint32_t *seg_cnt, uint32_t nrows, uint32_t pack_min)
{
    uint64_t u = 0;
    std::vector<uint32_t> per_item;
    for (uint32_t r = 0; r < nrows; r++) {
        if (!seg_cnt[r]) continue;
        const uint64_t c = std::max(seg_cnt[r], pack_min);
        for (uint64_t it = u / 128; it <= (u + c - 1) / 128; it++) {
            if (per_item.size() <= it) per_item.resize(it + 1, 0);
            per_item[it]++;
        }
        u += c;
    }
    uint32_t m = 0;
    for (uint32_t x : per_item) m = std::max(m, x);
    return m;
}

// discover (both forms), every merge form of `forms`, scatter over `prefill`; ref(row, col): the reference of a candidate.
// col_key(c): what a segment ascends in.  small_list: also a listing launch with half the room it needs.
template <class Prefill, class Ref>
static int run_stages(const char *what, SparseArgs a, const Want &w, unsigned forms, bool small_list, const std::vector<uint32_t> *rep_h, Prefill prefill, Ref ref)
{
    g_what = what;
    int bad = 0;
    const uint32_t nrows = a.row_end - a.row_begin;
    auto fail = [&](const char *fmt, auto... x) {
        if (bad++ >= 12) return;
        fprintf(stderr, "%s: ", what);
        if constexpr (sizeof...(x) == 0) fputs(fmt, stderr); else fprintf(stderr, fmt, x...);
        fprintf(stderr, "\n");
    };
    if (!sparse_discover_supported(a.triangle ? a.row_end : a.ncols)) { fail("discover does not take %u columns", a.ncols); return bad; }
    unsigned long long counters[4] = {0, 0, 0, 0};
    a.counters = counters;
    Fenced<unsigned long long> seg_base;
    Fenced<uint32_t> seg_cnt, chunks, chunk_inc;
    seg_base.make(nrows, 0); seg_cnt.make(nrows, 0); chunks.make(nrows, 0); chunk_inc.make(nrows, 0);
    a.seg_base = seg_base.p; a.seg_cnt = seg_cnt.p; a.chunk_inc = chunk_inc.p;
    // ---- count only
    a.cand = nullptr; a.cand_cap = 0;
    if (launch_sparse_discover(a, true, nullptr) != hipSuccess) { fail("discover (count) failed"); return bad; }
    const unsigned long long K = counters[0];
    if (K != w.cand.size()) fail("count-only discover: %llu candidates, the table has %llu", K, (unsigned long long)w.cand.size());
    if (counters[1] != w.shared) fail("count-only discover: %llu shared hashes, the table has %llu", counters[1], w.shared);
    if (counters[2] != 0) fail("count-only discover raised the overflow flag");
    // ---- listing, into a list with exactly the room it needs and guard words behind
    const uint64_t cap = std::max<unsigned long long>(K, w.cand.size());
    std::vector<uint2> cand(cap + 16, POISON);
    a.cand = cand.data(); a.cand_cap = cap;
    memset(counters, 0, sizeof counters);
    if (launch_sparse_discover(a, false, nullptr) != hipSuccess) { fail("discover (list) failed"); return bad; }
    if (counters[0] != K || counters[1] != w.shared || counters[2] != 0)
        fail("listing discover: counters {%llu, %llu, %llu}, count-only {%llu, %llu, 0}", counters[0], counters[1], counters[2], K, w.shared);
    for (uint64_t k = cap; k < cap + 16; k++) if (!is_poison(cand[k])) fail("discover wrote behind cand_cap (slot %llu)", (unsigned long long)k);
    {
        std::vector<std::pair<unsigned long long, uint32_t>> segs;
        unsigned long long listed = 0;
        for (uint32_t sl = 0; sl < nrows; sl++) if (seg_cnt[sl]) { segs.push_back({seg_base[sl], sl}); listed += seg_cnt[sl]; }
        if (listed != K) fail("the segments hold %llu candidates, counters[0] is %llu", listed, K);
        std::sort(segs.begin(), segs.end());
        unsigned long long at = 0;
        std::set<std::pair<uint32_t, uint32_t>> got;
        for (auto &sg : segs) {
            if (sg.first != at) { fail("segment of slot %u starts at %llu, the one before ends at %llu", sg.second, sg.first, at); break; }
            const uint32_t row = a.order ? a.order[sg.second] : a.row_end - 1u - sg.second;
            for (uint32_t t = 0; t < seg_cnt[sg.second] && at + t < cap; t++) {
                const uint2 c = cand[at + t];
                if (c.x != row) fail("slot %u (row %u) lists a pair of row %u", sg.second, row, c.x);
                if (t) {
                    const uint2 p = cand[at + t - 1];
                    const bool asc = rep_h ? std::make_pair((*rep_h)[p.y], p.y) < std::make_pair((*rep_h)[c.y], c.y) : p.y < c.y;
                    if (!asc) fail("row %u: column %u listed behind column %u", row, c.y, p.y);
                }
                if (!got.insert({c.x, c.y}).second) fail("pair (%u, %u) listed twice", c.x, c.y);
            }
            at += seg_cnt[sg.second];
        }
        if (got != w.cand) {
            for (auto &pr : w.cand) if (!got.count(pr)) { fail("pair (%u, %u) shares a value and is not listed", pr.first, pr.second); break; }
            for (auto &pr : got) if (!w.cand.count(pr)) { fail("pair (%u, %u) is listed and shares no value", pr.first, pr.second); break; }
        }
    }
    if (bad) return bad;
    g_t.cands += K;
    printf("%s: %llu candidates, %llu shared hashes\n", what, K, w.shared);
    // ---- a list too small: the flag, the full count, nothing behind the cap
    if (small_list && K >= 2) {
        const uint64_t cap2 = K / 2;
        std::vector<uint2> c2(cap2 + 16, POISON);
        Fenced<unsigned long long> sb2; Fenced<uint32_t> sc2;
        sb2.make(nrows, 0); sc2.make(nrows, 0);
        SparseArgs b = a;
        unsigned long long ctr2[4] = {0, 0, 0, 0};
        b.counters = ctr2; b.cand = c2.data(); b.cand_cap = cap2; b.seg_base = sb2.p; b.seg_cnt = sc2.p;
        if (launch_sparse_discover(b, false, nullptr) != hipSuccess) fail("discover (small list) failed");
        if (ctr2[2] != 1) fail("a list of %llu for %llu candidates: counters[2] = %llu", (unsigned long long)cap2, K, ctr2[2]);
        if (ctr2[0] != K) fail("a list too small: counters[0] = %llu, not the %llu the host grows the list to", ctr2[0], K);
        for (uint64_t k = cap2; k < cap2 + 16; k++) if (!is_poison(c2[k])) fail("discover wrote behind a cand_cap too small (slot %llu)", (unsigned long long)k);
    }
    // ---- the merge forms
    std::vector<uint2> want_res(K);
    for (uint64_t k = 0; k < K; k++) want_res[k] = ref(cand[k].x, cand[k].y);
    std::vector<uint2> first_res;
    const bool must_decline = a.rs_row > 2056u;             // (SPM_AWIN + 8: the largest row the whole-row and pack kernels stage)
    unsigned char temp[16];
    for (int f = 0; f < 6; f++) {
        if (!(forms & (1u << f))) continue;
        std::vector<uint2> res(cap + 16, POISON);
        a.res = res.data();
        unsetenv("MASHGPU_SPARSE_MERGE_WINDOWS");
        unsetenv("MASHGPU_SPARSE_PACK_MIN");
        hipError_t e = hipSuccess;
        bool declined = false;
        if (f == 0) {
            e = launch_sparse_merge(a, K, 0, nullptr);
        } else if (f == 1 || f == 2) {
            if (f == 2) setenv("MASHGPU_SPARSE_MERGE_WINDOWS", "1", 1);
            bool windowed = false;
            e = launch_sparse_merge_rows(a, K, chunks.p, temp, sizeof temp, nullptr, &windowed);
            if (K && f == 2 && !windowed) fail("the windowed form was asked for and the whole-row kernel ran");
            if (f == 1 && windowed) declined = true;        // (the launcher took the windowed kernel: checked as form 2)
        } else {
            const uint32_t pm = f == 3 ? 32u : f == 4 ? 43u : 64u;
            setenv("MASHGPU_SPARSE_PACK_MIN", f == 3 ? "32" : f == 4 ? "43" : "64", 1);
            bool used = false;
            uint32_t ran = 0;
            e = launch_sparse_merge_pack(a, K, chunks.p, temp, sizeof temp, &used, nullptr, &ran);
            declined = !used;
            if (used && ran != pm) fail("pack %u was asked for and pack %u ran", pm, ran);
            if (used) g_t.max_pack_rows[f - 3] = std::max(g_t.max_pack_rows[f - 3], most_rows_per_item(seg_cnt.p, nrows, pm));
        }
        unsetenv("MASHGPU_SPARSE_MERGE_WINDOWS");
        unsetenv("MASHGPU_SPARSE_PACK_MIN");
        if (e != hipSuccess) { fail("%s: the launcher failed", form_name[f]); continue; }
        if (K == 0) continue;                               // (nothing to merge: every launcher returns at once)
        if (declined) {
            g_t.declined++;
            printf("%s: %s declined (rs_row %u)\n", what, form_name[f], a.rs_row);
            if (!must_decline) fail("%s declined a row stride of %u", form_name[f], a.rs_row);
            continue;
        }
        if (must_decline && f != 0 && f != 2) fail("%s took a row stride of %u", form_name[f], a.rs_row);
        g_t.forms_run++;
        int shown = 0;
        for (uint64_t k = 0; k < K; k++)
            if (res[k].x != want_res[k].x || res[k].y != want_res[k].y) {
                if (shown++ < 4) fail("%s: candidate %llu (%u, %u): got {%u, %u}, reference {%u, %u}", form_name[f], (unsigned long long)k, cand[k].x, cand[k].y, res[k].x, res[k].y, want_res[k].x, want_res[k].y);
                else bad++;
            }
        for (uint64_t k = K; k < cap + 16; k++) if (!is_poison(res[k])) fail("%s wrote res[%llu] behind the %llu candidates", form_name[f], (unsigned long long)k, K);
        if (first_res.empty()) first_res.assign(res.begin(), res.begin() + K);
        else if (memcmp(first_res.data(), res.data(), K * sizeof(uint2)) != 0) fail("%s: res differs from the first form's", form_name[f]);
        // ---- the output: the constant, the short pairs and the class pairs, then this form's results scattered over them
        if (!w.out.empty()) {
            std::vector<uint2> out(w.out.size() + 1, POISON);
            a.out = out.data();
            prefill(out.data(), w.out.size());
            if (launch_sparse_scatter(a, K, 0, nullptr) != hipSuccess) fail("scatter failed");
            shown = 0;
            for (size_t o = 0; o < w.out.size(); o++)
                if (out[o].x != w.out[o].x || out[o].y != w.out[o].y) {
                    if (shown++ < 4) fail("%s: output slot %llu: got {%u, %u}, reference {%u, %u}", form_name[f], (unsigned long long)o, out[o].x, out[o].y, w.out[o].x, w.out[o].y);
                    else bad++;
                }
            if (!is_poison(out[w.out.size()])) fail("%s: wrote past the end of the output", form_name[f]);
            g_t.pairs += w.out.size();
        }
    }
    if (K == 0 && !w.out.empty()) {                         // no candidate at all: the fills are the whole answer
        std::vector<uint2> out(w.out.size() + 1, POISON);
        prefill(out.data(), w.out.size());
        for (size_t o = 0; o < w.out.size(); o++)
            if (out[o].x != w.out[o].x || out[o].y != w.out[o].y) fail("output slot %llu without candidates: got {%u, %u}, reference {%u, %u}", (unsigned long long)o, out[o].x, out[o].y, w.out[o].x, w.out[o].y);
        g_t.pairs += w.out.size();
    }
    return bad;
}

struct TriOpt {
    uint32_t rb = 0, re = 0;                                // re = 0: the whole table
    bool dedup = true, permute = false, order = false, small_list = false, no_out = false;
    unsigned forms = F_ALL;
};

// triangle over rows [rb, re) of the INDEX; permute: the index stands on the table in another order (index row a = table row inv[a])
static int run_triangle(const char *what, const Rows &table_in, uint32_t s, TriOpt o, std::mt19937_64 &rng)
{
    const Rows table = clipped(table_in, s);
    const uint32_t n = (uint32_t)table.size();
    if (o.re == 0) o.re = n;
    std::vector<uint32_t> inv(n);
    for (uint32_t i = 0; i < n; i++) inv[i] = i;
    if (o.permute) { std::shuffle(inv.begin(), inv.end(), rng); o.rb = 0; o.re = n; }
    Rows rows(n);
    for (uint32_t a2 = 0; a2 < n; a2++) rows[a2] = table[inv[a2]];
    Index ix;
    build_index(ix, rows, s, o.dedup);
    if (ix.E == 0) return 0;
    SparseArgs a;
    column_side(a, ix, s);
    a.triangle = 1;
    a.lo_img = ix.code.p; a.hi_img = ix.pos.p; a.lo_shift = 1;
    a.off = ix.off.p; a.row_img = ix.code.p; a.rs_row = ix.rs;
    a.row_begin = o.rb; a.row_end = o.re;
    a.out_base = o.rb ? (uint64_t)o.rb * (o.rb - 1) / 2 : 0;
    a.inv = o.permute ? inv.data() : nullptr;
    std::vector<uint32_t> order;
    if (o.order) {
        for (uint32_t r = o.rb; r < o.re; r++) order.push_back(r);
        std::shuffle(order.begin(), order.end(), rng);
        a.order = order.data();
    }
    const std::vector<uint32_t> &rep = ix.rep_h;
    // what the table says
    Want w;
    std::map<uint64_t, std::vector<uint32_t>> holders;      // per value: the representatives that hold it, ascending
    for (uint32_t j = 0; j < n; j++)
        if (rep[j] == j) for (uint64_t v : rows[j]) holders[v].push_back(j);
    for (uint32_t i = o.rb; i < o.re; i++) {
        const Row &A = rows[rep[i]];
        if (A.empty() || i == 0) continue;
        for (uint32_t j = 0; j < i; j++)
            if (rep[i] != rep[j] && share_a_value(A, rows[rep[j]])) w.cand.insert({i, j});
        // shared hashes as discovery counts them: per value of the row the representatives below it that hold it; a copy
        // walks the whole run of each of its representative's values
        for (uint64_t v : A) {
            const std::vector<uint32_t> &h = holders[v];
            w.shared += rep[i] != i ? h.size() : (size_t)(std::lower_bound(h.begin(), h.end(), i) - h.begin());
        }
    }
    const uint64_t npairs = (uint64_t)o.re * (o.re - 1) / 2 - a.out_base;
    if (!o.no_out) {
        w.out.assign(npairs, make_uint2(0, 0));
        for (uint32_t i = o.rb; i < o.re; i++)
            for (uint32_t j = 0; j < i; j++) {
                const uint32_t ti = inv[i], tj = inv[j], hi = std::max(ti, tj), lo = std::min(ti, tj);
                w.out[(uint64_t)hi * (hi - 1) / 2 + lo - a.out_base] = reference_pair(table[hi], table[lo], s);
            }
    }
    const uint32_t k0 = (uint32_t)(std::lower_bound(ix.short_h.begin(), ix.short_h.end(), o.rb) - ix.short_h.begin());
    const uint32_t k1 = (uint32_t)(std::lower_bound(ix.short_h.begin(), ix.short_h.end(), o.re) - ix.short_h.begin());
    auto prefill = [&](uint2 *out, size_t count) {
        for (size_t k = 0; k < count; k++) out[k] = make_uint2(0u, s);      // (the fill kernels' constant)
        launch_sparse_fill_short(out, ix.short_rows.p + k0, ix.short_cnt.p + k0, k1 - k0, ix.short_rows.p, ix.short_cnt.p, ix.nshort, a.row_begin, a.ncols, 1u,
                                 a.out_base, s, a.inv, nullptr);
        if (ix.cls_members) launch_sparse_class_pairs(out, ix.cls_rows.p, ix.cls_first.p, ix.off.p, ix.rep.p, ix.cls_members, a.row_begin, a.row_end, a.out_base, a.inv, nullptr);
    };
    auto ref = [&](uint32_t i, uint32_t j) { return reference_pair(rows[i], rows[j], s); };
    return run_stages(what, a, w, o.forms, o.small_list, ix.copies ? &ix.rep_h : nullptr, prefill, ref);
}

// rect: queries [q_begin, q_begin + nq) of a query table of sketch size sq, located in the reference table's index
static int run_rect(const char *what, const Rows &ref_in, const Rows &qry_in, uint32_t s, uint32_t sq, unsigned forms, bool small_list = false)
{
    const Rows ref = clipped(ref_in, s), qry = clipped(qry_in, std::min(s, sq));
    Index ix;
    build_index(ix, ref, s, true);
    if (ix.E == 0) return 0;
    const uint32_t nq = (uint32_t)qry.size(), nr = (uint32_t)ref.size(), q_begin = 2;
    // the query image takes the table's stride in the library; a smaller sketch size is given its own here (the kernels take any)
    const uint32_t rsq = sq < s ? sparse_img_stride(sq) : ix.rs;
    Fenced<uint64_t> qh;
    qh.make((size_t)(q_begin + nq) * sq, ~0ull);
    std::vector<uint32_t> qoff(nq + 1, 0), qshort, qshort_cnt;
    for (uint32_t q = 0; q < nq; q++) {
        for (uint32_t p = 0; p < qry[q].size(); p++) qh[(size_t)(q_begin + q) * sq + p] = qry[q][p];
        qoff[q + 1] = qoff[q] + (uint32_t)qry[q].size();
        if (qry[q].size() < s) { qshort.push_back(q); qshort_cnt.push_back((uint32_t)qry[q].size()); }
    }
    Fenced<uint32_t> q_off, q_lo, q_hi, q_img, q_short, q_short_cnt;
    q_off.from(qoff); q_short.from(qshort); q_short_cnt.from(qshort_cnt);
    q_lo.make((size_t)nq * rsq, 0u); q_hi.make((size_t)nq * rsq, 0u); q_img.make((size_t)nq * rsq, 0u);       // (no slack: as host_compare.cpp allocates them)
    g_what = what;
    if (launch_sparse_locate(qh.p, sq, q_off.p, q_begin, nq, ix.keys_sorted.p, ix.gend.p, ix.E, rsq, q_lo.p, q_hi.p, q_img.p, nullptr) != hipSuccess) return 1;
    SparseArgs a;
    column_side(a, ix, s);
    a.triangle = 0;
    a.lo_img = q_lo.p; a.hi_img = q_hi.p; a.lo_shift = 0;
    a.off = q_off.p; a.row_img = q_img.p; a.rs_row = rsq;
    a.row_begin = 0; a.row_end = nq; a.out_base = 0;
    Want w;
    for (uint32_t q = 0; q < nq; q++) {
        for (uint32_t r = 0; r < nr; r++)
            if (share_a_value(qry[q], ref[ix.rep_h[r]])) w.cand.insert({q, r});
        for (uint64_t v : qry[q])
            for (uint32_t r = 0; r < nr; r++)
                if (ix.rep_h[r] == r && std::binary_search(ref[r].begin(), ref[r].end(), v)) w.shared++;
    }
    w.out.assign((size_t)nq * nr, make_uint2(0, 0));
    for (uint32_t q = 0; q < nq; q++)
        for (uint32_t r = 0; r < nr; r++) w.out[(size_t)q * nr + r] = reference_pair(qry[q], ref[r], s);
    auto prefill = [&](uint2 *out, size_t count) {
        for (size_t k = 0; k < count; k++) out[k] = make_uint2(0u, s);
        launch_sparse_fill_short(out, q_short.p, q_short_cnt.p, (uint32_t)qshort.size(), ix.short_rows.p, ix.short_cnt.p, ix.nshort, 0u, nr, 0u, 0ull, s, nullptr, nullptr);
    };
    auto refp = [&](uint32_t q, uint32_t r) { return reference_pair(qry[q], ref[r], s); };
    return run_stages(what, a, w, forms, small_list, ix.copies ? &ix.rep_h : nullptr, prefill, refp);
}

// ------------------------------------------------------------------------------------------------ the tables
// (tests/test_sparse_merge_gpu.py builds the same tables by the same recipes)

// rows of every length 0 .. s over one pool of 2 s + 3 values; row 0 is full, the last row is not empty
static Rows table_sizes(uint32_t s)
{
    const uint32_t n = std::max(40u, s + 2u), P = 2u * s + 3u;
    Rows t;
    for (uint32_t r = 0; r < n; r++) {
        uint32_t L = s - r % (s + 1u);
        if (r == n - 1u && L == 0) L = s;
        const uint32_t start = (3u * r) % P, step = 1u + (r & 1u);
        Row v;
        for (uint32_t k = 0; k < L; k++) v.push_back(V(1000u + (start + k * step) % P));
        t.push_back(finish_row(v, s));
    }
    return t;
}

static Row span(uint64_t first, uint32_t count, uint64_t stride = 1)
{
    Row v;
    for (uint32_t k = 0; k < count; k++) v.push_back(V(first + k * stride));
    return v;
}
static Row with(Row v, const Row &more) { v.insert(v.end(), more.begin(), more.end()); return v; }

// s = 200: what the ring of 32 codes and its refill of eight a round can meet
static Rows table_ring()
{
    Rows t;
    const Row M = span(20000, 200);
    t.push_back(with(span(0, 199), {M[0]}));                // 0: a column below the row: ib advances 8 every round
    t.push_back(with({M[0]}, span(40000, 199)));            // 1: a column above the row: its ring stalls full
    t.push_back(M);                                         // 2: the row of both
    for (uint32_t run : {9u, 17u, 33u}) {                   // 3 .. 8: runs of 9, 17, 33 values alternate between the two sides
        const uint64_t b = 50000 + 1000 * run;
        Row x = {V(b)}, y = {V(b)};
        for (uint32_t k = 0; x.size() < 200 || y.size() < 200; k++) {
            Row &side = (k / run) % 2 ? y : x;
            if (side.size() < 200) side.push_back(V(b + 1 + k));
        }
        t.push_back(x);
        t.push_back(y);
    }
    t.push_back(span(60000, 200));                          // 9, 10: the same row twice (a class; without classes common = s)
    t.push_back(span(60000, 200));
    // 11 .. 26: a side exhausted at union size 17, 23, 24, 25 = step 1, 7, 8, 9 of a round, as column and as row
    uint64_t b = 61000;
    for (int role = 0; role < 2; role++)
        for (uint32_t u : {17u, 23u, 24u, 25u}) {
            Row lng, sht;
            if (u % 2 == 0) {                               // the shared value first, then the sides alternate: the short side's m-th ends step 2 m
                const uint32_t m = u / 2;
                lng = with({V(b)}, span(b + 2, 199, 2));
                sht = with({V(b)}, span(b + 1, m - 1, 2));
                sht.push_back(V(b + 2 * m - 1));
            } else {                                        // the shared value is the short side's last: step 2 m + 1
                const uint32_t m = (u - 1) / 2;
                lng = span(b + 2, 200, 2);
                sht = with(span(b + 1, m, 2), {V(b + 2 * m + 2)});
            }
            if (role == 0) { t.push_back(sht); t.push_back(lng); } else { t.push_back(lng); t.push_back(sht); }
            b += 1000;
        }
    // 27 .. 91: a row with 64 candidates in one wave -- 63 of them 200 codes from any bound, one with five codes in all
    for (uint32_t c = 0; c < 64; c++) {
        Row v;
        if (c == 40) v = {V(70000), V(70002), V(70005), V(70006), V(70008)};
        else for (uint32_t k = 0; k < 200; k++) v.push_back(V(70000 + 2 * k + ((k + c) % 2)));
        t.push_back(v);
    }
    t.push_back(span(70000, 200, 2));
    return t;
}

// s = 8: rows with 1 .. 256 candidates (the leaves: leaf k shares a tag with every leaf below it) and with exactly 127, 128,
// 129, 256, 257 (the last five rows)
static Rows table_chunks()
{
    const uint32_t ms[5] = {127, 128, 129, 256, 257};
    auto G = [](uint32_t i) { return i < 2 ? V(10 + i) : V(900000 + i); };
    Rows t;
    for (uint32_t k = 0; k < 257; k++) {
        Row v = span(1000 + 10 * k, 3);
        for (uint32_t i = 0; i < 5; i++) if (ms[i] > k) v.push_back(G(i));
        t.push_back(finish_row(v, 8));
    }
    for (uint32_t i = 0; i < 5; i++) t.push_back(finish_row(with({G(i)}, span(500000 + 10 * i, 7)), 8));
    return t;
}

// s = 300: 300 leaves that share nothing with each other, then rows with exactly PACK_COUNTS[i] candidates among the leaves,
// the first of the list last in the table (visited first without an order)
static const uint32_t PACK_COUNTS[25] = {0, 1, 31, 32, 33, 0, 0, 42, 43, 44, 63, 64, 65, 127, 128, 129, 300, 1, 1, 1, 1, 1, 1, 1, 1};
static Rows table_pack()
{
    Rows t;
    for (uint32_t k = 0; k < 300; k++) t.push_back(span(1000 + 32 * k, 25));
    for (int i = 24; i >= 0; i--) {
        Row v = span(100000 + 8 * i, 2);
        for (uint32_t k = 0; k < PACK_COUNTS[i]; k++) v.push_back(V(1000 + 32 * k + i));
        t.push_back(finish_row(v, 300));
    }
    return t;
}

// rows of 2047, 2048, 2049, 4096, 4097 values (at most s) and short ones over one pool, and in front of them four columns
// made for the last row A: denom reaches s exactly at ia = 2048; a column exhausted exactly at the window's edge; a lane
// done in the first window (A's first value) and one that needs the last (A's last value)
static Rows table_windows(uint32_t s)
{
    const uint32_t Ls[8] = {2047, 2048, 2049, 4096, 4097, 5, 100, 0};
    Rows body;
    for (uint32_t r = 0; r < 16; r++) {
        const uint32_t L = std::min(r == 15 ? 4097u : Ls[r % 8], s);
        Row v;
        for (uint32_t k = 0; v.size() < L; k++) if ((k + r) % 4 != 0) v.push_back(V(5000 + k));
        body.push_back(v);
    }
    const Row &A = body.back();
    Rows t;
    if (A.size() >= 2048) {
        t.push_back(with(span(0, s - 2048), {A[2047]}));
        t.push_back(Row(A.begin() + 2040, A.begin() + 2048));
    }
    t.push_back({A[0]});
    t.push_back({A.back()});
    t.insert(t.end(), body.begin(), body.end());
    return t;
}

// s = 40, 110 rows over one pool: classes of 2, 3 and 70 rows, one of them of a short row
static Rows table_copies()
{
    Rows t;
    for (uint32_t r = 0; r < 110; r++) {
        const uint32_t L = 40u - r % 7u, start = (5u * r) % 83u, step = 1u + (r & 1u);
        Row v;
        for (uint32_t k = 0; k < L; k++) v.push_back(V(1000u + (start + k * step) % 83u));
        t.push_back(finish_row(v, 40));
    }
    t[5].resize(3);
    t[107] = t[5];
    t[50] = t[10];
    t[30] = t[11]; t[99] = t[11];
    for (uint32_t r = 35; r < 104; r++) if (r != 50 && r != 99) t[r] = t[34];
    t[104] = t[34]; t[105] = t[34];                         // (rows 50 and 99 are of other classes: 70 rows in all)
    return t;
}

// s = 32: 45 reference rows (a value of its own in front of each and another between the values of an even-numbered pool -- a
// column code without the shared bit behind the column's first chunk --, then values of that pool), copies among them;
// queries below every table value, above every one, between two, equal to a value of one row and of many, empty, and rows of
// the table itself
static void tables_rect(Rows &ref, Rows &qry)
{
    ref.clear(); qry.clear();
    for (uint32_t r = 0; r < 45; r++) {
        const uint32_t L = 31u - r % 5u, start = (7u * r) % 71u, step = 1u + (r & 1u);
        Row v = {V(900 + r), V(1001 + 2 * r)};
        for (uint32_t k = 0; k < L; k++) v.push_back(V(1000u + 2u * ((start + k * step) % 71u)));
        ref.push_back(finish_row(v, 32));
    }
    ref[40] = ref[3]; ref[41] = ref[3]; ref[7] = ref[44];
    qry.push_back(span(0, 32));                                     // below every table value: no candidate
    qry.push_back(with(span(0, 31), {V(900 + 12)}));                // below, and the value row 12 alone holds
    qry.push_back(with({V(1000 + 2 * 20)}, span(5000, 31)));        // a value many rows hold, then above every table value
    qry.push_back(span(1091, 26, 2));                               // between two table values, all of them: no candidate
    qry.push_back(span(1000, 32));                                  // found and not found in turn
    qry.push_back({});                                              // empty
    qry.push_back(with({V(900 + 3)}, span(6000, 3)));               // the value of a class of three reference rows
    qry.push_back({V(1000 + 2 * 70)});
    for (uint32_t r : {0u, 3u, 7u, 20u, 44u}) qry.push_back(ref[r]);
    for (uint32_t r = 0; r < 45; r += 4) { Row v = ref[r]; v.resize(v.size() / 2 + r % 3); qry.push_back(with(v, span(1001 + 2 * r, 6, 2))); }
    for (Row &v : qry) v = finish_row(v, 32);
}

// s = 64: runs of 6, 7, 64, 65, 129, 200 rows below the last row; rows with 3, 4, 5, 9 runs of ten among their 64 entries
static Rows table_runs()
{
    const uint32_t Ls[6] = {6, 7, 64, 65, 129, 200};
    Rows t;
    for (uint32_t k = 0; k < 200; k++) {
        Row v = span(100000 + 4 * k, 2);
        for (uint32_t i = 0; i < 6; i++) if (Ls[i] > k) v.push_back(V(10 + i));
        if (k < 10) v = with(v, span(50, 9));
        t.push_back(finish_row(v, 64));
    }
    for (uint32_t m : {3u, 4u, 5u, 9u}) t.push_back(finish_row(with(span(50, m), span(200000 + 100 * m, 64 - m)), 64));
    t.push_back(finish_row(with(span(10, 6), span(300000, 20)), 64));
    return t;
}

// s = 2, 8194 rows: row 8192 marks 8192 columns (256 bitmap words, one per thread), row 8193 marks 8193 (257 words, two)
static Rows table_bitmap()
{
    Rows t;
    for (uint32_t k = 0; k < 8194; k++) t.push_back({V(k >= 8191 ? 42 : k % 50), V(100 + k)});
    return t;
}

static Rows pool_rows(uint32_t n, uint32_t s, std::mt19937_64 &rng, double pool_factor, double keep, bool ragged)
{
    Row pool;
    for (uint32_t k = 0; k < (uint32_t)(pool_factor * s) + 4; k++) pool.push_back(rng() >> 10);
    Rows rows;
    for (uint32_t i = 0; i < n; i++) {
        Row v;
        for (uint64_t x : pool)
            if ((double)(rng() % 10000) < keep * 10000.0) v.push_back(x);
        for (uint32_t k = 0; k < s / 10 + 1; k++) v.push_back(rng() >> 10);
        uint32_t kn = s;
        if (ragged && rng() % 2) kn = (uint32_t)(rng() % (s + 1));
        rows.push_back(finish_row(v, kn));
    }
    return rows;
}

// a tree of descent: slot k of a row holds a value of stratum k; on every edge a share of the slots is replaced
static Rows tree_rows(uint32_t n, uint32_t s, std::mt19937_64 &rng, double q, bool ragged)
{
    uint32_t L = 1;
    while ((1u << L) < n) L++;
    const uint64_t salt = rng();
    Rows rows;
    for (uint32_t i = 0; i < n; i++) {
        Row v(s);
        for (uint32_t k = 0; k < s; k++) {
            uint64_t origin = 0;
            for (uint32_t lev = 1; lev <= L; lev++) {
                const uint64_t anc = i >> (L - lev);
                std::mt19937_64 h(salt ^ ((uint64_t)k * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)lev << 50) ^ (anc * 0xC2B2AE3D27D4EB4Full));
                if ((double)(h() >> 11) / 9007199254740992.0 < q) origin = ((uint64_t)lev << 40) | anc;
            }
            std::mt19937_64 h2(salt ^ ((uint64_t)k * 0xC2B2AE3D27D4EB4Full) ^ (origin * 0x9E3779B97F4A7C15ull));
            v[k] = ((uint64_t)k << 40) + (h2() & ((1ull << 40) - 1));
        }
        uint32_t keep = s;
        if (ragged && rng() % 3 == 0) keep = (uint32_t)(rng() % (s + 1));
        rows.push_back(finish_row(v, keep));
    }
    std::shuffle(rows.begin(), rows.end(), rng);
    return rows;
}

static int check_takes_part(const char *what, const Rows &t, uint32_t s)
{
    const Rows c = clipped(t, s);
    bool first = false, last = false;
    for (size_t j = 1; j < c.size(); j++) first = first || share_a_value(c[0], c[j]);
    for (size_t j = 0; j + 1 < c.size(); j++) last = last || share_a_value(c.back(), c[j]);
    if (!first || !last) { fprintf(stderr, "%s: row 0 or the last row shares nothing (a fault of the table)\n", what); return 1; }
    return 0;
}

int main(int argc, char **argv)
{
    signal(SIGSEGV, on_fault);
    signal(SIGBUS, on_fault);
    const std::string which = argc > 1 ? argv[1] : "sizes";
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    std::mt19937_64 rng(seed * 0x9E3779B97F4A7C15ull + 7);
    const auto t0 = std::chrono::steady_clock::now();
    int bad = 0;
    char what[160];
    if (which == "sizes") {
        for (uint32_t s : {1u, 3u, 4u, 5u, 7u, 8u, 9u, 15u, 16u, 17u, 24u, 25u, 31u, 32u, 33u, 40u, 63u, 64u, 65u}) {
            const Rows t = table_sizes(s);
            snprintf(what, sizeof what, "sizes, s %u", s);
            bad += check_takes_part(what, t, s);
            TriOpt o;
            bad += run_triangle(what, t, s, o, rng);
            if (s == 1) {                                   // (two rows of one value that share it are copies: the merge runs without classes only)
                o.dedup = false;
                bad += run_triangle("sizes, s 1, no classes", t, s, o, rng);
            }
        }
    } else if (which == "ring") {
        const Rows t = table_ring();
        TriOpt o;
        bad += run_triangle("ring", t, 200, o, rng);
        o.dedup = false;                                    // (the identical pair goes through the merge: common = s)
        bad += run_triangle("ring, no classes", t, 200, o, rng);
        o.rb = 20; o.re = 60; o.order = true;
        bad += run_triangle("ring, rows [20, 60) in an order", t, 200, o, rng);
    } else if (which == "chunks") {
        const Rows t = table_chunks();
        TriOpt o;
        bad += run_triangle("chunks", t, 8, o, rng);
        o.rb = 120; o.re = 262; o.order = true;
        bad += run_triangle("chunks, rows [120, 262) in an order", t, 8, o, rng);
    } else if (which == "pack") {
        const Rows t = table_pack();
        TriOpt o;
        bad += run_triangle("pack", t, 300, o, rng);        // visiting order: the table's last row first = PACK_COUNTS as listed
        o.rb = 300; o.re = 325;
        bad += run_triangle("pack, rows [300, 325)", t, 300, o, rng);
        o.rb = 0; o.re = 0; o.order = true;
        bad += run_triangle("pack, in an order", t, 300, o, rng);
        const uint32_t most[3] = {5, 4, 3};
        for (int k = 0; k < 3; k++)
            if (g_t.max_pack_rows[k] != most[k]) { fprintf(stderr, "pack: no item of %s stages %u rows (most: %u; a fault of the table)\n", form_name[3 + k], most[k], g_t.max_pack_rows[k]); bad++; }
    } else if (which == "windows") {
        for (uint32_t s : {2044u, 2048u, 2052u, 2053u, 4096u, 4100u}) {
            snprintf(what, sizeof what, "windows, s %u", s);
            TriOpt o;
            bad += run_triangle(what, table_windows(s), s, o, rng);
        }
        // the windowed form where a row is one window
        TriOpt o;
        o.forms = F_LANES | F_WIN;
        for (uint32_t s : {1u, 4u, 7u, 9u, 33u, 64u}) { snprintf(what, sizeof what, "windows on sizes, s %u", s); bad += run_triangle(what, table_sizes(s), s, o, rng); }
        o.dedup = false;
        bad += run_triangle("windows on ring", table_ring(), 200, o, rng);
    } else if (which == "copies") {
        const Rows t = table_copies();
        TriOpt o;
        bad += run_triangle("copies", t, 40, o, rng);
        o.rb = 60; o.re = 100;
        bad += run_triangle("copies, rows [60, 100) cut the class of 70", t, 40, o, rng);
        o.order = true;
        o.forms = F_LANES | F_ROWS | F_P43;
        bad += run_triangle("copies, rows [60, 100) in an order", t, 40, o, rng);
        o = TriOpt();
        o.forms = F_LANES | F_WIN | F_P64;
        o.permute = true;
        bad += run_triangle("copies, permuted index", t, 40, o, rng);
        o.dedup = false; o.permute = false;
        bad += run_triangle("copies, no classes", t, 40, o, rng);
    } else if (which == "rect") {
        Rows ref, qry;
        tables_rect(ref, qry);
        bad += run_rect("rect", ref, qry, 32, 32, F_ALL, true);
        bad += run_rect("rect, queries of sketch size 20", ref, qry, 32, 20, F_ALL);
        bad += run_rect("rect, queries of sketch size 48", ref, qry, 32, 48, F_ALL);
        for (uint32_t nr : {31u, 32u, 33u}) {
            snprintf(what, sizeof what, "rect, %u columns", nr);
            bad += run_rect(what, Rows(ref.begin(), ref.begin() + nr), qry, 32, 32, F_LANES | F_P43);
        }
    } else if (which == "discover") {
        const Rows t = table_runs();
        TriOpt o;
        o.small_list = true;
        bad += run_triangle("discover, runs", t, 64, o, rng);
        o.permute = true; o.order = true;
        bad += run_triangle("discover, runs, permuted index in an order", t, 64, o, rng);
        o = TriOpt();
        o.forms = F_LANES | F_P32;
        for (uint32_t n : {32u, 33u, 34u}) {                 // the last row marks 31, 32, 33 columns
            snprintf(what, sizeof what, "discover, %u columns", n - 1);
            Rows u(t.begin(), t.begin() + n - 1);
            u.push_back(t.back());
            bad += run_triangle(what, u, 64, o, rng);
        }
        o.no_out = true;                                    // (33 million pairs: the candidates and their results only)
        o.rb = 8100;
        bad += run_triangle("discover, 8192 and 8193 columns", table_bitmap(), 2, o, rng);
    } else if (which == "fuzz") {
        const int cases = argc > 3 ? atoi(argv[3]) : 10;
        for (int c = 0; c < cases && !bad; c++) {
            uint32_t n = 2 + (uint32_t)(rng() % 299), s = 1 + (uint32_t)(rng() % 150);
            if (rng() % 12 == 0) { s = 2053 + (uint32_t)(rng() % 300); n = 2 + (uint32_t)(rng() % 24); }
            const int kind = (int)(rng() % 3);
            Rows t = kind == 0 ? tree_rows(n, s, rng, 0.02 + (double)(rng() % 30) / 100.0, rng() % 2)
                               : pool_rows(n, s, rng, 1.0 + (double)(rng() % 300) / 100.0, 0.1 + (double)(rng() % 89) / 100.0, rng() % 2);
            if (kind == 2) for (uint32_t k = 0; k < n / 6 + 1; k++) t[(size_t)(rng() % n)] = t[(size_t)(rng() % n)];
            const unsigned forms = F_LANES | (2u << (rng() % 5));
            if (rng() % 3 == 0) {
                const uint32_t nq = 1 + (uint32_t)(rng() % 40), sq = rng() % 2 ? s : 1 + (uint32_t)(rng() % (2 * s));
                Rows q = pool_rows(nq, sq, rng, 1.5, 0.5, true);
                for (uint32_t k = 0; k < nq; k += 3) q[k] = t[(size_t)(rng() % n)];
                snprintf(what, sizeof what, "fuzz %d (rect, %u rows, %u queries, s %u, sq %u, kind %d, forms %u)", c, n, nq, s, sq, kind, forms);
                bad += run_rect(what, t, q, s, sq, forms, rng() % 2);
            } else {
                TriOpt o;
                o.forms = forms;
                if (rng() % 2) { o.rb = (uint32_t)(rng() % n); o.re = o.rb + 1 + (uint32_t)(rng() % (n - o.rb)); }
                o.permute = o.rb == 0 && o.re == 0 && rng() % 2;
                o.order = rng() % 2;
                o.dedup = rng() % 4 != 0;
                o.small_list = rng() % 2;
                snprintf(what, sizeof what, "fuzz %d (n %u, s %u, kind %d, rows [%u, %u), forms %u, permuted %d, order %d, classes %d)", c, n, s, kind, o.rb, o.re, forms, o.permute, o.order, o.dedup);
                bad += run_triangle(what, t, s, o, rng);
            }
        }
    } else {
        fprintf(stderr, "unknown case %s\n", which.c_str());
        return 2;
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%s: %llu pairs of output, %llu candidates, %llu merge launches compared, %llu declined, %d differ (%.1f s)\n", which.c_str(), (unsigned long long)g_t.pairs,
           (unsigned long long)g_t.cands, (unsigned long long)g_t.forms_run, (unsigned long long)g_t.declined, bad, secs);
    if (bad == 0) printf("all cases agree\n");
    return bad ? 1 : 0;
}
