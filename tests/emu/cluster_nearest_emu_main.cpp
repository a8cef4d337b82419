// cluster_nearest_emu_main.cpp -- runs the kernels of `mash cluster -B`, unchanged, through their launchers on the CPU (tools/hipemu):
// cf_append_kernel (cluster_forest.hip) over ballot words in list mode and in flat triangle mode, the rounds of cluster_greedy.hip
// over the list WITH counts (cg_round_edges_kernel<uint4>), and launch_nearest_assign (cg_rep_init_kernel, cn_key_kernel,
// cn_rep_kernel).  The judge is a sequential restatement written here: the walk in index order, then per member the best of all its
// edges to a representative by forest_before with the representative as the tie-break.  The driver does what the host does: append
// per launch, regrow and append again when the list overflows, rounds in batches until one leaves no row open, the assignment.
// Every case also goes through the list WITHOUT counts (cg_append_kernel, cg_round_edges_kernel<uint2>, cg_assign_kernel) and must
// give the walk's first representative: the path of `mash cluster -R` is what it was.
// TEST INFRASTRUCTURE (tests/test_cluster_nearest_emu.py); built with g++.  The emulator runs workgroups one after another: what is
// pinned here is the arithmetic (which end is the member, the keys, the ties, padding, the places in the list), not the races
// between workgroups.
//
//   cluster_nearest_emu <case>            cases: small star between ties zero band lengths padding overflow
//   cluster_nearest_emu fuzz <seed> <n>   n random jobs
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <cmath>
#include <random>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../mash_amd/csrc/cluster.hip"
#include "../../mash_amd/csrc/cluster_forest.hip"
#include "../../mash_amd/csrc/cluster_greedy.hip"

using namespace mg;

struct Edge { uint32_t row, col, numer, denom; };
static bool same(const Edge &a, const Edge &b) { return a.row == b.row && a.col == b.col && a.numer == b.numer && a.denom == b.denom; }
static bool by_fields(const Edge &a, const Edge &b)
{
    return a.row != b.row ? a.row < b.row : a.col != b.col ? a.col < b.col : a.numer != b.numer ? a.numer < b.numer : a.denom < b.denom;
}

// one append launch: a list of pairs with their counts and a mask, or rows [first_row, row_end) of the flat triangle with a mask
struct Launch {
    std::vector<uint2> rc;                       // list mode (empty: flat)
    std::vector<uint2> counts;                   // {numer, denom} of every pair of the launch, marked or not
    uint64_t first_row = 0, pairs = 0;
    std::vector<unsigned long long> masks;
    void set(uint64_t idx) { masks[idx >> 6] |= 1ull << (idx & 63); }
    bool get(uint64_t idx) const { return (masks[idx >> 6] >> (idx & 63)) & 1ull; }
};

static uint64_t tri(uint64_t r) { return r ? r * (r - 1) / 2 : 0; }

// every pair carries counts, also the ones no bit marks: they must not reach the list
static uint2 junk_counts(uint64_t idx) { return make_uint2((uint32_t)(idx * 7 % 61), 61u); }

static Launch list_launch(const std::vector<Edge> &pairs)
{
    Launch L;
    for (const Edge &e : pairs) {
        L.rc.push_back(make_uint2(e.row, e.col));
        L.counts.push_back(make_uint2(e.numer, e.denom));
    }
    L.pairs = pairs.size();
    L.masks.assign((L.pairs + 63) / 64, 0);
    return L;
}

static Launch list_all(const std::vector<Edge> &e)
{
    Launch L = list_launch(e);
    for (uint64_t i = 0; i < L.pairs; i++) L.set(i);
    return L;
}

static Launch flat_launch(uint64_t first_row, uint64_t row_end)
{
    Launch L;
    L.first_row = first_row;
    L.pairs = tri(row_end) - tri(first_row);
    L.masks.assign((L.pairs + 63) / 64, 0);
    L.counts.resize(L.pairs);
    for (uint64_t i = 0; i < L.pairs; i++) L.counts[i] = junk_counts(i);
    return L;
}

static void flat_set(Launch &L, const Edge &e)
{
    const uint64_t idx = tri(e.row) + e.col - tri(L.first_row);
    L.set(idx);
    L.counts[idx] = make_uint2(e.numer, e.denom);
}

// what a launch must leave in the list, by the definition of the layouts (not by pair_rc), as {larger, smaller, numer, denom}; a
// marked pair with an end outside the table of n rows is a padding entry, all zero
static void entries_of(const Launch &L, uint32_t n, std::vector<Edge> &out)
{
    if (!L.rc.empty()) {
        for (uint64_t i = 0; i < L.pairs; i++) {
            if (!L.get(i)) continue;
            if (L.rc[i].x >= n || L.rc[i].y >= n) out.push_back({0, 0, 0, 0});
            else out.push_back({std::max(L.rc[i].x, L.rc[i].y), std::min(L.rc[i].x, L.rc[i].y), L.counts[i].x, L.counts[i].y});
        }
        return;
    }
    uint64_t row = L.first_row, col = 0;
    if (row == 0) row = 1;
    for (uint64_t i = 0; i < L.pairs; i++) {
        if (L.get(i)) out.push_back({(uint32_t)row, (uint32_t)col, L.counts[i].x, L.counts[i].y});
        if (++col == row) { row++; col = 0; }
    }
}

static int failures = 0;
constexpr uint32_t GUARD = 0xDEADBEEFu;
constexpr unsigned long long GUARD64 = 0xDEADBEEFDEADBEEFull;

// the judge.  first[i]: the walk (`mash cluster -R`); near[i]: the same representatives, members under the best of ALL their edges
static void judge(uint32_t n, const std::vector<Edge> &edges, std::vector<uint32_t> &first, std::vector<uint32_t> &near)
{
    std::vector<std::vector<uint32_t>> smaller(n);
    for (const Edge &e : edges) smaller[e.row].push_back(e.col);
    first.assign(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        first[i] = i;
        for (uint32_t j : smaller[i])
            if (first[j] == j && (first[i] == i || j < first[i])) first[i] = j;
    }
    near.assign(n, 0);
    std::vector<const Edge *> best(n, nullptr);
    for (uint32_t i = 0; i < n; i++) near[i] = i;
    for (const Edge &e : edges) {
        const bool rr = first[e.row] == e.row, cr = first[e.col] == e.col;
        if (rr == cr) continue;
        const uint32_t member = rr ? e.col : e.row, rep = rr ? e.row : e.col;
        if (!best[member] || forest_before(e.numer, e.denom, rep, best[member]->numer, best[member]->denom, near[member])) {
            best[member] = &e;
            near[member] = rep;
        }
    }
}

// E: uint4 (with counts) or uint2; one append with the host's regrow
static hipError_t append(const FinishArgs &a, uint32_t n, uint4 *l, uint64_t cap, unsigned long long *cur, uint32_t *ov) { return launch_forest_append(a, n, l, cap, cur, ov, nullptr); }
static hipError_t append(const FinishArgs &a, uint32_t n, uint2 *l, uint64_t cap, unsigned long long *cur, uint32_t *ov) { return launch_greedy_append(a, n, l, cap, cur, ov, nullptr); }
static uint4 guard_of(uint4 *) { return make_uint4(GUARD, GUARD, GUARD, GUARD); }
static uint2 guard_of(uint2 *) { return make_uint2(GUARD, GUARD); }
static Edge edge_of(const uint4 &x) { return {x.x, x.y, x.z, x.w}; }
static Edge edge_of(const uint2 &x) { return {x.x, x.y, 0, 0}; }

struct Outcome { bool ok = true; uint64_t used = 0, regrows = 0, rounds = 0; std::vector<uint32_t> state; };

template <class E>
static Outcome fill_and_rounds(uint32_t n, const std::vector<Launch> &launches, uint64_t first_cap, uint64_t total, std::vector<E> &list, uint64_t &cap)
{
    constexpr bool counts = sizeof(E) == 16;
    Outcome o;
    cap = first_cap ? first_cap : std::max<uint64_t>(total, 1);
    list.assign(cap + 1, guard_of((E *)nullptr));
    unsigned long long cursor = 0;
    uint32_t overflow = 0;
    bool &ok = o.ok;
    for (const Launch &L : launches) {
        FinishArgs a{};
        a.pairs = L.pairs;
        a.first_row = L.first_row;
        a.triangle = 1;
        a.counts = L.counts.data();
        a.masks = const_cast<unsigned long long *>(L.masks.data());
        a.list_rc = L.rc.empty() ? nullptr : L.rc.data();
        std::vector<Edge> mine;
        entries_of(L, n, mine);
        if (!counts) for (Edge &e : mine) e.numer = e.denom = 0;
        for (int attempt = 0;; attempt++) {
            ok = ok && append(a, n, list.data(), cap, &cursor, &overflow) == hipSuccess;
            ok = ok && list[cap].x == GUARD && list[cap].y == GUARD;                // never a word behind the list
            ok = ok && cursor == o.used + mine.size() && (overflow != 0) == (cursor > cap);
            if (cursor <= cap) break;
            if (attempt) { ok = false; break; }
            const uint64_t bigger = std::max<uint64_t>(cursor, 2 * cap);          // regrow: the earlier launches' edges move over
            std::vector<E> nl(bigger + 1, guard_of((E *)nullptr));
            std::copy(list.begin(), list.begin() + (long)o.used, nl.begin());
            list.swap(nl);
            cap = bigger;
            cursor = o.used;
            overflow = 0;
            o.regrows++;
        }
        std::vector<Edge> got;
        for (uint64_t i = o.used; i < cursor && i < cap; i++) got.push_back(edge_of(list[i]));
        std::sort(got.begin(), got.end(), by_fields);
        std::sort(mine.begin(), mine.end(), by_fields);
        ok = ok && got.size() == mine.size() && std::equal(got.begin(), got.end(), mine.begin(), same);
        o.used = cursor;
    }
    o.state.assign(n + 1, 0);
    o.state[n] = GUARD;
    std::vector<uint32_t> left(257, GUARD);
    bool done = n == 0;
    for (uint32_t batch = 8; !done; batch = std::min(batch * 2, 256u)) {
        ok = ok && launch_greedy_rounds(list.data(), o.used, o.state.data(), n, left.data(), batch, nullptr) == hipSuccess;
        ok = ok && left[batch] == GUARD;
        uint32_t r = 0;
        while (r < batch && left[r]) r++;
        o.rounds += std::min(r + 1, batch);
        for (uint32_t k = r + 1; k < batch; k++) ok = ok && left[k] == 0;           // rounds behind the fixpoint do nothing
        done = r < batch;
        if (o.rounds > n) { ok = false; break; }                                    // at most n rounds, ever
    }
    for (uint32_t i = 0; i < n; i++) ok = ok && (o.state[i] == 2 || o.state[i] == 3);
    ok = ok && o.state[n] == GUARD && list[cap].x == GUARD;
    return o;
}

// first_cap: the first capacity of the edge list (0: room for everything); want: the expected rep where the case knows it in closed form
static void check(const char *name, uint32_t n, const std::vector<Launch> &launches, uint64_t first_cap = 0, bool want_regrow = false,
                  const std::vector<uint32_t> *want = nullptr)
{
    std::vector<Edge> entries, edges;
    for (const Launch &L : launches) entries_of(L, n, entries);
    for (const Edge &e : entries)
        if (e.row > e.col) edges.push_back(e);
    std::vector<uint32_t> first, near;
    judge(n, edges, first, near);
    uint64_t want_reps = 0, moved = 0, later = 0;
    for (uint32_t i = 0; i < n; i++) {
        want_reps += near[i] == i;
        moved += near[i] != first[i];
        later += near[i] > i;
    }
    bool ok = !want || *want == near;                                               // the judge itself against the closed form

    // with counts: the nearest representative
    std::vector<uint4> list4;
    uint64_t cap4 = 0;
    Outcome o4 = fill_and_rounds(n, launches, first_cap, entries.size(), list4, cap4);
    std::vector<uint32_t> rep(n + 1, GUARD);
    std::vector<unsigned long long> best_key(n + 1, GUARD64);
    unsigned long long reps = ~0ull;
    ok = ok && o4.ok && launch_nearest_assign(list4.data(), o4.used, o4.state.data(), n, best_key.data(), rep.data(), &reps, nullptr) == hipSuccess;
    ok = ok && o4.state[n] == GUARD && rep[n] == GUARD && best_key[n] == GUARD64 && list4[cap4].x == GUARD;      // nothing written behind the arrays
    uint64_t bad = 0;
    for (uint32_t i = 0; i < n; i++) bad += rep[i] != near[i];
    ok = ok && reps == want_reps;

    // without counts: the first representative, as before
    std::vector<uint2> list2;
    uint64_t cap2 = 0;
    Outcome o2 = fill_and_rounds(n, launches, first_cap, entries.size(), list2, cap2);
    std::vector<uint32_t> rep2(n + 1, GUARD);
    unsigned long long reps2 = ~0ull;
    ok = ok && o2.ok && launch_greedy_assign(list2.data(), o2.used, o2.state.data(), n, rep2.data(), &reps2, nullptr) == hipSuccess;
    ok = ok && rep2[n] == GUARD && reps2 == want_reps && o2.state == o4.state;   // (the number of rounds may differ where work-items are threads)
    uint64_t bad2 = 0;
    for (uint32_t i = 0; i < n; i++) bad2 += rep2[i] != first[i];

    const bool shaped = !want_regrow || (o4.regrows > 0 && o2.regrows > 0);
    if (!ok || bad || bad2 || !shaped) {
        failures++;
        printf("FAIL %s: n %u edges %zu: %llu reps differ (nearest), %llu (first), clusters %llu want %llu, rounds %llu, regrows %llu%s\n", name, n,
               edges.size(), (unsigned long long)bad, (unsigned long long)bad2, reps, (unsigned long long)want_reps, (unsigned long long)o4.rounds,
               (unsigned long long)o4.regrows, ok ? "" : " (launch, guard word, list content, counts or closed form)");
    } else {
        printf("ok   %s: n %u edges %zu clusters %llu rounds %llu regrows %llu, %llu members not under their first representative, %llu under a later one\n",
               name, n, edges.size(), (unsigned long long)want_reps, (unsigned long long)o4.rounds, (unsigned long long)o4.regrows,
               (unsigned long long)moved, (unsigned long long)later);
    }
}

static void case_star()
{
    // a star around row 0 makes rows 1 .. 999 its members; row 1234 is beside all of them and beside nothing else below it, so the
    // walk makes it a representative -- in the MIDDLE of the index range, with a better fraction to rows 1 .. 999 than row 0 has:
    // they must join it from below (the representative is `hi` of those edges), as rows 2000 .. 2999 do from above
    const uint32_t n = 3000, c = 1234;
    std::vector<Edge> e;
    for (uint32_t i = 1; i < 1000; i++) e.push_back({i, 0, 10, 64});
    for (uint32_t i = 1; i < 1000; i++) e.push_back({c, i, 11 + i % 3, 64});        // row c is above them: the representative is `hi`
    for (uint32_t i = 2000; i < n; i++) e.push_back({i, c, 20, 64});
    std::vector<uint32_t> want(n);
    for (uint32_t i = 0; i < n; i++) want[i] = (i >= 1 && i < 1000) || i >= 2000 ? c : i;
    check("star around a middle row, list", n, {list_all(e)}, 0, false, &want);
    Launch F = flat_launch(0, n);
    for (const Edge &x : e) flat_set(F, x);
    check("star around a middle row, flat", n, {F}, 0, false, &want);
    std::reverse(e.begin(), e.end());
    check("star around a middle row, list backwards", n, {list_all(e)}, 0, false, &want);
}

static void case_between()
{
    // rows 0 and 2 are representatives (no edge between them), row 1 the member between them
    std::vector<uint32_t> later{0, 2, 2}, earlier{0, 0, 2};
    check("the better representative is the later one", 3, {list_all({{1, 0, 30, 64}, {2, 1, 31, 64}})}, 0, false, &later);
    check("the better representative is the earlier one", 3, {list_all({{1, 0, 31, 64}, {2, 1, 30, 64}})}, 0, false, &earlier);
    check("later, edges named the other way round", 3, {list_all({{1, 2, 31, 64}, {0, 1, 30, 64}})}, 0, false, &later);
    // many members between the same two, alternately nearer to one and the other: rows 1 .. 998 between 0 and 999
    const uint32_t n = 1000;
    std::vector<Edge> e;
    std::vector<uint32_t> want(n);
    for (uint32_t i = 1; i + 1 < n; i++) {
        e.push_back({i, 0, 40 + (i & 1), 64});
        e.push_back({n - 1, i, 40 + (~i & 1), 64});
        want[i] = i & 1 ? 0 : n - 1;
    }
    want[0] = 0;
    want[n - 1] = n - 1;
    check("998 members between two representatives", n, {list_all(e)}, 0, false, &want);
}

static void case_ties()
{
    std::vector<uint32_t> smaller{0, 0, 2};
    check("32/64 beside 16/32", 3, {list_all({{1, 0, 32, 64}, {2, 1, 16, 32}})}, 0, false, &smaller);
    check("16/32 beside 32/64", 3, {list_all({{1, 0, 16, 32}, {2, 1, 32, 64}})}, 0, false, &smaller);
    check("0/64 beside 0/0", 3, {list_all({{1, 0, 0, 64}, {2, 1, 0, 0}})}, 0, false, &smaller);
    check("0/0 beside 0/64", 3, {list_all({{1, 0, 0, 0}, {2, 1, 0, 64}})}, 0, false, &smaller);
    std::vector<uint32_t> larger{0, 2, 2};
    check("31/64 beside 16/32", 3, {list_all({{1, 0, 31, 64}, {2, 1, 16, 32}})}, 0, false, &larger);
    check("0/64 beside 1/2000000", 3, {list_all({{1, 0, 0, 64}, {2, 1, 1, 2000000}})}, 0, false, &larger);
    check("2097150/2097151 beside 2097149/2097150", 3, {list_all({{1, 0, 2097149, 2097150}, {2, 1, 2097150, 2097151}})}, 0, false, &larger);
    // a tie among five representatives of a member in their middle: rows 0 .. 4 and 6 .. 9 have no edge among them
    std::vector<Edge> e;
    for (uint32_t i = 0; i < 10; i++)
        if (i != 5) e.push_back({std::max(i, 5u), std::min(i, 5u), i == 3 || i == 7 || i == 8 ? 6u : 5u, i == 7 ? 10u : i == 8 ? 20u : 10u});
    std::vector<uint32_t> want{0, 1, 2, 3, 4, 3, 6, 7, 8, 9};                      // 6/10 at 3 and 7, 6/20 at 8: the smaller of 3 and 7
    check("a tie among representatives on both sides", 10, {list_all(e)}, 0, false, &want);
}

static void case_zero()
{
    std::vector<uint32_t> w2{0, 0};
    check("a numer == 0 edge is the member's only edge", 2, {list_all({{1, 0, 0, 64}})}, 0, false, &w2);
    check("0/0 is the member's only edge", 2, {list_all({{0, 1, 0, 0}})}, 0, false, &w2);
    std::vector<uint32_t> w3{0, 1, 1};
    check("a numer == 0 edge between rows 1 and 2 of 3", 3, {list_all({{2, 1, 0, 64}})}, 0, false, &w3);
    const uint32_t n = 500;                                                        // every edge 0/64: the first rule and the nearest one agree
    std::vector<Edge> e;
    for (uint32_t i = 1; i < n; i++) { e.push_back({i, i / 2, 0, 64}); e.push_back({i, i - 1, 0, 64}); }
    std::sort(e.begin(), e.end(), by_fields);
    e.erase(std::unique(e.begin(), e.end(), same), e.end());
    check("every edge carries 0/64", n, {list_all(e)});
}

// window_table semantics: row i beside rows i - 1 .. i - 3, sharing s - k * step of s
static std::vector<uint32_t> band_want(uint32_t n)
{
    std::vector<uint32_t> want(n);
    for (uint32_t i = 0; i < n; i++) want[i] = i % 4 == 3 && i + 1 < n ? i + 1 : i - i % 4;
    return want;
}

static void case_band()
{
    for (uint32_t n : {300u, 301u, 302u, 303u, 2500u}) {
        const std::vector<uint32_t> want = band_want(n);
        Launch F = flat_launch(0, n);
        std::vector<Edge> e;
        for (uint32_t i = 1; i < n; i++)
            for (uint32_t k = 1; k <= 3 && k <= i; k++) { flat_set(F, {i, i - k, 1000 - 100 * k, 1000}); e.push_back({i, i - k, 1000 - 100 * k, 1000}); }
        check(("band of " + std::to_string(n) + " rows, flat").c_str(), n, {F}, 0, false, &want);
        if (n <= 303) check(("band of " + std::to_string(n) + " rows, list").c_str(), n, {list_all(e)}, 0, false, &want);
    }
}

static std::vector<Edge> random_pairs(std::mt19937_64 &rng, uint32_t n, uint64_t K, uint32_t fam)
{
    std::vector<Edge> q;
    for (uint64_t i = 0; i < K; i++) {
        const uint32_t a = 1 + (uint32_t)(rng() % (n - 1));
        uint32_t b = (uint32_t)(rng() % a);
        b -= std::min(b, (b % fam + fam - a % fam) % fam);
        const uint32_t d = rng() % 4 ? 64u : (uint32_t)(rng() % 3) * 32u;           // 64 mostly; 0, 32 and 64 otherwise
        const uint32_t m = d ? (uint32_t)(rng() % 5) * (d / 4) : 0u;                // quarters: ties are common, also across denominators
        if (rng() % 2) q.push_back({a, b, m, d}); else q.push_back({b, a, m, d});   // a list names a pair either way round
    }
    return q;
}

// a pair is named once in a job (it is one pair of a triangle): later copies are unmarked
static void mark_distinct(Launch &L, std::mt19937_64 &rng, double dens, std::unordered_set<uint64_t> &seen)
{
    for (uint64_t i = 0; i < L.pairs; i++) {
        const uint32_t hi = std::max(L.rc[i].x, L.rc[i].y), lo = std::min(L.rc[i].x, L.rc[i].y);
        const uint64_t key = (uint64_t)hi << 32 | lo;
        if (hi == lo || (double)(rng() % 1000000) >= dens * 1e6 || seen.count(key)) continue;
        seen.insert(key);
        L.set(i);
    }
}

static void case_lengths()
{
    std::mt19937_64 rng(29);
    for (uint32_t K : {1u, 37u, 63u, 64u, 65u, 255u, 257u, 4097u}) {                // lists whose length is not a multiple of 64 (or of 256)
        Launch Q = list_launch(random_pairs(rng, 900, K, 3));
        std::unordered_set<uint64_t> seen;
        mark_distinct(Q, rng, 0.6, seen);
        check(("list of " + std::to_string(K) + " pairs").c_str(), 900, {Q});
    }
}

static void case_padding()
{
    // marked pairs with an end outside the table become {0, 0, 0, 0}: hi == lo, skipped by the rounds and by both passes -- also
    // where row 0 is a member, a representative, or has junk counts beside it
    std::vector<Edge> e{{1, 0, 30, 64}, {2, 1, 31, 64}, {7, 1, 64, 64}, {3, 9, 64, 64}, {4, 3, 5, 64}, {5, 5, 64, 64}};
    Launch L = list_launch(e);
    for (uint64_t i = 0; i < L.pairs; i++)
        if (e[i].row != e[i].col) L.set(i);
    std::vector<uint32_t> want{0, 2, 2, 3, 3};
    check("pairs outside a table of 5 rows", 5, {L}, 0, false, &want);
    std::mt19937_64 rng(31);
    std::vector<Edge> q = random_pairs(rng, 1200, 5000, 4);                          // rows up to 1199 over a table of 800
    Launch Q = list_launch(q);
    std::unordered_set<uint64_t> seen;
    mark_distinct(Q, rng, 0.7, seen);
    check("a third of the pairs outside a table of 800 rows", 800, {Q});
    check("the same, a list of 1 edge at first", 800, {Q}, 1, true);
}

static std::vector<Launch> five_blocks(uint32_t n, uint64_t seed)
{
    std::mt19937_64 rng(seed);
    std::vector<Launch> v;
    for (auto rb : {std::make_pair(0u, 1u), std::make_pair(1u, 700u), std::make_pair(700u, 701u), std::make_pair(701u, n - 1), std::make_pair(n - 1, n)}) {
        Launch F = flat_launch(rb.first, rb.second);
        for (uint32_t r = std::max(rb.first, 1u); r < rb.second; r++)
            for (int k = 0; k < 3; k++) {
                const uint32_t c = (uint32_t)(rng() % r);
                if ((r % 7) == (c % 7)) flat_set(F, {r, c, (uint32_t)(rng() % 5) * 16u, 64u});
            }
        if (rb.second == n) { flat_set(F, {n - 1, 3, 1, 64}); flat_set(F, {n - 1, 4, 2, 64}); flat_set(F, {n - 1, n - 2, 2, 64}); }
        v.push_back(F);
    }
    return v;
}

static void case_overflow()
{
    check("five row blocks, one list", 1500, five_blocks(1500, 17));
    check("five row blocks, a list of 1 edge at first", 1500, five_blocks(1500, 19), 1, true);
    check("five row blocks, a list of 100 edges at first", 1500, five_blocks(1500, 23), 100, true);
    const uint32_t n = 900;
    std::vector<Edge> e;
    for (uint32_t i = 2; i < n; i++) { e.push_back({i, i / 2, i % 9, 8}); e.push_back({i, i - 1, (i * 5) % 9, 8}); }
    e.push_back({1, 0, 3, 8});
    check("one list, a capacity inside a word", n, {list_all(e)}, 70, true);
    check("one list, a capacity of exactly its edges", n, {list_all(e)}, e.size(), false);
    check("one list, a capacity one short", n, {list_all(e)}, e.size() - 1, true);
}

static void case_small()                                                     // (also the ThreadSanitizer build's case)
{
    check("no rows", 0, {});
    check("one row", 1, {});
    check("no edge", 300, {list_launch({{5, 1, 3, 64}, {7, 2, 64, 64}})});
    std::vector<Edge> e;
    for (uint32_t i = 299; i >= 2; i--) e.push_back({i, (i * 7) % (i - 1), i % 5 * 16, 64});
    for (uint32_t i = 2; i < 300; i++)
        if (i / 2 != (i * 7) % (i - 1)) e.push_back({i, i / 2, (i * 3) % 5 * 8, 32});
    check("300 rows, a list", 300, {list_all(e)});
    check("300 rows, a list that is regrown", 300, {list_all(e)}, 50, true);
    Launch F = flat_launch(0, 100);
    for (uint64_t i = 0; i < F.pairs; i += 3) { F.set(i); F.counts[i] = make_uint2((uint32_t)(i % 5) * 16u, 64u); }
    check("100 rows, flat", 100, {F});
    std::vector<uint32_t> later{0, 2, 2};
    check("the better representative is the later one", 3, {list_all({{1, 0, 30, 64}, {2, 1, 31, 64}})}, 0, false, &later);
}

static void fuzz(uint64_t seed, int jobs)
{
    std::mt19937_64 rng(seed);
    for (int j = 0; j < jobs; j++) {
        const uint32_t n = 2 + (uint32_t)(rng() % (j % 5 == 0 ? 20000 : 1500));
        std::vector<Launch> v;
        const int nl = 1 + (int)(rng() % 3);
        const bool flat = rng() % 2;
        const double dens = std::pow(10.0, -(double)(rng() % 4));            // 1 .. 1e-3
        const uint32_t fam = 1 + (uint32_t)(rng() % 40);                     // edges only inside residue classes
        if (flat && n <= 3000) {
            uint32_t r = 0;
            for (int l = 0; l < nl; l++) {
                const uint32_t r2 = l + 1 == nl ? n : std::min<uint32_t>(n, r + 1 + (uint32_t)(rng() % n));
                Launch F = flat_launch(r, r2);
                uint64_t row = std::max<uint64_t>(r, 1), col = 0;
                for (uint64_t i = 0; i < F.pairs; i++) {
                    if (row % fam == col % fam && (double)(rng() % 1000000) < dens * 1e6) {
                        F.set(i);
                        const uint32_t d = rng() % 4 ? 64u : (uint32_t)(rng() % 3) * 32u;
                        F.counts[i] = make_uint2(d ? (uint32_t)(rng() % 5) * (d / 4) : 0u, d);
                    }
                    if (++col == row) { row++; col = 0; }
                }
                v.push_back(F);
                r = r2;
                if (r >= n) break;
            }
        } else {
            std::unordered_set<uint64_t> seen;
            for (int l = 0; l < nl; l++) {
                Launch L = list_launch(random_pairs(rng, n, rng() % 6000, fam));
                mark_distinct(L, rng, dens, seen);
                v.push_back(L);
            }
        }
        const uint64_t cap = rng() % 3 ? 0 : 1 + rng() % 5000;               // every third job starts with a short list
        check(("fuzz " + std::to_string(j)).c_str(), n, v, cap);
    }
}

int main(int argc, char **argv)
{
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "star") case_star();
    else if (c == "between") case_between();
    else if (c == "ties") case_ties();
    else if (c == "zero") case_zero();
    else if (c == "band") case_band();
    else if (c == "lengths") case_lengths();
    else if (c == "padding") case_padding();
    else if (c == "overflow") case_overflow();
    else if (c == "small") case_small();
    else if (c == "fuzz" && argc > 3) fuzz(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
    else { fprintf(stderr, "usage: cluster_nearest_emu small|star|between|ties|zero|band|lengths|padding|overflow | fuzz <seed> <n>\n"); return 2; }
    if (failures) { printf("%d case(s) FAILED\n", failures); return 1; }
    printf("all cases agree\n");
    return 0;
}
