// cluster_density_emu_main.cpp -- runs the kernels of `mash cluster -D`, unchanged, through their launchers on the CPU (tools/hipemu):
// cf_append_kernel (cluster_forest.hip) over ballot words in list mode and in flat triangle mode, then launch_density
// (cluster_density.hip: cd_degree_kernel in both forms, cd_union_kernel, cl_label_kernel, cd_key_kernel, cd_pick_kernel,
// cd_file_kernel, cd_gather_kernel).  The judge is a sequential restatement written here: degrees, the cores united by a plain
// union-find, per border the best of its edges to a core by forest_before with the core as the tie-break, the smallest member per
// cluster.  The driver does what the host does: append per launch, regrow and append again when the list overflows, then one batch.
// TEST INFRASTRUCTURE (tests/test_cluster_density_emu.py); built with g++.  The emulator runs workgroups one after another: what is
// pinned here is the arithmetic (degrees, which end is the core, the keys, the ties, the relabelling, padding, the places in the
// list), not the races between workgroups.
//
//   cluster_density_emu <case>            cases: small bridge ties relabel noise degree lengths padding overflow
//   cluster_density_emu fuzz <seed> <n>   n random jobs
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <cmath>
#include <random>
#include <set>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../mash_amd/csrc/cluster.hip"
#include "../../mash_amd/csrc/cluster_forest.hip"
#include "../../mash_amd/csrc/cluster_density.hip"

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

struct Answer {
    std::vector<uint32_t> label, via, deg;
    uint64_t clusters = 0, cores = 0, borders = 0, noise = 0;
    uint64_t ties = 0, between = 0, first = 0, later = 0;     // borders with a tie for best; with cores of two clusters; first of their cluster; under a later core
};

// the judge
static Answer judge(uint32_t n, const std::vector<Edge> &edges, uint32_t m)
{
    Answer a;
    a.deg.assign(n, 0);
    for (const Edge &e : edges) { a.deg[e.row]++; a.deg[e.col]++; }
    std::vector<uint32_t> up(n);
    for (uint32_t i = 0; i < n; i++) up[i] = i;
    auto find = [&](uint32_t x) { while (up[x] != x) x = up[x] = up[up[x]]; return x; };
    auto core = [&](uint32_t i) { return a.deg[i] >= m; };
    for (const Edge &e : edges) {
        if (!core(e.row) || !core(e.col)) continue;
        const uint32_t x = find(e.row), y = find(e.col);
        if (x != y) up[std::max(x, y)] = std::min(x, y);
    }
    a.via.resize(n);
    for (uint32_t i = 0; i < n; i++) a.via[i] = i;
    std::vector<const Edge *> best(n, nullptr);
    std::vector<uint32_t> n_best(n, 0);
    std::vector<std::set<uint32_t>> beside(n);
    for (const Edge &e : edges) {
        if (core(e.row) == core(e.col)) continue;
        const uint32_t member = core(e.row) ? e.col : e.row, c = core(e.row) ? e.row : e.col;
        beside[member].insert(find(c));
        const Edge *b = best[member];
        if (!b) n_best[member] = 1;
        else if (forest_before(e.numer, e.denom, 0, b->numer, b->denom, 0)) n_best[member] = 1;            // strictly better
        else if (!forest_before(b->numer, b->denom, 0, e.numer, e.denom, 0)) n_best[member]++;             // the same fraction
        if (!b || forest_before(e.numer, e.denom, c, b->numer, b->denom, a.via[member])) {
            best[member] = &e;
            a.via[member] = c;
        }
    }
    std::vector<uint32_t> first(n, 0xFFFFFFFFu);
    a.label.resize(n);
    for (uint32_t i = 0; i < n; i++) first[find(a.via[i])] = std::min(first[find(a.via[i])], i);
    for (uint32_t i = 0; i < n; i++) {
        a.label[i] = first[find(a.via[i])];
        const bool border = !core(i) && a.via[i] != i;
        a.clusters += a.label[i] == i;
        a.cores += core(i);
        a.borders += border;
        a.noise += !core(i) && !border;
        a.ties += border && n_best[i] >= 2;
        a.between += border && beside[i].size() >= 2;
        a.first += border && a.label[i] == i;
        a.later += border && a.via[i] > i;
    }
    return a;
}

struct Filled { bool ok = true; uint64_t used = 0, regrows = 0, cap = 0; std::vector<uint4> list; };

// the appends with the host's regrow.  first_cap: the first capacity of the edge list (0: room for everything)
static Filled fill(uint32_t n, const std::vector<Launch> &launches, uint64_t first_cap, uint64_t total)
{
    Filled o;
    const uint4 guard = make_uint4(GUARD, GUARD, GUARD, GUARD);
    o.cap = first_cap ? first_cap : std::max<uint64_t>(total, 1);
    o.list.assign(o.cap + 1, guard);
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
        for (int attempt = 0;; attempt++) {
            ok = ok && launch_forest_append(a, n, o.list.data(), o.cap, &cursor, &overflow, nullptr) == hipSuccess;
            ok = ok && o.list[o.cap].x == GUARD && o.list[o.cap].y == GUARD;          // never a word behind the list
            ok = ok && cursor == o.used + mine.size() && (overflow != 0) == (cursor > o.cap);
            if (cursor <= o.cap) break;
            if (attempt) { ok = false; break; }
            const uint64_t bigger = std::max<uint64_t>(cursor, 2 * o.cap);            // regrow: the earlier launches' edges move over
            std::vector<uint4> nl(bigger + 1, guard);
            std::copy(o.list.begin(), o.list.begin() + (long)o.used, nl.begin());
            o.list.swap(nl);
            o.cap = bigger;
            cursor = o.used;
            overflow = 0;
            o.regrows++;
        }
        std::vector<Edge> got;
        for (uint64_t i = o.used; i < cursor && i < o.cap; i++) got.push_back({o.list[i].x, o.list[i].y, o.list[i].z, o.list[i].w});
        std::sort(got.begin(), got.end(), by_fields);
        std::sort(mine.begin(), mine.end(), by_fields);
        ok = ok && got.size() == mine.size() && std::equal(got.begin(), got.end(), mine.begin(), same);
        o.used = cursor;
    }
    return o;
}

struct Want { const std::vector<uint32_t> *label = nullptr, *via = nullptr; };

// every m of `ms` over one filled list, the degree pass in both forms; want: the expected arrays where the case knows them in closed
// form, for the first m
static void check(const char *name, uint32_t n, const std::vector<Launch> &launches, const std::vector<uint32_t> &ms, uint64_t first_cap = 0,
                  bool want_regrow = false, Want want = {})
{
    std::vector<Edge> entries, edges;
    for (const Launch &L : launches) entries_of(L, n, entries);
    for (const Edge &e : entries)
        if (e.row > e.col) edges.push_back(e);
    Filled f = fill(n, launches, first_cap, entries.size());
    bool ok = f.ok && (!want_regrow || f.regrows > 0);
    uint64_t bad = 0;
    Answer shown;
    for (size_t k = 0; k < ms.size(); k++) {
        const uint32_t m = ms[k];
        const Answer a = judge(n, edges, m);
        if (k == 0) {
            shown = a;
            ok = ok && (!want.label || *want.label == a.label) && (!want.via || *want.via == a.via);      // the judge itself against the closed form
        }
        for (int plain = 0; plain < 2; plain++) {
            std::vector<uint32_t> deg(n + 1, GUARD), parent(n + 1, GUARD), label(n + 1, GUARD), via(n + 1, GUARD), first(n + 1, GUARD);
            std::vector<unsigned long long> best_key(n + 1, GUARD64), counts(6, GUARD64);
            const DensityBufs b{deg.data(), parent.data(), label.data(), via.data(), first.data(), best_key.data(), counts.data()};
            ok = ok && launch_density(f.list.data(), f.used, b, n, m, plain != 0, nullptr) == hipSuccess;
            ok = ok && deg[n] == GUARD && parent[n] == GUARD && label[n] == GUARD && via[n] == GUARD && first[n] == GUARD && best_key[n] == GUARD64 &&
                 counts[5] == GUARD64 && f.list[f.cap].x == GUARD;                                        // nothing written behind the arrays
            for (uint32_t i = 0; i < n; i++) bad += (label[i] != a.label[i]) + (via[i] != a.via[i]) + (deg[i] != a.deg[i]);
            ok = ok && counts[0] == a.cores && counts[1] == a.borders && counts[2] == a.noise && counts[3] == a.clusters;
        }
    }
    if (!ok || bad) {
        failures++;
        printf("FAIL %s: n %u edges %zu: %llu words differ, regrows %llu%s\n", name, n, edges.size(), (unsigned long long)bad, (unsigned long long)f.regrows,
               ok ? "" : " (launch, guard word, list content, counts or closed form)");
    } else {
        printf("ok   %s: n %u edges %zu m %u clusters %llu cores %llu borders %llu noise %llu regrows %llu, %llu ties for best, %llu between two clusters, "
               "%llu first of their cluster, %llu under a later core\n",
               name, n, edges.size(), ms.empty() ? 0u : ms[0], (unsigned long long)shown.clusters, (unsigned long long)shown.cores,
               (unsigned long long)shown.borders, (unsigned long long)shown.noise, (unsigned long long)f.regrows, (unsigned long long)shown.ties,
               (unsigned long long)shown.between, (unsigned long long)shown.first, (unsigned long long)shown.later);
    }
}

// a clique over rows [r0, r1), every edge numer/64
static void clique(std::vector<Edge> &e, uint32_t r0, uint32_t r1, uint32_t numer)
{
    for (uint32_t i = r0; i < r1; i++)
        for (uint32_t j = r0; j < i; j++) e.push_back({i, j, numer, 64});
}

static void case_bridge()
{
    // cliques over rows 0 .. 5 and 7 .. 12, row 6 between them with one edge to each: at m = 5 a border, never a core
    for (int nearer_later = 1; nearer_later >= 0; nearer_later--) {
        std::vector<Edge> e;
        clique(e, 0, 6, 60);
        clique(e, 7, 13, 60);
        e.push_back({6, 5, nearer_later ? 30u : 31u, 64});
        e.push_back({7, 6, nearer_later ? 31u : 30u, 64});
        std::vector<uint32_t> label(13), via(13);
        for (uint32_t i = 0; i < 13; i++) { via[i] = i; label[i] = i < 6 ? 0 : nearer_later ? 6 : 7; }
        via[6] = nearer_later ? 7 : 5;
        if (!nearer_later) label[6] = 0;
        check(nearer_later ? "a bridge row nearer the later clique" : "a bridge row nearer the earlier clique", 13, {list_all(e)}, {5, 1, 2, 3, 6, 7}, 0, false,
              {&label, &via});
        std::reverse(e.begin(), e.end());
        check("the same, list backwards", 13, {list_all(e)}, {5}, 0, false, {&label, &via});
        Launch F = flat_launch(0, 13);
        for (const Edge &x : e) flat_set(F, x);
        check("the same, flat", 13, {F}, {5}, 0, false, {&label, &via});
    }
    // a thin run of three bridge rows between two cliques of 40: single linkage (m = 1) chains, m = 3 .. 39 does not
    std::vector<Edge> e;
    clique(e, 0, 40, 50);
    clique(e, 43, 83, 50);
    for (uint32_t i = 40; i <= 43; i++) e.push_back({i, i - 1, 40, 64});
    check("a run of bridge rows, m = 3", 83, {list_all(e)}, {3, 1, 2, 39, 40, 41});
}

static void case_ties()
{
    // cliques 0 .. 3 and 5 .. 8 (m = 3), row 4 between rows 3 and 5
    auto with = [](Edge a, Edge b) { std::vector<Edge> e; clique(e, 0, 4, 60); clique(e, 5, 9, 60); e.push_back(a); e.push_back(b); return e; };
    std::vector<uint32_t> smaller{0, 1, 2, 3, 3, 5, 6, 7, 8}, larger{0, 1, 2, 3, 5, 5, 6, 7, 8};
    check("32/64 beside 16/32", 9, {list_all(with({4, 3, 32, 64}, {5, 4, 16, 32}))}, {3}, 0, false, {nullptr, &smaller});
    check("16/32 beside 32/64", 9, {list_all(with({4, 3, 16, 32}, {5, 4, 32, 64}))}, {3}, 0, false, {nullptr, &smaller});
    check("0/64 beside 0/0", 9, {list_all(with({4, 3, 0, 64}, {5, 4, 0, 0}))}, {3}, 0, false, {nullptr, &smaller});
    check("0/0 beside 0/64", 9, {list_all(with({4, 3, 0, 0}, {5, 4, 0, 64}))}, {3}, 0, false, {nullptr, &smaller});
    check("31/64 beside 16/32", 9, {list_all(with({4, 3, 31, 64}, {5, 4, 16, 32}))}, {3}, 0, false, {nullptr, &larger});
    check("0/64 beside 1/2000000", 9, {list_all(with({4, 3, 0, 64}, {5, 4, 1, 2000000}))}, {3}, 0, false, {nullptr, &larger});
    check("2097149/2097150 beside 2097150/2097151", 9, {list_all(with({4, 3, 2097149, 2097150}, {5, 4, 2097150, 2097151}))}, {3}, 0, false, {nullptr, &larger});
    check("a numer == 0 edge is the border's only edge to a core", 9, {list_all(with({4, 3, 0, 64}, {4, 4, 0, 64}))}, {3}, 0, false, {nullptr, &smaller});
}

static void case_relabel()
{
    // rows 0 and 1 are borders of the clique 2 .. 7 (m = 5): the cluster's label is a border's row; row 8 is a border of the clique
    // 9 .. 14 from below, row 15 one from above
    std::vector<Edge> e;
    clique(e, 2, 8, 60);
    clique(e, 9, 15, 60);
    e.push_back({2, 0, 10, 64});
    e.push_back({7, 1, 10, 64});
    e.push_back({9, 8, 10, 64});
    e.push_back({15, 14, 10, 64});
    std::vector<uint32_t> label{0, 0, 0, 0, 0, 0, 0, 0, 8, 8, 8, 8, 8, 8, 8, 8}, via{2, 7, 2, 3, 4, 5, 6, 7, 9, 9, 10, 11, 12, 13, 14, 14};
    check("borders below every core of their cluster", 16, {list_all(e)}, {5, 6}, 0, false, {&label, &via});
}

static void case_noise()
{
    // clique 0 .. 4 (m = 4); row 5 beside rows 6 and 7 only, which are no cores: noise, as they are; row 8 without an edge
    std::vector<Edge> e;
    clique(e, 0, 5, 60);
    e.push_back({6, 5, 64, 64});
    e.push_back({7, 5, 64, 64});
    e.push_back({7, 6, 64, 64});
    std::vector<uint32_t> own{0, 0, 0, 0, 0, 5, 6, 7, 8}, id{0, 1, 2, 3, 4, 5, 6, 7, 8};
    check("edges among rows that are no cores", 9, {list_all(e)}, {4, 3, 2}, 0, false, {&own, &id});
    // two rows that are no cores, joined to each other (64/64) and to cores of different clusters (10/64): the clusters stay apart
    std::vector<Edge> f;
    clique(f, 0, 5, 60);
    clique(f, 7, 12, 60);
    f.push_back({5, 4, 10, 64});
    f.push_back({7, 6, 10, 64});
    f.push_back({6, 5, 64, 64});
    std::vector<uint32_t> label{0, 0, 0, 0, 0, 0, 6, 6, 6, 6, 6, 6}, via{0, 1, 2, 3, 4, 4, 7, 7, 8, 9, 10, 11};
    check("two borders joined to each other", 12, {list_all(f)}, {4, 3}, 0, false, {&label, &via});
}

static void case_degree()
{
    // a star of 100 rays around row 50: deg(50) = 100, every other row 1.  m = 100: the centre is the only core, every ray a border;
    // m = 101: nothing is a core.  Then degrees of exactly m and m - 1 side by side: row i of a chain-with-chords has min(i, 7) + ... edges
    std::vector<Edge> e;
    for (uint32_t i = 0; i <= 100; i++)
        if (i != 50) e.push_back({std::max(i, 50u), std::min(i, 50u), i % 5 * 16, 64});
    std::vector<uint32_t> label(101, 0), via(101, 50);
    check("a star, the degree exactly m", 101, {list_all(e)}, {100, 101, 99, 1, 2}, 0, false, {&label, &via});
    // runs of equal rows in every position of a wave: row i has an edge to each of the i % 9 rows below it
    std::vector<Edge> g;
    for (uint32_t i = 1; i < 700; i++)
        for (uint32_t k = 1; k <= i % 9 && k <= i; k++) g.push_back({i, i - k, (i + k) % 5 * 16, 64});
    check("runs of every length, in input order", 700, {list_all(g)}, {1, 2, 5, 8, 9, 12, 16, 17});
    std::mt19937_64 rng(7);
    std::shuffle(g.begin(), g.end(), rng);
    check("the same edges, shuffled", 700, {list_all(g)}, {5, 8, 9});
    Launch F = flat_launch(0, 700);
    for (const Edge &x : g) flat_set(F, x);
    check("the same edges, flat", 700, {F}, {5, 8, 9});
}

static std::vector<Edge> random_pairs(std::mt19937_64 &rng, uint32_t n, uint64_t K, uint32_t fam)
{
    std::vector<Edge> q;
    for (uint64_t i = 0; i < K; i++) {
        const uint32_t a = 1 + (uint32_t)(rng() % (n - 1));
        uint32_t b = (uint32_t)(rng() % a);
        if (rng() % 8) b -= std::min(b, (b % fam + fam - a % fam) % fam);            // mostly inside a family, some bridges between them
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
        Launch Q = list_launch(random_pairs(rng, 300, K, 3));
        std::unordered_set<uint64_t> seen;
        mark_distinct(Q, rng, 0.8, seen);
        check(("list of " + std::to_string(K) + " pairs").c_str(), 300, {Q}, {2, 1, 5});
    }
}

static void case_padding()
{
    // marked pairs with an end outside the table become {0, 0, 0, 0}: hi == lo, skipped by every pass -- also where row 0 is a core,
    // a border or noise
    std::vector<Edge> e{{1, 0, 30, 64}, {2, 1, 31, 64}, {2, 0, 31, 64}, {7, 1, 64, 64}, {3, 9, 64, 64}, {4, 3, 5, 64}, {5, 5, 64, 64}, {3, 2, 9, 64}};
    Launch L = list_launch(e);
    for (uint64_t i = 0; i < L.pairs; i++)
        if (e[i].row != e[i].col) L.set(i);
    std::vector<uint32_t> label{0, 0, 0, 0, 4}, via{2, 2, 2, 2, 4};                 // degrees 2 2 3 2 1 -> m = 3: row 2 the only core
    check("pairs outside a table of 5 rows", 5, {L}, {3, 2, 1}, 0, false, {&label, &via});
    std::mt19937_64 rng(31);
    std::vector<Edge> q = random_pairs(rng, 1200, 5000, 4);                          // rows up to 1199 over a table of 800
    Launch Q = list_launch(q);
    std::unordered_set<uint64_t> seen;
    mark_distinct(Q, rng, 0.7, seen);
    check("a third of the pairs outside a table of 800 rows", 800, {Q}, {4, 1, 8});
    check("the same, a list of 1 edge at first", 800, {Q}, {4}, 1, true);
}

static std::vector<Launch> five_blocks(uint32_t n, uint64_t seed)
{
    std::mt19937_64 rng(seed);
    std::vector<Launch> v;
    for (auto rb : {std::make_pair(0u, 1u), std::make_pair(1u, 700u), std::make_pair(700u, 701u), std::make_pair(701u, n - 1), std::make_pair(n - 1, n)}) {
        Launch F = flat_launch(rb.first, rb.second);
        for (uint32_t r = std::max(rb.first, 1u); r < rb.second; r++)
            for (int k = 0; k < 6; k++) {
                const uint32_t c = (uint32_t)(rng() % r);
                if ((r % 7) == (c % 7) || rng() % 16 == 0) flat_set(F, {r, c, (uint32_t)(rng() % 5) * 16u, 64u});
            }
        if (rb.second == n) { flat_set(F, {n - 1, 3, 16, 64}); flat_set(F, {n - 1, 4, 32, 64}); flat_set(F, {n - 1, n - 2, 32, 64}); }
        v.push_back(F);
    }
    return v;
}

static void case_overflow()
{
    check("five row blocks, one list", 1500, five_blocks(1500, 17), {3, 2, 1});
    check("five row blocks, a list of 1 edge at first", 1500, five_blocks(1500, 19), {3}, 1, true);
    check("five row blocks, a list of 100 edges at first", 1500, five_blocks(1500, 23), {2}, 100, true);
    const uint32_t n = 900;
    std::vector<Edge> e;
    for (uint32_t i = 2; i < n; i++) { e.push_back({i, i / 2, i % 9, 8}); e.push_back({i, i - 1, (i * 5) % 9, 8}); }
    e.push_back({1, 0, 3, 8});
    check("one list, a capacity inside a word", n, {list_all(e)}, {3}, 70, true);
    check("one list, a capacity of exactly its edges", n, {list_all(e)}, {3}, e.size(), false);
    check("one list, a capacity one short", n, {list_all(e)}, {3}, e.size() - 1, true);
}

static void case_small()                                                     // (also the ThreadSanitizer build's case)
{
    check("no rows", 0, {}, {1, 3});
    check("one row", 1, {}, {1, 3});
    check("no edge", 300, {list_launch({{5, 1, 3, 64}, {7, 2, 64, 64}})}, {1, 2});
    std::vector<Edge> e;
    for (uint32_t i = 299; i >= 2; i--) e.push_back({i, (i * 7) % (i - 1), i % 5 * 16, 64});
    for (uint32_t i = 2; i < 300; i++)
        if (i / 2 != (i * 7) % (i - 1)) e.push_back({i, i / 2, (i * 3) % 5 * 8, 32});
    check("300 rows, a list", 300, {list_all(e)}, {3, 1, 2, 4, 1000});
    check("300 rows, a list that is regrown", 300, {list_all(e)}, {3}, 50, true);
    Launch F = flat_launch(0, 100);
    for (uint64_t i = 0; i < F.pairs; i += 3) { F.set(i); F.counts[i] = make_uint2((uint32_t)(i % 5) * 16u, 64u); }
    check("100 rows, flat", 100, {F}, {34, 33, 1});
    std::vector<Edge> b;
    clique(b, 0, 6, 60);
    clique(b, 7, 13, 60);
    b.push_back({6, 5, 30, 64});
    b.push_back({7, 6, 31, 64});
    check("a bridge row nearer the later clique", 13, {list_all(b)}, {5});
}

static void fuzz(uint64_t seed, int jobs)
{
    std::mt19937_64 rng(seed);
    for (int j = 0; j < jobs; j++) {
        const uint32_t n = 2 + (uint32_t)(rng() % (j % 5 == 0 ? 20000 : 1500));
        std::vector<Launch> v;
        const int nl = 1 + (int)(rng() % 3);
        const bool flat = rng() % 2;
        const double dens = 1.0 / (double)(1 + rng() % 3 * 2);              // 1, 1/3, 1/5
        const uint32_t fam = 1 + (uint32_t)(rng() % 40);                     // edges mostly inside residue classes
        if (flat && n <= 3000) {
            uint32_t r = 0;
            for (int l = 0; l < nl; l++) {
                const uint32_t r2 = l + 1 == nl ? n : std::min<uint32_t>(n, r + 1 + (uint32_t)(rng() % n));
                Launch F = flat_launch(r, r2);
                uint64_t row = std::max<uint64_t>(r, 1), col = 0;
                for (uint64_t i = 0; i < F.pairs; i++) {
                    if ((row % fam == col % fam || rng() % 64 == 0) && (double)(rng() % 1000000) < dens * 1e6 * 0.05) {
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
                Launch L = list_launch(random_pairs(rng, n, std::min<uint64_t>(12000, n / 2 + rng() % (3 * (uint64_t)n + 1)), fam));
                mark_distinct(L, rng, dens, seen);
                v.push_back(L);
            }
        }
        const uint64_t cap = rng() % 3 ? 0 : 1 + rng() % 5000;               // every third job starts with a short list
        uint64_t marked = 0;
        for (const Launch &L : v)
            for (unsigned long long w : L.masks) marked += (uint64_t)__builtin_popcountll(w);
        const uint32_t m = 1 + (uint32_t)(rng() % (2 + 2 * marked / n));      // 1 .. the mean degree + 2
        check(("fuzz " + std::to_string(j)).c_str(), n, v, {m, m + 1}, cap);
    }
}

int main(int argc, char **argv)
{
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "bridge") case_bridge();
    else if (c == "ties") case_ties();
    else if (c == "relabel") case_relabel();
    else if (c == "noise") case_noise();
    else if (c == "degree") case_degree();
    else if (c == "lengths") case_lengths();
    else if (c == "padding") case_padding();
    else if (c == "overflow") case_overflow();
    else if (c == "small") case_small();
    else if (c == "fuzz" && argc > 3) fuzz(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
    else { fprintf(stderr, "usage: cluster_density_emu small|bridge|ties|relabel|noise|degree|lengths|padding|overflow | fuzz <seed> <n>\n"); return 2; }
    if (failures) { printf("%d case(s) FAILED\n", failures); return 1; }
    printf("all cases agree\n");
    return 0;
}
