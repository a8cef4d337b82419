// forest_emu_main.cpp -- runs mash_amd/csrc/cluster_forest.hip, unchanged, through its launchers (cf_append_kernel over ballot words
// in list mode and in flat triangle mode; the rounds cf_key_kernel / cf_rc_kernel / cf_pick_kernel / cf_flatten_kernel, the labels,
// the padding, the bitonic sort and the denominator flags, all queued by launch_forest_rounds) on the CPU (tools/hipemu) and compares
// the forest, its order, the labels and the counts with Kruskal over the same edges under a comparator written here (128-bit cross-
// multiplication).  The driver below does what cluster_forest_tri does on the host: append per launch, regrow and append again when the
// list overflows, one batch behind the last append.
// TEST INFRASTRUCTURE (tests/test_forest_emu.py); built with g++.  The emulator runs workgroups one after another: what is pinned here
// is the arithmetic (word / bit / pair indices, the places in the lists, the keys, the rounds, the network), not the races between
// workgroups.
//
//   forest_emu <case>            cases: small path clique star parts denoms density blocks overflow
//   forest_emu fuzz <seed> <n>   n random jobs
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <cmath>
#include <random>
#include <string>
#include <vector>

#include "../../mash_amd/csrc/cluster.hip"
#include "../../mash_amd/csrc/cluster_forest.hip"

using namespace mg;

struct Edge { uint32_t row, col, numer, denom; };
static bool same(const Edge &a, const Edge &b) { return a.row == b.row && a.col == b.col && a.numer == b.numer && a.denom == b.denom; }
static bool by_fields(const Edge &a, const Edge &b)
{
    return a.row != b.row ? a.row < b.row : a.col != b.col ? a.col < b.col : a.numer != b.numer ? a.numer < b.numer : a.denom < b.denom;
}

// the definition: larger fraction first, equal fractions by row, then column
static bool ranks_before(const Edge &a, const Edge &b)
{
    const unsigned __int128 l = (unsigned __int128)a.numer * (b.denom ? b.denom : 1u), r = (unsigned __int128)b.numer * (a.denom ? a.denom : 1u);
    return l != r ? l > r : a.row != b.row ? a.row < b.row : a.col < b.col;
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

// the edges a launch stands for, by the definition of the layouts (not by pair_rc), as {larger, smaller}
static void edges_of(const Launch &L, std::vector<Edge> &out)
{
    if (!L.rc.empty()) {
        for (uint64_t i = 0; i < L.pairs; i++)
            if (L.get(i)) out.push_back({std::max(L.rc[i].x, L.rc[i].y), std::min(L.rc[i].x, L.rc[i].y), L.counts[i].x, L.counts[i].y});
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

// first_cap: the first capacity of the edge list (0: room for everything); s: the sketch size of the denominator flags
static void check(const char *name, uint32_t n, const std::vector<Launch> &launches, uint64_t first_cap = 0, bool want_regrow = false, uint32_t s = 64)
{
    // the definition: Kruskal over the edges in their order
    std::vector<Edge> edges;
    for (const Launch &L : launches) edges_of(L, edges);
    std::vector<Edge> sorted = edges, want;
    std::sort(sorted.begin(), sorted.end(), ranks_before);
    std::vector<uint32_t> up(n);
    for (uint32_t i = 0; i < n; i++) up[i] = i;
    auto find = [&](uint32_t x) { while (up[x] != x) { up[x] = up[up[x]]; x = up[x]; } return x; };
    for (const Edge &e : sorted) {
        const uint32_t a = find(e.row), b = find(e.col);
        if (a == b) continue;
        up[std::max(a, b)] = std::min(a, b);
        want.push_back(e);
    }
    uint64_t want_roots = 0;
    for (uint32_t i = 0; i < n; i++) want_roots += find(i) == i;

    bool ok = true;
    uint64_t cap = first_cap ? first_cap : std::max<uint64_t>(edges.size(), 1), used = 0, regrows = 0;
    std::vector<uint4> list(cap + 1, make_uint4(GUARD, GUARD, GUARD, GUARD));
    unsigned long long cursor = 0;
    uint32_t overflow = 0;
    for (const Launch &L : launches) {
        FinishArgs a{};
        a.pairs = L.pairs;
        a.first_row = L.first_row;
        a.triangle = 1;
        a.counts = L.counts.data();
        a.masks = const_cast<unsigned long long *>(L.masks.data());
        a.list_rc = L.rc.empty() ? nullptr : L.rc.data();
        std::vector<Edge> mine;
        edges_of(L, mine);
        for (int attempt = 0;; attempt++) {
            ok = ok && launch_forest_append(a, n, list.data(), cap, &cursor, &overflow, nullptr) == hipSuccess;
            ok = ok && list[cap].x == GUARD && list[cap].w == GUARD;                // never a word behind the list
            ok = ok && cursor == used + mine.size() && (overflow != 0) == (cursor > cap);
            if (cursor <= cap) break;
            if (attempt) { ok = false; break; }
            const uint64_t bigger = std::max<uint64_t>(cursor, 2 * cap);          // regrow: the earlier launches' edges move over
            std::vector<uint4> nl(bigger + 1, make_uint4(GUARD, GUARD, GUARD, GUARD));
            std::copy(list.begin(), list.begin() + (long)used, nl.begin());
            list.swap(nl);
            cap = bigger;
            cursor = used;
            overflow = 0;
            regrows++;
        }
        // what this launch appended is its edges with their counts, in some order
        std::vector<Edge> got;
        for (uint64_t i = used; i < cursor && i < cap; i++) got.push_back({list[i].x, list[i].y, list[i].z, list[i].w});
        std::sort(got.begin(), got.end(), by_fields);
        std::sort(mine.begin(), mine.end(), by_fields);
        ok = ok && got.size() == mine.size() && std::equal(got.begin(), got.end(), mine.begin(), same);
        used = cursor;
    }

    const uint32_t rq = forest_rounds(n);
    const uint64_t room = forest_room(n);
    uint32_t lg = 0;
    while ((n >> lg) > 1) lg++;
    ok = ok && rq == lg + 2 && room >= std::max<uint64_t>(n, 2) && (room & (room - 1)) == 0 && (room == 2 || room / 2 < n);
    std::vector<uint32_t> parent(n + 1, GUARD), comp(n + 1, GUARD), merged(rq + 1, GUARD), label(n + 1, GUARD), seen(s + 2, GUARD);
    std::vector<unsigned long long> best_key(n + 1, GUARD64), best_rc(n + 1, GUARD64), live(rq + 1, GUARD64);
    std::vector<uint4> forest(room + 1, make_uint4(GUARD, GUARD, GUARD, GUARD));
    unsigned long long count = GUARD64, roots = GUARD64;
    const ForestBufs fb{parent.data(), comp.data(), best_key.data(), best_rc.data(), forest.data(), &count, merged.data(), live.data()};
    ok = ok && launch_forest_rounds(list.data(), used, fb, n, label.data(), &roots, seen.data(), s, nullptr) == hipSuccess;
    // nothing written behind the arrays
    ok = ok && parent[n] == GUARD && comp[n] == GUARD && merged[rq] == GUARD && label[n] == GUARD && seen[s + 1] == GUARD && best_key[n] == GUARD64 &&
         best_rc[n] == GUARD64 && live[rq] == GUARD64 && forest[room].x == GUARD && forest[room].w == GUARD && list[cap].x == GUARD;
    // the rounds: the first that chose nothing is the fixpoint, at most floor(log2 n) + 1 rounds reach it, what is queued behind it
    // chooses nothing and leaves the rounds' arrays as the fixpoint's flatten left them
    uint32_t r = 0;
    uint64_t chosen = 0;
    while (r < rq && merged[r]) chosen += merged[r++];
    const uint64_t rounds = used ? r + 1 : 0;
    if (used) ok = ok && r < rq && rounds <= lg + 1;
    for (uint32_t k = r; k < rq; k++) ok = ok && merged[k] == 0 && live[k] == 0;
    // a round begins with the edges that no earlier round's choices have closed: round 0 with every edge, and no round with fewer
    // live edges than it chooses
    if (used) ok = ok && live[0] == edges.size();
    for (uint32_t k = 0; k < r; k++) ok = ok && live[k] >= merged[k] && (k == 0 || live[k] < live[k - 1]);
    ok = ok && chosen == count;
    uint64_t bad = 0;
    for (uint32_t i = 0; i < n; i++) {
        bad += label[i] != find(i);
        ok = ok && comp[i] == label[i] && best_key[i] == 0 && best_rc[i] == ~0ull;
    }
    ok = ok && roots == want_roots && count == want.size() && count + roots == n;
    for (uint64_t i = 0; i < want.size() && i < count; i++) bad += !same(want[i], Edge{forest[i].x, forest[i].y, forest[i].z, forest[i].w});
    if (used && n > 1)
        for (uint64_t i = count; i < room; i++) ok = ok && forest[i].x == 0xFFFFFFFFu && forest[i].y == 0xFFFFFFFFu && forest[i].z == 0 && forest[i].w == 1;
    std::vector<uint32_t> want_seen(s + 1, 0);
    for (const Edge &e : want)
        if (e.denom <= s) want_seen[e.denom] = 1;
    for (uint32_t d = 0; d <= s; d++) ok = ok && seen[d] == want_seen[d];
    const bool shaped = !want_regrow || regrows > 0;
    if (!ok || bad || !shaped) {
        failures++;
        printf("FAIL %s: n %u edges %zu: %llu records or labels differ, forest %llu want %zu, clusters %llu want %llu, rounds %llu (<= %u), regrows %llu%s\n",
               name, n, edges.size(), (unsigned long long)bad, count, want.size(), roots, (unsigned long long)want_roots, (unsigned long long)rounds, lg + 1,
               (unsigned long long)regrows, ok ? "" : " (launch, guard word, list content, rounds or flags)");
    } else {
        printf("ok   %s: n %u edges %zu forest %zu clusters %llu rounds %llu of %u regrows %llu\n", name, n, edges.size(), want.size(),
               (unsigned long long)want_roots, (unsigned long long)rounds, rq, (unsigned long long)regrows);
    }
}

// weights with heavy ties: a handful of fractions under three denominators
static void weigh(std::vector<Edge> &e, uint64_t seed, uint32_t values = 9)
{
    std::mt19937_64 rng(seed);
    const uint32_t dens[3] = {16, 32, 64};
    for (Edge &x : e) {
        x.denom = dens[rng() % 3];
        x.numer = (uint32_t)(1 + rng() % std::min(values, 16u)) * (x.denom / 16);
    }
}

static Launch flat_of(uint32_t n, const std::vector<Edge> &e)
{
    Launch F = flat_launch(0, n);
    for (const Edge &x : e) flat_set(F, x);
    return F;
}

static void case_small()                                                     // (also the ThreadSanitizer build's case)
{
    check("no rows", 0, {});
    check("one row", 1, {});
    check("two rows, one edge", 2, {list_all({{1, 0, 3, 4}})});
    check("no edge", 300, {list_launch({{5, 1, 1, 2}, {7, 2, 1, 2}})});
    std::vector<Edge> e;
    for (uint32_t i = 299; i >= 1; i--) e.push_back({i, (i * 7) % i, 0, 0});
    for (uint32_t i = 2; i < 300; i++)
        if (i / 2 != (i * 7) % i) e.push_back({i, i / 2, 0, 0});
    weigh(e, 1);
    check("300 rows, a list", 300, {list_all(e)});
    check("300 rows, a list that is regrown", 300, {list_all(e)}, 50, true);
    std::vector<Edge> f;
    for (uint32_t r = 1; r < 100; r++)
        for (uint32_t c = r % 3; c < r; c += 3) f.push_back({r, c, 0, 0});
    weigh(f, 2);
    check("100 rows, flat", 100, {flat_of(100, f)});
}

static void case_path()
{
    const uint32_t n = 3000;
    std::vector<Edge> e;
    for (uint32_t i = 1; i < n; i++) e.push_back({i, i - 1, 0, 0});
    weigh(e, 3);
    check("path in index order, list", n, {list_all(e)});                        // (the greedy rounds need n / 2 here: these need 13 at most)
    check("path in index order, flat", n, {flat_of(n, e)});
    for (Edge &x : e) { x.numer = 32; x.denom = 64; }
    check("path in index order, one weight", n, {list_all(e)});
    std::vector<uint32_t> perm(n);
    for (uint32_t i = 0; i < n; i++) perm[i] = i;
    std::mt19937_64 rng(3);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<Edge> s;
    for (uint32_t i = 1; i < n; i++) s.push_back({std::max(perm[i], perm[i - 1]), std::min(perm[i], perm[i - 1]), 0, 0});
    weigh(s, 4);
    std::shuffle(s.begin(), s.end(), rng);
    check("path over shuffled rows, list", n, {list_all(s)});
}

static void case_clique()
{
    const uint32_t n = 300;                                                     // 44 850 pairs: not a multiple of 64
    std::vector<Edge> e;
    for (uint32_t r = 1; r < n; r++)
        for (uint32_t c = 0; c < r; c++) e.push_back({r, c, 48, 64});
    // every fraction equal: the order is {row, col} alone, Kruskal keeps (r, 0) for every r -- the star around row 0
    check("clique, all fractions equal: the star around row 0", n, {flat_of(n, e)});
    for (Edge &x : e)
        if (x.col == 7 || x.row == 7) { x.numer = 25; x.denom = 32; }           // 25/32 > 48/64: now the star around row 7
    check("clique, the edges of row 7 better: the star around row 7", n, {list_all(e)});
}

static void case_star()
{
    const uint32_t n = 3000, c = 1234;
    std::vector<Edge> e;
    for (uint32_t i = n; i-- > 0;)
        if (i != c) e.push_back({std::max(i, c), std::min(i, c), 0, 0});
    weigh(e, 5, 3);
    check("star around 1234, list", n, {list_all(e)});                          // every live edge names one component from round 2 on
    check("star around 1234, flat", n, {flat_of(n, e)});
}

static void case_parts()
{
    const uint32_t n = 2000;
    std::mt19937_64 rng(6);
    std::vector<Edge> e;
    std::vector<unsigned char> have((size_t)n * n, 0);
    for (int k = 0; k < 30000; k++) {                                           // 13 residue classes, a few rows with no edge at all
        const uint32_t a = 1 + (uint32_t)(rng() % (n - 1));
        uint32_t b = (uint32_t)(rng() % a);
        b -= std::min(b, (b % 13 + 13 - a % 13) % 13);
        if (a % 13 != b % 13 || a % 97 == 0 || b % 97 == 0 || have[(size_t)a * n + b]++) continue;
        e.push_back({a, b, 0, 0});
    }
    weigh(e, 7);
    check("a disconnected graph, list", n, {list_all(e)});
    check("a disconnected graph, flat", n, {flat_of(n, e)});
}

static void case_denoms()
{
    // equal fractions under three denominators: 1/2 = 2/4 = 32/64 rank by {row, col}, whatever the denominator
    std::vector<Edge> e = {{3, 0, 1, 2}, {2, 1, 2, 4}, {3, 1, 32, 64}, {2, 0, 32, 64}, {1, 0, 2, 4}, {3, 2, 1, 2}, {4, 0, 31, 64}, {4, 3, 33, 64}, {5, 4, 0, 0}};
    check("1/2, 2/4 and 32/64", 6, {list_all(e)});
    const uint32_t n = 500;
    std::mt19937_64 rng(8);
    std::vector<Edge> g;
    for (uint32_t r = 1; r < n; r++)
        for (int k = 0; k < 6; k++) {
            const uint32_t c = (uint32_t)(rng() % r), d = 1u << (1 + rng() % 6);
            bool dup = false;
            for (const Edge &x : g) dup = dup || (x.row == r && x.col == c);
            if (!dup) g.push_back({r, c, d / 2 + (rng() % 3 == 0 ? d / 4 : 0), d});
        }
    check("halves and three quarters under six denominators", n, {list_all(g)});
    // denominators at the key's limit: neighbours that a 32-bit or a float key would merge
    const uint32_t top = FOREST_DENOM_LIMIT - 1;
    std::vector<Edge> t = {{1, 0, top - 2, top - 1}, {2, 0, top - 1, top}, {2, 1, top - 3, top - 2}, {3, 0, 1, top}, {3, 1, 1, top - 1}, {3, 2, 2, top}};
    check("denominators of 2^21 - 1", 4, {list_all(t)}, 0, false, top);
}

static void case_density()
{
    const uint32_t n = 4000;
    std::mt19937_64 rng(11);
    std::vector<Edge> e;
    std::vector<unsigned char> have((size_t)n * n, 0);
    while (e.size() < 65 * 5 * 64) {
        const uint32_t a = 1 + (uint32_t)(rng() % (n - 1)), b = (uint32_t)(rng() % a);
        if (!have[(size_t)a * n + b]++) e.push_back({a, b, 0, 0});
    }
    weigh(e, 12);
    Launch L = list_launch(e);
    for (uint32_t w = 0; w < 65 * 5; w++) {                                      // word w carries w % 65 bits, 0 .. 64
        std::vector<int> bits(64);
        for (int b = 0; b < 64; b++) bits[b] = b;
        std::shuffle(bits.begin(), bits.end(), rng);
        for (uint32_t k = 0; k < w % 65; k++) L.set((uint64_t)w * 64 + bits[k]);
    }
    check("mask words of every density, list", n, {L});
    Launch F = flat_launch(0, 700);                                              // 244 650 pairs
    for (uint64_t w = 0; w < F.masks.size(); w++) {
        const uint64_t left = F.pairs - w * 64;
        unsigned long long m = 0;
        for (uint32_t k = 0; k < (w * 7) % 65; k++) m |= 1ull << (rng() % 64);
        if (w % 3) m = w % 5 ? 0 : m & rng() & rng() & rng();
        F.masks[w] = left >= 64 ? m : m & ((1ull << left) - 1);
    }
    for (uint64_t i = 0; i < F.pairs; i++) F.counts[i] = make_uint2((uint32_t)(1 + rng() % 8) * 8, 64u);
    check("mask words of every density, flat", 700, {F});
    for (uint32_t K : {1u, 37u, 63u, 64u, 65u, 4097u}) {                         // lists whose length is not a multiple of 64
        std::vector<Edge> q;
        std::vector<unsigned char> hq(900 * 900, 0);
        while (q.size() < K) {
            const uint32_t a = 1 + (uint32_t)(rng() % 899), b = (uint32_t)(rng() % a);
            if (!hq[a * 900 + b]++) q.push_back({a, b, 0, 0});
        }
        weigh(q, K);
        Launch Q = list_launch(q);
        for (uint32_t i = 0; i < K; i++)
            if (rng() % 100 < 40 || i + 1 == K) Q.set(i);
        check(("list of " + std::to_string(K) + " pairs").c_str(), 900, {Q});
    }
}

static std::vector<Launch> five_blocks(uint32_t n, uint64_t seed)
{
    // row blocks of one triangle over one list; seven families by residue, chains inside them
    std::mt19937_64 rng(seed);
    std::vector<Launch> v;
    for (auto rb : {std::make_pair(0u, 1u), std::make_pair(1u, 700u), std::make_pair(700u, 701u), std::make_pair(701u, n - 1), std::make_pair(n - 1, n)}) {
        Launch F = flat_launch(rb.first, rb.second);
        for (uint32_t r = std::max(rb.first, 1u); r < rb.second; r++)
            for (int k = 0; k < 3; k++) {
                const uint32_t c = (uint32_t)(rng() % r);
                if ((r % 7) == (c % 7)) flat_set(F, {r, c, (uint32_t)(1 + rng() % 6) * 8, 64u});
            }
        if (rb.second == n) { flat_set(F, {n - 1, 3, 40, 64}); flat_set(F, {n - 1, 4, 20, 32}); flat_set(F, {n - 1, n - 2, 5, 8}); }
        v.push_back(F);
    }
    return v;
}

static void case_blocks() { check("five row blocks, one list", 1500, five_blocks(1500, 17)); }

static void case_overflow()
{
    check("five row blocks, a list of 1 edge at first", 1500, five_blocks(1500, 19), 1, true);
    check("five row blocks, a list of 100 edges at first", 1500, five_blocks(1500, 23), 100, true);
    const uint32_t n = 900;
    std::vector<Edge> e;
    for (uint32_t i = 1; i < n; i++) {
        e.push_back({i, i / 2, 0, 0});
        if (i / 2 != i - 1) e.push_back({i, i - 1, 0, 0});
    }
    weigh(e, 29);
    check("one list, a capacity inside a word", n, {list_all(e)}, 70, true);
    check("one list, a capacity of exactly its edges", n, {list_all(e)}, e.size(), false);
    check("one list, a capacity one short", n, {list_all(e)}, e.size() - 1, true);
}

static void fuzz(uint64_t seed, int jobs)
{
    std::mt19937_64 rng(seed);
    for (int j = 0; j < jobs; j++) {
        const uint32_t n = 2 + (uint32_t)(rng() % (j % 5 == 0 ? 6000 : 1200));
        std::vector<Launch> v;
        const int nl = 1 + (int)(rng() % 3);
        const bool flat = rng() % 2;
        const double dens = std::pow(10.0, -(double)(rng() % 4));           // 1 .. 1e-3
        const uint32_t fam = 1 + (uint32_t)(rng() % 20);                     // edges only inside residue classes
        const uint32_t values = 1 + (uint32_t)(rng() % 16);
        auto weight = [&](uint32_t &numer, uint32_t &denom) {
            denom = 16u << (rng() % 3);
            numer = (uint32_t)(1 + rng() % values) * (denom / 16);
        };
        if (flat && n <= 2000) {
            uint32_t r = 0;
            for (int l = 0; l < nl; l++) {
                const uint32_t r2 = l + 1 == nl ? n : std::min<uint32_t>(n, r + 1 + (uint32_t)(rng() % n));
                Launch F = flat_launch(r, r2);
                uint64_t row = std::max<uint64_t>(r, 1), col = 0;
                for (uint64_t i = 0; i < F.pairs; i++) {
                    if (row % fam == col % fam && (double)(rng() % 1000000) < dens * 1e6) {
                        F.set(i);
                        weight(F.counts[i].x, F.counts[i].y);
                    }
                    if (++col == row) { row++; col = 0; }
                }
                v.push_back(F);
                r = r2;
                if (r >= n) break;
            }
        } else {
            std::vector<unsigned char> have((size_t)n * n, 0);               // a pair is marked once over all lists
            for (int l = 0; l < nl; l++) {
                const uint64_t K = rng() % 30000;
                std::vector<Edge> e;
                std::vector<bool> mark;
                for (uint64_t i = 0; i < K; i++) {
                    const uint32_t a = 1 + (uint32_t)(rng() % (n - 1));
                    uint32_t b = (uint32_t)(rng() % a);
                    b -= std::min(b, (b % fam + fam - a % fam) % fam);
                    Edge x{a, b, 0, 0};
                    weight(x.numer, x.denom);
                    if (rng() % 2) std::swap(x.row, x.col);                   // a list names a pair either way round
                    e.push_back(x);
                    mark.push_back(a % fam == b % fam && (double)(rng() % 1000000) < dens * 1e6 && !have[(size_t)a * n + b]++);
                }
                Launch L = list_launch(e);
                for (uint64_t i = 0; i < K; i++)
                    if (mark[i]) L.set(i);
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
    if (c == "small") case_small();
    else if (c == "path") case_path();
    else if (c == "clique") case_clique();
    else if (c == "star") case_star();
    else if (c == "parts") case_parts();
    else if (c == "denoms") case_denoms();
    else if (c == "density") case_density();
    else if (c == "blocks") case_blocks();
    else if (c == "overflow") case_overflow();
    else if (c == "fuzz" && argc > 3) fuzz(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
    else { fprintf(stderr, "usage: forest_emu small|path|clique|star|parts|denoms|density|blocks|overflow | fuzz <seed> <n>\n"); return 2; }
    if (failures) { printf("%d case(s) FAILED\n", failures); return 1; }
    printf("all cases agree\n");
    return 0;
}
