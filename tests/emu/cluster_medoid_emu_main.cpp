// cluster_medoid_emu_main.cpp -- runs the kernels of `mash cluster -M`, unchanged, through their launchers on the CPU (tools/hipemu):
// cm_union_kernel (cluster_medoid.hip) in both variants -- a row's weights combined in the wave, and two atomics per edge -- over
// ballot words in list mode and in flat triangle mode, cl_label_kernel (cluster.hip), and launch_medoid_pick (cm_best_kernel,
// cm_pick_kernel, cm_medoid_kernel).  The judge is a sequential restatement written here: a plain union-find, one pass over the edges
// for the scores, a walk in index order for the medoids.  Which pairs a launch names is stated by the definition of the layouts
// (entries_of), not by pair_rc.  The driver does what the host does: parent and score live across the launches of a job, score is
// cleared once, then labels, then the pick.
// TEST INFRASTRUCTURE (tests/test_cluster_medoid_emu.py); built with g++.  The emulator runs workgroups one after another: what is
// pinned here is the arithmetic (which lanes combine, the weights, the floors, the ties, the bounds), not the races between
// workgroups.
//
//   cluster_medoid_emu <case>            cases: small lengths words lists space blocks weights shapes ties
//   cluster_medoid_emu fuzz <seed> <n>   n random jobs
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <random>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../mash_amd/csrc/cluster.hip"
#include "../../mash_amd/csrc/cluster_medoid.hip"

using namespace mg;

struct Edge { uint32_t row, col, numer, denom; };

// one union launch: a list of pairs with their counts and a mask, or rows [first_row, row_end) of the flat triangle with a mask;
// sp: the launch's pair space (rows == 0: the whole table)
struct Launch {
    std::vector<uint2> rc;                       // list mode (empty: flat)
    std::vector<uint2> counts;                   // {numer, denom} of every pair of the launch, marked or not
    uint64_t first_row = 0, pairs = 0;
    std::vector<unsigned long long> masks;
    PairSpace sp{0, 0, 0, 0};
    void set(uint64_t idx) { masks[idx >> 6] |= 1ull << (idx & 63); }
    bool get(uint64_t idx) const { return (masks[idx >> 6] >> (idx & 63)) & 1ull; }
};

static uint64_t tri(uint64_t r) { return r ? r * (r - 1) / 2 : 0; }

// every pair carries counts, also the ones no bit marks: they must not reach a score
static uint2 junk_counts(uint64_t idx) { return make_uint2((uint32_t)(idx * 7 % 61) + 1u, 61u); }

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

// the edges a launch names over a table of n rows, in parent[]'s index space, by the definition of the layouts
static void entries_of(const Launch &L, uint32_t n, std::vector<Edge> &out)
{
    const PairSpace sp = L.sp.rows ? L.sp : PairSpace{n, n, 0u, 0u};
    if (!L.rc.empty()) {
        for (uint64_t i = 0; i < L.pairs; i++)
            if (L.get(i) && L.rc[i].x < sp.rows && L.rc[i].y < sp.cols)
                out.push_back({sp.row_base + L.rc[i].x, sp.col_base + L.rc[i].y, L.counts[i].x, L.counts[i].y});
        return;
    }
    uint64_t row = L.first_row, col = 0;
    if (row == 0) row = 1;
    for (uint64_t i = 0; i < L.pairs; i++) {
        if (L.get(i) && row < sp.rows && col < sp.cols) out.push_back({sp.row_base + (uint32_t)row, sp.col_base + (uint32_t)col, L.counts[i].x, L.counts[i].y});
        if (++col == row) { row++; col = 0; }
    }
}

static int failures = 0;
constexpr uint32_t GUARD = 0xDEADBEEFu;
constexpr unsigned long long GUARD64 = 0xDEADBEEFDEADBEEFull;
constexpr unsigned long long ONE = 1ull << 32;
static const uint32_t kRareDenom[3] = {0u, 32u, 63u}, kMixedDenom[3] = {63u, 64u, 32u};

struct Answer { std::vector<uint32_t> label, medoid; std::vector<unsigned long long> score; uint64_t clusters = 0, moved = 0, ties = 0; };

// the judge: the division is written out here, not taken from forest_key.h
static Answer judge(uint32_t n, const std::vector<Edge> &edges)
{
    Answer w;
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) { while (parent[x] != x) x = parent[x]; return x; };
    w.score.assign(n, 0);
    for (const Edge &e : edges) {
        const uint32_t a = find(e.row), b = find(e.col);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
        const unsigned long long wt = (unsigned long long)e.numer * ONE / (e.denom == 0 ? 1u : e.denom);
        w.score[e.row] += wt;
        w.score[e.col] += wt;
    }
    w.label.resize(n);
    w.medoid.resize(n);
    std::vector<uint32_t> top(n), size(n, 0), at_top(n, 0);
    for (uint32_t i = 0; i < n; i++) { w.label[i] = find(i); top[i] = i; }
    for (uint32_t i = 0; i < n; i++)
        if (w.score[i] > w.score[top[w.label[i]]]) top[w.label[i]] = i;
    for (uint32_t i = 0; i < n; i++) {
        w.medoid[i] = top[w.label[i]];
        size[w.label[i]]++;
        at_top[w.label[i]] += w.score[i] == w.score[top[w.label[i]]];
    }
    for (uint32_t i = 0; i < n; i++) {
        if (w.label[i] != i) continue;
        w.clusters++;
        w.moved += top[i] != i;
        w.ties += size[i] >= 2 && at_top[i] >= 2;
    }
    return w;
}

struct Want { const std::vector<uint32_t> *medoid = nullptr; const std::vector<unsigned long long> *score = nullptr; };

static void check(const char *name, uint32_t n, const std::vector<Launch> &launches, Want want = {})
{
    std::vector<Edge> edges;
    for (const Launch &L : launches) entries_of(L, n, edges);
    const Answer w = judge(n, edges);
    bool ok = (!want.medoid || *want.medoid == w.medoid) && (!want.score || *want.score == w.score);      // the judge itself against the closed form
    uint64_t bad = 0;
    for (int plain = 0; plain < 2; plain++) {
        std::vector<uint32_t> parent(n + 1, GUARD), label(n + 1, GUARD), medoid(n + 1, GUARD), pick(n + 1, GUARD);
        std::vector<unsigned long long> score(n + 1, GUARD64), best(n + 1, GUARD64);                      // (best and pick: junk the launcher must clear)
        unsigned long long roots = ~0ull;
        ok = ok && launch_cluster_init(parent.data(), n, nullptr) == hipSuccess;
        std::fill(score.begin(), score.begin() + n, 0ull);                                               // once, before the first launch
        for (const Launch &L : launches) {
            FinishArgs a{};
            a.pairs = L.pairs;
            a.first_row = L.first_row;
            a.triangle = 1;
            a.counts = L.counts.data();
            a.masks = const_cast<unsigned long long *>(L.masks.data());
            a.list_rc = L.rc.empty() ? nullptr : L.rc.data();
            ok = ok && launch_medoid_union(a, parent.data(), score.data(), L.sp.rows ? L.sp : PairSpace{n, n, 0u, 0u}, nullptr, plain != 0) == hipSuccess;
        }
        ok = ok && launch_cluster_label(parent.data(), n, label.data(), &roots, nullptr) == hipSuccess;
        ok = ok && launch_medoid_pick(label.data(), score.data(), n, best.data(), pick.data(), medoid.data(), nullptr) == hipSuccess;
        ok = ok && parent[n] == GUARD && label[n] == GUARD && medoid[n] == GUARD && pick[n] == GUARD && score[n] == GUARD64 && best[n] == GUARD64;
        ok = ok && roots == w.clusters;
        for (uint32_t i = 0; i < n; i++) bad += (label[i] != w.label[i]) + (score[i] != w.score[i]) + (medoid[i] != w.medoid[i]);
    }
    if (!ok || bad) {
        failures++;
        printf("FAIL %s: n %u edges %zu: %llu values differ%s\n", name, n, edges.size(), (unsigned long long)bad,
               ok ? "" : " (launch, guard word, cluster count or closed form)");
    } else {
        printf("ok   %s: n %u edges %zu clusters %llu, %llu with a medoid that is not their first member, %llu with a tie for the top score\n", name, n,
               edges.size(), (unsigned long long)w.clusters, (unsigned long long)w.moved, (unsigned long long)w.ties);
    }
}

static std::vector<Edge> random_pairs(std::mt19937_64 &rng, uint32_t n, uint64_t K, uint32_t fam)
{
    std::vector<Edge> q;
    for (uint64_t i = 0; i < K; i++) {
        const uint32_t a = 1 + (uint32_t)(rng() % (n - 1));
        uint32_t b = (uint32_t)(rng() % a);
        b -= std::min(b, (b % fam + fam - a % fam) % fam);
        const uint32_t d = rng() % 4 ? 64u : kRareDenom[rng() % 3];  // 64 mostly; 0, 32 and 63 otherwise
        const uint32_t m = d == 63 ? (uint32_t)(rng() % 4) * 21u : d ? (uint32_t)(rng() % 5) * (d / 4) : 0u;   // quarters and thirds: ties are common
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
    Launch F = flat_launch(0, 100);
    for (uint64_t i = 0; i < F.pairs; i += 3) { F.set(i); F.counts[i] = make_uint2((uint32_t)(i % 5) * 16u, 64u); }
    check("100 rows, flat", 100, {F});
    std::vector<uint32_t> star(20, 19u);
    std::vector<Edge> s;
    for (uint32_t i = 0; i < 19; i++) s.push_back({19, i, 32, 64});
    check("a star whose centre is the last row", 20, {list_all(s)}, {&star, nullptr});
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
    for (uint32_t n : {2u, 3u, 12u, 65u, 91u, 130u}) {                               // triangles of 1, 3, 66, 2080, 4095, 8385 pairs, every bit set
        Launch F = flat_launch(0, n);
        for (uint32_t r = 1; r < n; r++)
            for (uint32_t c = 0; c < r; c++) flat_set(F, {r, c, (r * 5 + c) % 65, 64});
        check(("whole triangle of " + std::to_string(n) + " rows").c_str(), n, {F});
    }
}

static void case_words()
{
    // the first word of a flat triangle spans rows 1 .. 11 (and the second rows 11 .. 16): more rows than the wave combines
    Launch F = flat_launch(0, 17);
    std::vector<unsigned long long> score(17, 16ull * (ONE / 2));
    std::vector<uint32_t> med(17, 0u);
    for (uint32_t r = 1; r < 17; r++)
        for (uint32_t c = 0; c < r; c++) flat_set(F, {r, c, 32, 64});
    check("the first words of a triangle, every bit set", 17, {F}, {&med, &score});
    // words that span exactly two rows: rows 100 .. 102 begin at pair 4950 = 77 * 64 + 22
    Launch G = flat_launch(100, 103);
    for (uint32_t r = 100; r < 103; r++)
        for (uint32_t c = 0; c < r; c++) flat_set(G, {r, c, 1 + (r + c) % 64, 64});
    check("words of two rows, every bit set", 103, {G});
    Launch H = flat_launch(100, 103);
    for (uint32_t r = 100; r < 103; r++)
        for (uint32_t c = r % 3; c < r; c += 3) flat_set(H, {r, c, 21, 63});
    check("words of two rows, every third bit", 103, {H});
    // a single set bit, in the last lane of its word
    Launch S = flat_launch(0, 40);
    S.set(63);
    S.counts[63] = make_uint2(21, 63);                                              // pair 63 = {11, 8}
    std::vector<unsigned long long> one(40, 0ull);
    one[11] = one[8] = ONE / 3;
    check("one set bit in lane 63, flat", 40, {S}, {nullptr, &one});
    std::vector<Edge> q(128, Edge{1, 0, 5, 64});
    q[63] = {30, 2, 64, 64};
    q[127] = {31, 30, 16, 32};
    Launch Q = list_launch(q);
    Q.set(63);
    Q.set(127);
    check("one set bit in lane 63 of two words, list", 40, {Q});
}

static void case_lists()
{
    // rows in no order, the same row in lanes far apart: three rows dealt round the lanes, then seven (more than the wave combines),
    // then every lane a row of its own, then one row in all 64 lanes
    for (uint32_t k : {1u, 2u, 3u, 4u, 5u, 7u, 64u}) {
        std::vector<Edge> e;
        for (uint32_t i = 0; i < 192; i++) {
            const uint32_t row = 500 + (i * 5) % k * 7;                              // (rows 500, 507, .. in an order that is not ascending)
            e.push_back({row, i + (i % 2) * 200, 1 + i % 63, 63 + i % 2});           // distinct columns below 500, two denominators
        }
        check(("a list dealing " + std::to_string(k) + " rows round the lanes").c_str(), 1000, {list_all(e)});
        Launch L = list_launch(e);
        for (uint64_t i = 0; i < L.pairs; i++)
            if (i % 3 != 1) L.set(i);
        check("the same, a third of the bits clear", 1000, {L});
        for (Edge &x : e) std::swap(x.row, x.col);                                   // the shared index in the COLUMN place: no lanes to combine
        check("the same, named the other way round", 1000, {list_all(e)});
    }
    // descending rows
    std::vector<Edge> d;
    for (uint32_t i = 0; i < 300; i++) d.push_back({900 - i / 4, i, 32, 64});
    check("a list with descending rows", 1000, {list_all(d)});
}

static void case_space()
{
    // a pair space smaller than the table: set bits whose row or column lies outside it add nothing and join nothing
    std::vector<Edge> e;
    for (uint32_t i = 0; i < 200; i++) e.push_back({i % 40, (i * 7) % 25 + 40 * (i % 2), 16 + i % 40, 64});
    Launch L = list_all(e);
    L.sp = PairSpace{30, 50, 100, 0};                                                // rows 0 .. 29 -> 100 .. 129; columns 0 .. 49
    check("a list, rows and columns outside the pair space", 200, {L});
    L.sp = PairSpace{40, 20, 60, 10};
    check("a list, a base on both sides", 200, {L});
    Launch F = flat_launch(0, 90);
    for (uint32_t r = 1; r < 90; r++)
        for (uint32_t c = r % 2; c < r; c += 2) flat_set(F, {r, c, 8 + (r + c) % 50, 64});
    F.sp = PairSpace{70, 33, 0, 0};
    check("flat, rows >= 70 and columns >= 33 outside the pair space", 90, {F});
    F.sp = PairSpace{1, 90, 0, 0};                                                   // no row of a triangle is below 1: nothing at all
    check("flat, every set bit outside the pair space", 90, {F});
}

static std::vector<Launch> row_blocks(uint32_t n, const std::vector<uint32_t> &cuts, uint64_t seed)
{
    std::mt19937_64 rng(seed);
    std::vector<Launch> v;
    for (size_t b = 0; b + 1 < cuts.size(); b++) {
        Launch F = flat_launch(cuts[b], cuts[b + 1]);
        for (uint32_t r = std::max(cuts[b], 1u); r < cuts[b + 1]; r++)
            for (int k = 0; k < 6; k++) {
                const uint32_t c = (uint32_t)(rng() % r);
                if ((r % 7) == (c % 7)) flat_set(F, {r, c, (uint32_t)(rng() % 5) * 16u, 64u});
            }
        v.push_back(F);
    }
    (void)n;
    return v;
}

static void case_blocks()
{
    check("two row blocks over one score[]", 900, row_blocks(900, {0, 450, 900}, 17));
    check("three row blocks over one score[]", 900, row_blocks(900, {0, 1, 700, 900}, 19));
    check("five row blocks, the first and the last of one row", 1500, row_blocks(1500, {0, 1, 700, 701, 1499, 1500}, 23));
    // a list and a flat block in one job (no route mixes them, the arithmetic does not care)
    std::vector<Launch> v = row_blocks(400, {0, 200}, 5);
    std::vector<Edge> e;
    for (uint32_t r = 200; r < 400; r++) e.push_back({r, r - 200, 21, 63});
    v.push_back(list_all(e));
    check("a flat block, then a list", 400, v);
}

static void case_weights()
{
    // 0/0 and 0/d edges join and add nothing
    std::vector<uint32_t> m5{2, 2, 2, 2, 4};
    std::vector<unsigned long long> s5{0, 0, ONE / 64, ONE / 64, 0};
    check("0/0 and 0/64 edges", 5, {list_all({{1, 0, 0, 0}, {2, 1, 0, 64}, {3, 2, 1, 64}})}, {&m5, &s5});
    // 21/63: a weight that is no multiple of 2^-32 -- the floor is taken per edge, before any sum, in the wave or in memory
    std::vector<unsigned long long> s4{ONE / 3 + ONE / 2, 2 * (ONE / 3), 2 * (ONE / 3), ONE / 3 + ONE / 2};
    std::vector<uint32_t> m4{0, 0, 0, 0};
    check("21/63 beside 32/64", 4, {list_all({{1, 0, 21, 63}, {2, 1, 21, 63}, {3, 2, 21, 63}, {3, 0, 32, 64}})}, {&m4, &s4});
    // one row with 64 edges of 21/63 in one word: 64 * floor(2^32 / 3), not floor(64 * 2^32 / 3)
    std::vector<Edge> e;
    for (uint32_t c = 0; c < 64; c++) e.push_back({64, c, 21, 63});
    std::vector<unsigned long long> s65(65, ONE / 3);
    s65[64] = 64 * (ONE / 3);
    std::vector<uint32_t> m65(65, 64u);
    check("64 edges of 21/63 at one row", 65, {list_all(e)}, {&m65, &s65});
    Launch F = flat_launch(64, 65);
    for (uint32_t c = 0; c < 64; c++) flat_set(F, {64, c, 21, 63});
    check("the same, flat", 65, {F}, {&m65, &s65});
    // denominators 63, 64 and 32 mixed in the words of a triangle
    Launch G = flat_launch(0, 150);
    for (uint32_t r = 1; r < 150; r++)
        for (uint32_t c = 0; c < r; c++) {
            if ((r + 2 * c) % 3 == 0) continue;
            const uint32_t d = kMixedDenom[(r * 3 + c) % 3];
            flat_set(G, {r, c, (r * 11 + c * 5) % (d + 1), d});
        }
    check("denominators 63, 64 and 32 in one triangle", 150, {G});
    // full weights: numer == denom, 2^32 each
    std::vector<Edge> f;
    for (uint32_t c = 0; c < 200; c++) f.push_back({200, c, 64, 64});
    std::vector<unsigned long long> s201(201, ONE);
    s201[200] = 200 * ONE;
    check("200 edges of 64/64 at one row", 201, {list_all(f)}, {nullptr, &s201});
}

static void case_shapes()
{
    const uint32_t n = 700;
    std::vector<Edge> clique;
    for (uint32_t r = 1; r < 90; r++)
        for (uint32_t c = 0; c < r; c++) clique.push_back({r, c, 16, 64});
    std::vector<uint32_t> m_clique(90, 0u);
    check("a clique of equal weights", 90, {list_all(clique)}, {&m_clique, nullptr});
    Launch F = flat_launch(0, n);
    std::vector<uint32_t> m_star(n, n - 1);
    for (uint32_t c = 0; c + 1 < n; c++) flat_set(F, {n - 1, c, 40, 64});
    check("a star whose centre is the LAST row, flat", n, {F}, {&m_star, nullptr});
    std::vector<Edge> path;
    for (uint32_t i = 1; i < n; i++) path.push_back({i, i - 1, 64, 64});
    std::vector<uint32_t> m_path(n, 1u);
    check("a path", n, {list_all(path)}, {&m_path, nullptr});
    // two clusters interleaved in index order: the even rows around row 400, the odd rows around row 301
    std::vector<Edge> two;
    std::vector<uint32_t> m_two(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t centre = i % 2 ? 301u : 400u;
        m_two[i] = centre;
        if (i != centre) two.push_back({std::max(i, centre), std::min(i, centre), 30 + i % 20, 64});
    }
    check("two clusters interleaved in index order", n, {list_all(two)}, {&m_two, nullptr});
    Launch T = flat_launch(0, n);
    for (const Edge &e : two) flat_set(T, e);
    check("the same, flat", n, {T}, {&m_two, nullptr});
    // the band of window_table: row i beside rows i - 1 .. i - 3 sharing 1000 - 100 k of 1000; rows 3 .. n - 4 tie, row 3 wins
    Launch B = flat_launch(0, 300);
    std::vector<uint32_t> m_band(300, 3u);
    std::vector<unsigned long long> s_band(300, 0ull);
    for (uint32_t i = 1; i < 300; i++)
        for (uint32_t k = 1; k <= 3 && k <= i; k++) {
            flat_set(B, {i, i - k, 1000 - 100 * k, 1000});
            s_band[i] += (unsigned long long)(1000 - 100 * k) * ONE / 1000;
            s_band[i - k] += (unsigned long long)(1000 - 100 * k) * ONE / 1000;
        }
    check("the band of 300 rows", 300, {B}, {&m_band, &s_band});
}

static void case_ties()
{
    std::vector<uint32_t> m2{0, 0};
    check("a cluster of two", 2, {list_all({{1, 0, 17, 64}})}, {&m2, nullptr});
    // rows 2 and 5 reach the same sum by different edges, also under different denominators: the smaller row
    std::vector<Edge> e{{2, 0, 32, 64}, {2, 1, 16, 64}, {5, 3, 8, 32}, {5, 4, 16, 32}, {5, 2, 0, 64}};
    std::vector<uint32_t> m6{2, 2, 2, 2, 2, 2};
    check("equal sums under different denominators", 6, {list_all(e)}, {&m6, nullptr});
    std::reverse(e.begin(), e.end());
    check("the same, edges backwards", 6, {list_all(e)}, {&m6, nullptr});
    // the tie is among rows that are not the first member, in many clusters at once
    std::vector<Edge> many;
    std::vector<uint32_t> m_many(4 * 300);
    for (uint32_t g = 0; g < 300; g++) {
        const uint32_t b = 4 * g;                                                    // b - (b+2) - (b+3) - (b+1): the inner rows b + 2 and b + 3 tie
        many.push_back({b + 2, b, 10, 64});
        many.push_back({b + 3, b + 2, 20, 64});
        many.push_back({b + 3, b + 1, 10, 64});
        for (uint32_t k = 0; k < 4; k++) m_many[b + k] = b + 2;
    }
    check("300 clusters, each with a tie away from its first member", 1200, {list_all(many)}, {&m_many, nullptr});
    Launch F = flat_launch(0, 1200);
    for (const Edge &x : many) flat_set(F, x);
    check("the same, flat", 1200, {F}, {&m_many, nullptr});
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
                        const uint32_t d = rng() % 4 ? 64u : kRareDenom[rng() % 3];
                        F.counts[i] = make_uint2(d == 63 ? (uint32_t)(rng() % 4) * 21u : d ? (uint32_t)(rng() % 5) * (d / 4) : 0u, d);
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
        check(("fuzz " + std::to_string(j)).c_str(), n, v);
    }
}

int main(int argc, char **argv)
{
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "small") case_small();
    else if (c == "lengths") case_lengths();
    else if (c == "words") case_words();
    else if (c == "lists") case_lists();
    else if (c == "space") case_space();
    else if (c == "blocks") case_blocks();
    else if (c == "weights") case_weights();
    else if (c == "shapes") case_shapes();
    else if (c == "ties") case_ties();
    else if (c == "fuzz" && argc > 3) fuzz(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
    else { fprintf(stderr, "usage: cluster_medoid_emu small|lengths|words|lists|space|blocks|weights|shapes|ties | fuzz <seed> <n>\n"); return 2; }
    if (failures) { printf("%d case(s) FAILED\n", failures); return 1; }
    printf("all cases agree\n");
    return 0;
}
