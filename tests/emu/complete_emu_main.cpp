// complete_emu_main.cpp -- runs mash_amd/csrc/cluster_complete.hip, unchanged, through its launchers (the keys and the lookup of
// launch_complete_begin; the rounds cc_key_kernel / cc_rc_kernel / cc_mate_kernel / cc_decide_kernel / cc_commit_kernel as
// launch_complete_rounds queues them) behind cluster_forest.hip's append and in front of cluster.hip's labels, on the CPU
// (tools/hipemu), and compares the labels with a sequential walk of the definition written here (adjacency maps, an ordered set,
// 128-bit cross-multiplication).  The driver below does what cluster_complete_tri does on the host: append per launch, regrow and
// append again when the list overflows, the index once behind the last append, the rounds in batches that double, one look at
// merged[] per batch.
// TEST INFRASTRUCTURE (tests/test_complete_emu.py); built with g++.  The emulator runs workgroups one after another: what is pinned
// here is the arithmetic (the keys, the probes, the decisions of a round, the batches), not the races between workgroups.
//
//   complete_emu <case>            cases: small clique path joined both denoms lists hash batches
//   complete_emu fuzz <seed> <n>   n random jobs
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../mash_amd/csrc/cluster.hip"
#include "../../mash_amd/csrc/cluster_forest.hip"
#include "../../mash_amd/csrc/cluster_complete.hip"

using namespace mg;

struct Edge { uint32_t row, col, numer, denom; };

// the definition's order: larger fraction first, equal fractions by the larger id, then the smaller
struct RanksBefore {
    bool operator()(const Edge &a, const Edge &b) const
    {
        const unsigned __int128 l = (unsigned __int128)a.numer * (b.denom ? b.denom : 1u), r = (unsigned __int128)b.numer * (a.denom ? a.denom : 1u);
        return l != r ? l > r : a.row != b.row ? a.row < b.row : a.col < b.col;
    }
};

struct Weight { uint32_t numer, denom; };
static Weight worse(const Weight &a, const Weight &b)
{
    const unsigned __int128 l = (unsigned __int128)a.numer * (b.denom ? b.denom : 1u), r = (unsigned __int128)b.numer * (a.denom ? a.denom : 1u);
    return l < r ? a : b;
}

// the sequential walk -> label; *merges = how many links it merged
static std::vector<uint32_t> walk(uint32_t n, const std::vector<Edge> &edges, uint64_t *merges)
{
    std::vector<std::map<uint32_t, Weight>> links(n);
    std::set<Edge, RanksBefore> order;
    auto link_of = [](uint32_t a, uint32_t b, const Weight &w) { return Edge{std::max(a, b), std::min(a, b), w.numer, w.denom}; };
    for (const Edge &e : edges) {
        links[e.row][e.col] = links[e.col][e.row] = Weight{e.numer, e.denom};
        order.insert(link_of(e.row, e.col, Weight{e.numer, e.denom}));
    }
    std::vector<uint32_t> up(n);
    for (uint32_t i = 0; i < n; i++) up[i] = i;
    *merges = 0;
    while (!order.empty()) {
        const Edge first = *order.begin();
        const uint32_t gone = first.row, stay = first.col;
        std::map<uint32_t, Weight> both;
        for (const auto &kv : links[gone]) {
            order.erase(link_of(gone, kv.first, kv.second));
            links[kv.first].erase(gone);
            const auto at = links[stay].find(kv.first);
            if (kv.first != stay && at != links[stay].end()) both[kv.first] = worse(kv.second, at->second);
        }
        for (const auto &kv : links[stay]) {
            order.erase(link_of(stay, kv.first, kv.second));
            links[kv.first].erase(stay);
        }
        for (const auto &kv : both) {
            links[kv.first][stay] = kv.second;
            order.insert(link_of(stay, kv.first, kv.second));
        }
        links[gone].clear();
        links[stay] = both;
        up[gone] = stay;
        ++*merges;
    }
    for (uint32_t i = 0; i < n; i++) up[i] = up[up[i]];           // (larger under smaller: one pass in index order)
    return up;
}

// one append launch: a list of pairs with their counts and a mask, or rows [first_row, row_end) of the flat triangle with a mask
struct Launch {
    std::vector<uint2> rc;                       // list mode (empty: flat)
    std::vector<uint2> counts;
    uint64_t first_row = 0, pairs = 0;
    std::vector<unsigned long long> masks;
    void set(uint64_t idx) { masks[idx >> 6] |= 1ull << (idx & 63); }
    bool get(uint64_t idx) const { return (masks[idx >> 6] >> (idx & 63)) & 1ull; }
};

static uint64_t tri(uint64_t r) { return r ? r * (r - 1) / 2 : 0; }

// a list that names every edge, either way round, between pairs that no bit marks
static Launch list_of(const std::vector<Edge> &e, bool with_unmarked = false)
{
    Launch L;
    std::vector<bool> marked;
    for (size_t i = 0; i < e.size(); i++) {
        if (with_unmarked && i % 3 == 0) {
            L.rc.push_back(make_uint2(e[i].col, e[i].row));
            L.counts.push_back(make_uint2(1u, 1u));                // (a perfect pair that is NOT marked: it must not reach the list)
            marked.push_back(false);
        }
        L.rc.push_back(i % 2 ? make_uint2(e[i].row, e[i].col) : make_uint2(e[i].col, e[i].row));
        L.counts.push_back(make_uint2(e[i].numer, e[i].denom));
        marked.push_back(true);
    }
    L.pairs = L.rc.size();
    L.masks.assign((L.pairs + 63) / 64, 0);
    for (uint64_t i = 0; i < L.pairs; i++)
        if (marked[i]) L.set(i);
    return L;
}

static Launch flat_rows(uint64_t first_row, uint64_t row_end, const std::vector<Edge> &e)
{
    Launch L;
    L.first_row = first_row;
    L.pairs = tri(row_end) - tri(first_row);
    L.masks.assign((L.pairs + 63) / 64, 0);
    L.counts.assign(L.pairs, make_uint2(1u, 1u));
    for (const Edge &x : e)
        if (x.row >= first_row && x.row < row_end) {
            const uint64_t idx = tri(x.row) + x.col - tri(first_row);
            L.set(idx);
            L.counts[idx] = make_uint2(x.numer, x.denom);
        }
    return L;
}

static int failures = 0;
constexpr uint32_t GUARD = 0xDEADBEEFu;
constexpr unsigned long long GUARD64 = 0xDEADBEEFDEADBEEFull;

struct Opts {
    uint64_t first_cap = 0;                      // the first capacity of the edge list (0: room for everything)
    uint32_t first_batch = 8;
    uint64_t hash_and = ~0ull, hash_or = 0;      // hash_or == ~0: the table's last slot
    bool want_regrow = false;
    long want_rounds = -1, want_batches = -1, want_clusters = -1;      // rounds: all that ran, the one that merged nothing among them
};

static void check(const char *name, uint32_t n, const std::vector<Edge> &edges, const std::vector<Launch> &launches, const Opts &o = Opts())
{
    uint64_t want_merges = 0;
    const std::vector<uint32_t> want = walk(n, edges, &want_merges);

    bool ok = true;
    uint64_t cap = o.first_cap ? o.first_cap : std::max<uint64_t>(edges.size(), 1), used = 0, regrows = 0;
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
        for (int attempt = 0;; attempt++) {
            ok = ok && launch_forest_append(a, n, list.data(), cap, &cursor, &overflow, nullptr) == hipSuccess;
            ok = ok && list[cap].x == GUARD && (overflow != 0) == (cursor > cap);
            if (cursor <= cap) break;
            if (attempt) { ok = false; break; }
            const uint64_t bigger = std::max<uint64_t>(cursor, 2 * cap);
            std::vector<uint4> nl(bigger + 1, make_uint4(GUARD, GUARD, GUARD, GUARD));
            std::copy(list.begin(), list.begin() + (long)used, nl.begin());
            list.swap(nl);
            cap = bigger;
            cursor = used;
            overflow = 0;
            regrows++;
        }
        used = cursor;
    }
    const uint64_t m = used, slots = complete_slots(m);
    ok = ok && m == edges.size() && slots > 2 * m;

    constexpr uint32_t kBatchMax = 256;
    std::vector<uint32_t> parent(n + 1, GUARD), mate(n + 1, GUARD), merged(kBatchMax + 1, GUARD), label(n + 1, GUARD);
    std::vector<unsigned long long> best_key(n + 1, GUARD64), best_rc(n + 1, GUARD64), key(m + 1, GUARD64), next(m + 1, GUARD64), slot_rc(slots + 1, GUARD64),
        slot_e(slots + 1, GUARD64), live(kBatchMax + 1, GUARD64);
    const CompleteBufs cb{parent.data(), mate.data(), best_key.data(), best_rc.data(), key.data(), next.data(), slot_rc.data(), slot_e.data(), slots,
                          o.hash_and, o.hash_or == ~0ull ? slots - 1 : o.hash_or, merged.data(), live.data()};
    ok = ok && launch_complete_begin(list.data(), m, cb, n, nullptr) == hipSuccess;
    // the lookup holds every link once, at a slot its probe reaches, and nothing else
    uint64_t filled = 0;
    for (uint64_t s = 0; s < slots && m; s++)
        if (slot_rc[s] != CF_NONE) {
            filled++;
            const unsigned long long e = slot_e[s];
            ok = ok && e < m && forest_rc(list[e].x, list[e].y) == slot_rc[s] && key[e] == forest_key(list[e].z, list[e].w);
        }
    ok = ok && (!m || filled == m);

    uint64_t rounds = 0, batches = 0, total_merged = 0;
    std::vector<unsigned long long> all_live;
    bool reached = m == 0;
    for (uint32_t batch = o.first_batch; m && !reached; batch = std::min(batch * 2, kBatchMax)) {
        ok = ok && launch_complete_rounds(list.data(), m, cb, n, batch, nullptr) == hipSuccess;
        batches++;
        uint32_t r = 0;
        while (r < batch && merged[r]) r++;
        const uint32_t ran = std::min(r + 1, batch);
        for (uint32_t k = 0; k < ran; k++) {
            total_merged += merged[k];
            all_live.push_back(live[k]);
            ok = ok && live[k] >= merged[k];
        }
        for (uint32_t k = ran; k < batch; k++) ok = ok && merged[k] == 0 && live[k] == 0;          // queued behind the fixpoint: nothing ran
        ok = ok && merged[kBatchMax] == GUARD && live[kBatchMax] == GUARD64;
        rounds += ran;
        reached = r < batch;
        if (!reached && rounds > n) { ok = false; break; }
    }
    if (m) {
        ok = ok && reached && all_live[0] == edges.size() && all_live.back() == 0;      // (a live link: the first of all would have merged)
        for (size_t k = 1; k < all_live.size(); k++) ok = ok && all_live[k] < all_live[k - 1];
        // a whole batch more, queued behind the fixpoint: its first round runs and merges nothing, the others do nothing, and
        // every array is as the fixpoint left it
        const std::vector<uint32_t> p0 = parent;
        const std::vector<unsigned long long> k0 = key;
        ok = ok && launch_complete_rounds(list.data(), m, cb, n, 5, nullptr) == hipSuccess;
        ok = ok && merged[0] == 0 && live[0] == all_live.back() && merged[1] == 0 && live[1] == 0 && parent == p0 && key == k0;
    }
    for (uint32_t i = 0; i < n; i++) ok = ok && mate[i] == ~0u && best_key[i] == 0 && best_rc[i] == ~0ull && parent[i] <= i;

    unsigned long long roots = GUARD64;
    ok = ok && launch_cluster_label(parent.data(), n, label.data(), &roots, nullptr) == hipSuccess;
    ok = ok && parent[n] == GUARD && mate[n] == GUARD && label[n] == GUARD && best_key[n] == GUARD64 && best_rc[n] == GUARD64 && key[m] == GUARD64 &&
         next[m] == GUARD64 && slot_rc[slots] == GUARD64 && slot_e[slots] == GUARD64 && list[cap].x == GUARD;
    uint64_t bad = 0, want_roots = 0;
    for (uint32_t i = 0; i < n; i++) {
        bad += label[i] != want[i];
        want_roots += want[i] == i;
    }
    ok = ok && roots == want_roots && total_merged == want_merges && total_merged + roots == n;
    // what the walk gives is what the definition promises: every cluster a clique of the edges
    std::set<std::pair<uint32_t, uint32_t>> have;
    for (const Edge &e : edges) have.insert({e.row, e.col});
    std::map<uint32_t, std::vector<uint32_t>> members;
    for (uint32_t i = 0; i < n; i++) members[label[i]].push_back(i);
    for (const auto &kv : members)
        for (size_t x = 0; x < kv.second.size() && kv.second.size() <= 200; x++)
            for (size_t y = x + 1; y < kv.second.size(); y++) bad += !have.count({kv.second[y], kv.second[x]});
    const bool shaped = (!o.want_regrow || regrows > 0) && (o.want_rounds < 0 || (uint64_t)o.want_rounds == rounds) &&
                        (o.want_batches < 0 || (uint64_t)o.want_batches == batches) && (o.want_clusters < 0 || (uint64_t)o.want_clusters == roots);
    if (!ok || bad || !shaped) {
        failures++;
        printf("FAIL %s: n %u edges %zu: %llu labels or cliques differ, clusters %llu want %llu, merged %llu want %llu, rounds %llu batches %llu regrows %llu%s%s\n",
               name, n, edges.size(), (unsigned long long)bad, roots, (unsigned long long)want_roots, (unsigned long long)total_merged,
               (unsigned long long)want_merges, (unsigned long long)rounds, (unsigned long long)batches, (unsigned long long)regrows,
               ok ? "" : " (launch, guard word, lookup, rounds or reset state)", shaped ? "" : " (not the rounds, batches, clusters or regrow the case is about)");
    } else {
        printf("ok   %s: n %u edges %zu clusters %llu rounds %llu batches %llu regrows %llu\n", name, n, edges.size(), roots, (unsigned long long)rounds,
               (unsigned long long)batches, (unsigned long long)regrows);
    }
}

static void check_list(const char *name, uint32_t n, const std::vector<Edge> &e, const Opts &o = Opts()) { check(name, n, e, {list_of(e)}, o); }

static Opts rounds_and_clusters(long rounds, long clusters)
{
    Opts o;
    o.want_rounds = rounds;
    o.want_clusters = clusters;
    return o;
}

static std::vector<Edge> clique(uint32_t first, uint32_t end, uint32_t numer, uint32_t denom)
{
    std::vector<Edge> e;
    for (uint32_t r = first + 1; r < end; r++)
        for (uint32_t c = first; c < r; c++) e.push_back({r, c, numer, denom});
    return e;
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

static void case_small()                                                     // (also the ThreadSanitizer build's case)
{
    check("no rows", 0, {}, {});
    check("one row", 1, {}, {});
    check_list("two rows, one edge", 2, {{1, 0, 3, 4}}, rounds_and_clusters(2, 1));
    check_list("two rows, no edge", 2, {});
    Launch none = list_of({{5, 1, 1, 2}, {7, 2, 1, 2}});
    none.masks.assign(none.masks.size(), 0);
    check("300 rows, pairs but no edge", 300, {}, {none});
    std::vector<Edge> e;
    for (uint32_t f = 0; f < 12; f++) {
        std::vector<Edge> c = clique(f * 25, f * 25 + 20 + f % 5, 0, 0);
        e.insert(e.end(), c.begin(), c.end());
    }
    for (uint32_t f = 1; f < 12; f++) e.push_back({f * 25, f * 25 - 25 + 3, 0, 0});      // one edge from each clique to the one before
    weigh(e, 1);
    check_list("300 rows, twelve cliques, a list", 300, e);
    Opts o;
    o.first_cap = 50;
    o.want_regrow = true;
    check("300 rows, twelve cliques, a list that is regrown and pairs no bit marks", 300, e, {list_of(e, true)}, o);
    check("300 rows, twelve cliques, flat", 300, e, {flat_rows(0, 300, e)});
}

static void case_clique()
{
    const uint32_t n = 40;
    std::vector<Edge> e = clique(0, n, 48, 64);
    // every fraction equal: the first link of all is (1, 0), then (2, 0) ...: one pair per round, n - 1 rounds and the one that finds nothing
    check_list("clique, all fractions equal: n - 1 merging rounds", n, e, rounds_and_clusters(n, 1));
    // the same without {39, 0}: the cliques {0 .. 38} and {1 .. 39} overlap; 0's side is merged first, 39 stays alone
    std::vector<Edge> f;
    for (const Edge &x : e)
        if (!(x.row == n - 1 && x.col == 0)) f.push_back(x);
    check_list("clique with one edge missing: the tie rule decides", n, f, rounds_and_clusters(n - 1, 2));
    // ... but with the edges of row 39 better, 39 merges first and row 0 is the one left out
    for (Edge &x : f)
        if (x.row == n - 1) { x.numer = 25; x.denom = 32; }
    check_list("clique with one edge missing, row 39's edges better", n, f, rounds_and_clusters(-1, 2));
}

static void case_path()
{
    const uint32_t n = 1000;
    std::vector<Edge> e;
    for (uint32_t i = 1; i < n; i++) e.push_back({i, i - 1, 32, 64});
    // pairs, never triples: (1, 0) first, then 2's best link (2, 1) is dead and (3, 2) is mutual, ...: n / 2 merging rounds
    check_list("path in index order, one weight", n, e, rounds_and_clusters(n / 2 + 1, n / 2));
    weigh(e, 3);
    check_list("path in index order, mixed weights", n, e);
    check("path in index order, mixed weights, flat", n, e, {flat_rows(0, n, e)});
}

static void case_joined()
{
    // two cliques joined by one edge, the best edge of all: its ends merge first and neither clique can follow them
    std::vector<Edge> e = clique(0, 30, 40, 64), b = clique(30, 70, 20, 32);
    e.insert(e.end(), b.begin(), b.end());
    e.push_back({30, 29, 63, 64});
    check_list("two cliques joined by their best edge", 70, e, rounds_and_clusters(-1, 3));
    e.back() = Edge{30, 29, 1, 64};                                             // ... by their worst: it never merges
    check_list("two cliques joined by their worst edge", 70, e, rounds_and_clusters(-1, 2));
}

static void case_both()
{
    // round one merges (1, 0) and (3, 2) at once; the link {2, 0} needs {2, 0}, {2, 1}, {3, 0} and {3, 1}: three lookups
    std::vector<Edge> four = {{1, 0, 7, 8}, {3, 2, 7, 8}, {2, 0, 1, 2}, {3, 0, 1, 2}, {2, 1, 1, 2}};
    check_list("both ends merge, one of the four links absent", 4, four, rounds_and_clusters(2, 2));
    four.push_back({3, 1, 1, 4});
    check_list("both ends merge, all four links there: the worst of them is the new weight", 4, four, rounds_and_clusters(3, 1));
    // the new weight decides the next round: {0, 1} - {2, 3} has dropped to 1/4 and ranks behind {4} - {0, 1} at 3/8, so 4 joins
    // {0, 1}; {2, 3} cannot follow, {4, 3} is no edge.  At the old 1/2 the four would have merged and left 4 alone
    four.push_back({4, 0, 3, 8});
    four.push_back({4, 1, 3, 8});
    four.push_back({4, 2, 3, 8});
    check_list("the dropped weight decides the next merge", 5, four, rounds_and_clusters(3, 2));
    // one end merges (a single lookup), over many waves: pairs (2 i + 1, 2 i) at 7/8, every row to row 0's pair at 1/2 except one
    std::vector<Edge> e;
    const uint32_t n = 600;
    for (uint32_t i = 0; i < n / 2; i++) e.push_back({2 * i + 1, 2 * i, 7, 8});
    for (uint32_t i = 2; i < n; i++) {
        e.push_back({i, 0, 1, 2});
        if (i != 77) e.push_back({i, 1, 1, 2});
    }
    check_list("pairs around one pair", n, e);
}

static void case_denoms()
{
    // equal fractions under three denominators rank by the ids alone: 1/2 = 2/4 = 32/64
    std::vector<Edge> e = {{3, 0, 1, 2}, {2, 1, 2, 4}, {3, 1, 32, 64}, {2, 0, 32, 64}, {1, 0, 2, 4}, {3, 2, 1, 2}, {4, 0, 31, 64}, {4, 3, 33, 64}, {5, 4, 0, 0}};
    check_list("1/2, 2/4 and 32/64", 6, e);
    std::vector<Edge> c = clique(0, 60, 0, 0);
    std::mt19937_64 rng(8);
    for (Edge &x : c) {
        x.denom = 1u << (1 + rng() % 6);
        x.numer = x.denom / 2 + (rng() % 3 == 0 ? x.denom / 4 : 0);
    }
    check_list("a clique of halves and three quarters under six denominators", 60, c);
    // denominators at the key's limit: neighbours that a 32-bit or a float key would merge
    const uint32_t top = FOREST_DENOM_LIMIT - 1;
    std::vector<Edge> t = {{1, 0, top - 2, top - 1}, {2, 0, top - 1, top}, {2, 1, top - 3, top - 2}, {3, 0, 1, top}, {3, 1, 1, top - 1}, {3, 2, 2, top}};
    check_list("denominators of 2^21 - 1", 4, t, rounds_and_clusters(-1, 1));
    std::vector<Edge> u = {{1, 0, top - 2, top - 1}, {2, 0, top - 1, top}, {3, 1, top - 3, top - 2}, {3, 2, top - 3, top - 2}};
    check_list("denominators of 2^21 - 1, a square", 4, u, rounds_and_clusters(-1, 2));
}

static std::vector<Edge> families(uint32_t n, uint32_t size, uint64_t seed, double keep = 0.9)
{
    // cliques of `size` consecutive rows with a tenth of their edges missing, and a chain of single edges between them
    std::mt19937_64 rng(seed);
    std::vector<Edge> e;
    for (uint32_t f = 0; f < n; f += size) {
        for (uint32_t r = f + 1; r < std::min(n, f + size); r++)
            for (uint32_t c = f; c < r; c++)
                if ((double)(rng() % 1000) < keep * 1000) e.push_back({r, c, 0, 0});
        if (f) e.push_back({f, f - 1 - (uint32_t)(rng() % size), 0, 0});
    }
    weigh(e, seed + 1);
    return e;
}

static void case_lists()
{
    const uint32_t n = 900;
    const std::vector<Edge> e = families(n, 30, 17);
    Opts o;
    o.first_cap = 1;
    o.want_regrow = true;
    check("a list regrown from a capacity of 1", n, e, {list_of(e)}, o);
    std::vector<Launch> blocks;
    for (auto rb : {std::make_pair(0u, 1u), std::make_pair(1u, 400u), std::make_pair(400u, 401u), std::make_pair(401u, n - 1), std::make_pair(n - 1, n)})
        blocks.push_back(flat_rows(rb.first, rb.second, e));
    check("five row blocks appended to one list", n, e, blocks);
    o.first_cap = 100;
    check("five row blocks, a list of 100 edges at first", n, e, blocks, o);
    std::vector<Edge> a(e.begin(), e.begin() + (long)(e.size() / 3)), b(e.begin() + (long)(e.size() / 3), e.end());
    o.first_cap = a.size();
    check("two lists, room for the first alone", n, e, {list_of(a, true), list_of(b)}, o);
    o.first_cap = e.size();
    o.want_regrow = false;
    check("one list, a capacity of exactly its edges", n, e, {list_of(e)}, o);
}

static void case_hash()
{
    const uint32_t n = 400;
    const std::vector<Edge> e = families(n, 20, 23);
    Opts o;
    o.hash_and = 0;
    check_list("every link hashes to slot 0: one long probe run", n, e, o);
    o.hash_or = ~0ull;
    check_list("every link hashes to the last slot: the run wraps round the table's end", n, e, o);
    o.hash_and = 7;
    o.hash_or = 0;
    check_list("eight home slots", n, e, o);
    o.hash_and = ~0ull;
    check_list("the hash as it is", n, e, o);
}

static void case_batches()
{
    // a clique of ten equal fractions: nine merging rounds, the tenth finds nothing.  Batches double from the first one's size
    const std::vector<Edge> e = clique(0, 10, 1, 2);
    const struct { uint32_t first; long batches; const char *what; } shapes[] = {
        {10, 1, "the fixpoint is the last round of the batch"}, {11, 1, "the fixpoint lies before the batch's end"},
        {9, 2, "the fixpoint is the first round of the next batch"}, {1, 4, "batches of 1, 2, 4, 8"}, {3, 3, "batches of 3, 6, 12"},
        {256, 1, "one batch of 256"}};
    for (const auto &s : shapes) {
        Opts o = rounds_and_clusters(10, 1);
        o.first_batch = s.first;
        o.want_batches = s.batches;
        check_list(s.what, 10, e, o);
    }
    const std::vector<Edge> f = families(700, 35, 29, 1.0);                    // full cliques of mixed weights, many rounds
    for (uint32_t first : {1u, 2u, 8u}) {
        Opts o;
        o.first_batch = first;
        check_list(("cliques of 35, a first batch of " + std::to_string(first)).c_str(), 700, f, o);
    }
}

static void fuzz(uint64_t seed, int jobs)
{
    std::mt19937_64 rng(seed);
    for (int j = 0; j < jobs; j++) {
        const uint32_t n = 2 + (uint32_t)(rng() % (j % 5 == 0 ? 3000 : 800));
        const uint32_t size = 2 + (uint32_t)(rng() % 40);                       // rows of a family; edges inside families and a few between
        const double keep = 1.0 - (double)(rng() % 4) * 0.15;
        const uint32_t values = 1 + (uint32_t)(rng() % 16);
        std::vector<Edge> e;
        for (uint32_t f = 0; f < n; f += size)
            for (uint32_t r = f + 1; r < std::min(n, f + size); r++)
                for (uint32_t c = f; c < r; c++)
                    if ((double)(rng() % 1000) < keep * 1000) e.push_back({r, c, 0, 0});
        std::set<std::pair<uint32_t, uint32_t>> have;
        for (const Edge &x : e) have.insert({x.row, x.col});
        for (uint32_t k = 0; k < n / 4; k++) {
            const uint32_t a = 1 + (uint32_t)(rng() % (n - 1)), b = (uint32_t)(rng() % a);
            if (have.insert({a, b}).second) e.push_back({a, b, 0, 0});
        }
        for (Edge &x : e) {
            x.denom = 16u << (rng() % 3);
            x.numer = (uint32_t)(1 + rng() % values) * (x.denom / 16);
        }
        std::shuffle(e.begin(), e.end(), rng);
        std::vector<Launch> v;
        if (rng() % 2 && n <= 1500) {
            uint32_t r = 0;
            while (r < n) {
                const uint32_t r2 = std::min<uint32_t>(n, r + 1 + (uint32_t)(rng() % n));
                v.push_back(flat_rows(r, r2, e));
                r = r2;
            }
        } else {
            const size_t parts = 1 + rng() % 3;
            for (size_t p = 0; p < parts; p++)
                v.push_back(list_of(std::vector<Edge>(e.begin() + (long)(e.size() * p / parts), e.begin() + (long)(e.size() * (p + 1) / parts)), rng() % 2));
        }
        Opts o;
        o.first_cap = rng() % 3 ? 0 : 1 + rng() % 5000;                      // every third job starts with a short list
        o.first_batch = 1 + (uint32_t)(rng() % 8);
        if (j % 4 == 0) o.hash_and = 0xF;                                    // every fourth with sixteen home slots
        check(("fuzz " + std::to_string(j)).c_str(), n, e, v, o);
    }
}

int main(int argc, char **argv)
{
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "small") case_small();
    else if (c == "clique") case_clique();
    else if (c == "path") case_path();
    else if (c == "joined") case_joined();
    else if (c == "both") case_both();
    else if (c == "denoms") case_denoms();
    else if (c == "lists") case_lists();
    else if (c == "hash") case_hash();
    else if (c == "batches") case_batches();
    else if (c == "fuzz" && argc > 3) fuzz(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
    else { fprintf(stderr, "usage: complete_emu small|clique|path|joined|both|denoms|lists|hash|batches | fuzz <seed> <n>\n"); return 2; }
    if (failures) { printf("%d case(s) FAILED\n", failures); return 1; }
    printf("all cases agree\n");
    return 0;
}
