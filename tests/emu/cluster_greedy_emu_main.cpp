// cluster_greedy_emu_main.cpp -- runs mash_amd/csrc/cluster_greedy.hip, unchanged, through its launchers (cg_append_kernel over
// ballot words in list mode and in flat triangle mode, the rounds, cg_rep_init_kernel and cg_assign_kernel) on the CPU
// (tools/hipemu) and compares rep and the number of clusters with the sequential walk over the same edges.  The driver below
// does what cluster_greedy_tri does on the host: append per launch, regrow and append again when the list overflows, rounds
// in batches until one leaves no row open, the assignment.
// TEST INFRASTRUCTURE (tests/test_cluster_greedy_emu.py); built with g++.  The emulator runs workgroups one after another: what
// is pinned here is the arithmetic (word / bit / pair indices, the places in the list, the states, the rounds), not the races
// between workgroups.
//
//   cluster_greedy_emu <case>            cases: path band star clique density blocks overflow small
//   cluster_greedy_emu fuzz <seed> <n>   n random jobs
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <cmath>
#include <random>
#include <string>
#include <vector>

#include "../../mash_amd/csrc/cluster_greedy.hip"

using namespace mg;

typedef std::pair<uint32_t, uint32_t> Edge;      // {row, col}

// one append launch: a list of pairs with a mask, or rows [first_row, row_end) of the flat triangle with a mask
struct Launch {
    std::vector<uint2> rc;                       // list mode (empty: flat)
    uint64_t first_row = 0, pairs = 0;
    std::vector<unsigned long long> masks;
    void set(uint64_t idx) { masks[idx >> 6] |= 1ull << (idx & 63); }
    bool get(uint64_t idx) const { return (masks[idx >> 6] >> (idx & 63)) & 1ull; }
};

static uint64_t tri(uint64_t r) { return r ? r * (r - 1) / 2 : 0; }

static Launch list_launch(const std::vector<Edge> &pairs)
{
    Launch L;
    for (const Edge &e : pairs) L.rc.push_back(make_uint2(e.first, e.second));
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
    return L;
}

static void flat_set(Launch &L, uint32_t row, uint32_t col) { L.set(tri(row) + col - tri(L.first_row)); }

// the edges a launch stands for, by the definition of the layouts (not by pair_rc)
static void edges_of(const Launch &L, std::vector<Edge> &out)
{
    if (!L.rc.empty()) {
        for (uint64_t i = 0; i < L.pairs; i++)
            if (L.get(i)) out.push_back({L.rc[i].x, L.rc[i].y});
        return;
    }
    uint64_t row = L.first_row, col = 0;
    if (row == 0) row = 1;
    for (uint64_t i = 0; i < L.pairs; i++) {
        if (L.get(i)) out.push_back({(uint32_t)row, (uint32_t)col});
        if (++col == row) { row++; col = 0; }
    }
}

static int failures = 0;
constexpr uint32_t GUARD = 0xDEADBEEFu;

// first_cap: the first capacity of the edge list (0: room for everything); min_rounds / want_regrow: what the case is there for
static void check(const char *name, uint32_t n, const std::vector<Launch> &launches, uint64_t first_cap = 0, uint64_t min_rounds = 0, bool want_regrow = false)
{
    // the definition: the sequential walk in index order
    std::vector<Edge> edges;
    for (const Launch &L : launches) edges_of(L, edges);
    std::vector<std::vector<uint32_t>> smaller(n);
    for (const Edge &e : edges)
        if (e.first != e.second) smaller[std::max(e.first, e.second)].push_back(std::min(e.first, e.second));
    std::vector<uint32_t> want(n);
    uint64_t want_reps = 0;
    for (uint32_t i = 0; i < n; i++) {
        want[i] = i;
        for (uint32_t j : smaller[i])
            if (want[j] == j && (want[i] == i || j < want[i])) want[i] = j;
        want_reps += want[i] == i;
    }

    bool ok = true;
    uint64_t cap = first_cap ? first_cap : std::max<uint64_t>(edges.size(), 1), used = 0, regrows = 0;
    std::vector<uint2> list(cap + 1, make_uint2(GUARD, GUARD));
    unsigned long long cursor = 0;
    uint32_t overflow = 0;
    for (const Launch &L : launches) {
        FinishArgs a{};
        a.pairs = L.pairs;
        a.first_row = L.first_row;
        a.triangle = 1;
        a.masks = const_cast<unsigned long long *>(L.masks.data());
        a.list_rc = L.rc.empty() ? nullptr : L.rc.data();
        std::vector<Edge> mine;
        edges_of(L, mine);
        for (int attempt = 0;; attempt++) {
            ok = ok && launch_greedy_append(a, n, list.data(), cap, &cursor, &overflow, nullptr) == hipSuccess;
            ok = ok && list[cap].x == GUARD && list[cap].y == GUARD;              // never a word behind the list
            ok = ok && cursor == used + mine.size() && (overflow != 0) == (cursor > cap);
            if (cursor <= cap) break;
            if (attempt) { ok = false; break; }
            const uint64_t bigger = std::max<uint64_t>(cursor, 2 * cap);          // regrow: the earlier launches' edges move over
            std::vector<uint2> nl(bigger + 1, make_uint2(GUARD, GUARD));
            std::copy(list.begin(), list.begin() + (long)used, nl.begin());
            list.swap(nl);
            cap = bigger;
            cursor = used;
            overflow = 0;
            regrows++;
        }
        // what this launch appended is its edges, in some order
        std::vector<Edge> got;
        for (uint64_t i = used; i < cursor && i < cap; i++) got.push_back({list[i].x, list[i].y});
        for (Edge &e : mine) e = {std::max(e.first, e.second), std::min(e.first, e.second)};
        std::sort(got.begin(), got.end());
        std::sort(mine.begin(), mine.end());
        ok = ok && got == mine;
        used = cursor;
    }

    std::vector<uint32_t> state(n + 1, 0), rep(n + 1, GUARD), left(257, GUARD);
    state[n] = GUARD;
    uint64_t rounds = 0, batches = 0;
    bool done = n == 0;
    for (uint32_t batch = 8; !done; batch = std::min(batch * 2, 256u)) {
        ok = ok && launch_greedy_rounds(list.data(), used, state.data(), n, left.data(), batch, nullptr) == hipSuccess;
        ok = ok && left[batch] == GUARD;
        batches++;
        uint32_t r = 0;
        while (r < batch && left[r]) r++;
        rounds += std::min(r + 1, batch);
        for (uint32_t k = r + 1; k < batch; k++) ok = ok && left[k] == 0;           // rounds behind the fixpoint do nothing
        done = r < batch;
        if (rounds > n) { ok = false; break; }                                      // at most n rounds, ever
    }
    for (uint32_t i = 0; i < n; i++) ok = ok && (state[i] == 2 || state[i] == 3);
    unsigned long long reps = ~0ull;
    ok = ok && launch_greedy_assign(list.data(), used, state.data(), n, rep.data(), &reps, nullptr) == hipSuccess;
    ok = ok && state[n] == GUARD && rep[n] == GUARD && list[cap].x == GUARD;        // nothing written behind the arrays
    if (n == 0) ok = ok && reps == 0;
    uint64_t bad = 0;
    for (uint32_t i = 0; i < n; i++) bad += rep[i] != want[i];
    const bool shaped = rounds >= min_rounds && rounds <= std::max<uint64_t>(n, 0) && (!want_regrow || regrows > 0);
    if (!ok || bad || (n && reps != want_reps) || !shaped) {
        failures++;
        printf("FAIL %s: n %u edges %zu: %llu reps differ, clusters %llu want %llu, rounds %llu (want >= %llu, <= n), regrows %llu%s\n", name, n,
               edges.size(), (unsigned long long)bad, reps, (unsigned long long)want_reps, (unsigned long long)rounds, (unsigned long long)min_rounds,
               (unsigned long long)regrows, ok ? "" : " (launch, guard word or list content)");
    } else {
        printf("ok   %s: n %u edges %zu clusters %llu rounds %llu batches %llu regrows %llu\n", name, n, edges.size(), (unsigned long long)want_reps,
               (unsigned long long)rounds, (unsigned long long)batches, (unsigned long long)regrows);
    }
}

static void case_path()
{
    const uint32_t n = 3000;
    std::vector<Edge> e;
    for (uint32_t i = 1; i < n; i++) e.push_back({i, i - 1});
    // reps 0, 2, 4, ...: row i cannot be decided before row i - 1, a round decides two rows (a rep in part B, its successor in
    // the next part A) -- the deepest chain there is, n / 2 rounds of the n allowed
    check("path in index order, list", n, {list_all(e)}, 0, n / 2);
    Launch F = flat_launch(0, n);
    for (uint32_t i = 1; i < n; i++) flat_set(F, i, i - 1);
    check("path in index order, flat", n, {F}, 0, n / 2);
    std::vector<uint32_t> perm(n);
    for (uint32_t i = 0; i < n; i++) perm[i] = i;
    std::mt19937_64 rng(3);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<Edge> s;
    for (uint32_t i = 1; i < n; i++) s.push_back({std::max(perm[i], perm[i - 1]), std::min(perm[i], perm[i - 1])});
    std::shuffle(s.begin(), s.end(), rng);
    check("path over shuffled rows, list", n, {list_all(s)});
}

static void case_band()
{
    const uint32_t n = 2500;
    for (uint32_t w : {2u, 5u, 17u}) {                                           // row i beside rows i - 1 .. i - w: reps every w + 1 rows
        Launch F = flat_launch(0, n);
        for (uint32_t i = 1; i < n; i++)
            for (uint32_t k = 1; k <= w && k <= i; k++) flat_set(F, i, i - k);
        check(("band of width " + std::to_string(w) + ", flat").c_str(), n, {F}, 0, n / (w + 1) - 1);
    }
}

static void case_star()
{
    const uint32_t n = 3000, c = 1234;
    std::vector<Edge> z;
    for (uint32_t i = 1; i < n; i++) z.push_back({i, 0});
    check("star around 0, list", n, {list_all(z)});                             // one cluster
    std::vector<Edge> e;
    for (uint32_t i = n; i-- > 0;)
        if (i != c) e.push_back({std::max(i, c), std::min(i, c)});
    // rows below 1234 have no smaller neighbour: they are representatives, 1234 joins row 0, rows above it have lost their centre
    check("star around 1234, list", n, {list_all(e)});
    Launch F = flat_launch(0, n);
    for (const Edge &x : e) flat_set(F, x.first, x.second);
    check("star around 1234, flat", n, {F});
}

static void case_clique()
{
    const uint32_t n = 1500;                                                    // 1 124 250 pairs: not a multiple of 64
    Launch F = flat_launch(0, n);
    for (uint64_t i = 0; i < F.pairs; i++) F.set(i);
    check("clique of 1500, flat order", n, {F});
}

static void case_density()
{
    const uint32_t n = 4000;
    std::mt19937_64 rng(11);
    std::vector<Edge> e;
    for (uint32_t w = 0; w < 65 * 5; w++)
        for (int b = 0; b < 64; b++) {
            const uint32_t a = 1 + (uint32_t)(rng() % (n - 1));
            e.push_back({a, (uint32_t)(rng() % a)});
        }
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
    check("mask words of every density, flat", 700, {F});
    for (uint32_t K : {1u, 37u, 63u, 64u, 65u, 4097u}) {                         // lists whose length is not a multiple of 64
        std::vector<Edge> q;
        for (uint32_t i = 0; i < K; i++) {
            const uint32_t a = 1 + (uint32_t)(rng() % 899);
            q.push_back({a, (uint32_t)(rng() % a)});
        }
        Launch Q = list_launch(q);
        for (uint32_t i = 0; i < K; i++)
            if (rng() % 100 < 40 || i + 1 == K) Q.set(i);
        check(("list of " + std::to_string(K) + " pairs").c_str(), 900, {Q});
    }
}

static std::vector<Launch> five_blocks(uint32_t n, uint64_t seed)
{
    // row blocks of one triangle over one list and one state array; seven families by residue, chains inside them
    std::mt19937_64 rng(seed);
    std::vector<Launch> v;
    for (auto rb : {std::make_pair(0u, 1u), std::make_pair(1u, 700u), std::make_pair(700u, 701u), std::make_pair(701u, n - 1), std::make_pair(n - 1, n)}) {
        Launch F = flat_launch(rb.first, rb.second);
        for (uint32_t r = std::max(rb.first, 1u); r < rb.second; r++)
            for (int k = 0; k < 3; k++) {
                const uint32_t c = (uint32_t)(rng() % r);
                if ((r % 7) == (c % 7)) flat_set(F, r, c);
            }
        if (rb.second == n) { flat_set(F, n - 1, 3); flat_set(F, n - 1, 4); flat_set(F, n - 1, n - 2); }
        v.push_back(F);
    }
    return v;
}

static void case_blocks() { check("five row blocks, one list", 1500, five_blocks(1500, 17)); }

static void case_overflow()
{
    check("five row blocks, a list of 1 edge at first", 1500, five_blocks(1500, 19), 1, 0, true);
    check("five row blocks, a list of 100 edges at first", 1500, five_blocks(1500, 23), 100, 0, true);
    const uint32_t n = 900;
    std::vector<Edge> e;
    for (uint32_t i = 1; i < n; i++) { e.push_back({i, i / 2}); e.push_back({i, i - 1}); }
    check("one list, a capacity inside a word", n, {list_all(e)}, 70, 0, true);
    check("one list, a capacity of exactly its edges", n, {list_all(e)}, e.size(), 0, false);
    check("one list, a capacity one short", n, {list_all(e)}, e.size() - 1, 0, true);
}

static void case_small()                                                     // (also the ThreadSanitizer build's case)
{
    check("no rows", 0, {});
    check("one row", 1, {});
    check("no edge", 300, {list_launch({{5, 1}, {7, 2}})});
    std::vector<Edge> e;
    for (uint32_t i = 299; i >= 1; i--) e.push_back({i, (i * 7) % i});
    for (uint32_t i = 1; i < 300; i++) e.push_back({i, i / 2});
    check("300 rows, a list", 300, {list_all(e)});
    check("300 rows, a list that is regrown", 300, {list_all(e)}, 50, 0, true);
    Launch F = flat_launch(0, 100);
    for (uint64_t i = 0; i < F.pairs; i += 3) F.set(i);
    check("100 rows, flat", 100, {F});
}

static void fuzz(uint64_t seed, int jobs)
{
    std::mt19937_64 rng(seed);
    for (int j = 0; j < jobs; j++) {
        const uint32_t n = 2 + (uint32_t)(rng() % (j % 5 == 0 ? 20000 : 1500));
        std::vector<Launch> v;
        const int nl = 1 + (int)(rng() % 3);
        const bool flat = rng() % 2;
        const double dens = std::pow(10.0, -(double)(rng() % 5));           // 1 .. 1e-4
        const uint32_t fam = 1 + (uint32_t)(rng() % 40);                     // edges only inside residue classes
        if (flat && n <= 3000) {
            uint32_t r = 0;
            for (int l = 0; l < nl; l++) {
                const uint32_t r2 = l + 1 == nl ? n : std::min<uint32_t>(n, r + 1 + (uint32_t)(rng() % n));
                Launch F = flat_launch(r, r2);
                uint64_t row = std::max<uint64_t>(r, 1), col = 0;
                for (uint64_t i = 0; i < F.pairs; i++) {
                    if (row % fam == col % fam && (double)(rng() % 1000000) < dens * 1e6) F.set(i);
                    if (++col == row) { row++; col = 0; }
                }
                v.push_back(F);
                r = r2;
                if (r >= n) break;
            }
        } else {
            for (int l = 0; l < nl; l++) {
                const uint64_t K = rng() % 60000;
                std::vector<Edge> e;
                for (uint64_t i = 0; i < K; i++) {
                    const uint32_t a = 1 + (uint32_t)(rng() % (n - 1));
                    uint32_t b = (uint32_t)(rng() % a);
                    b -= std::min(b, (b % fam + fam - a % fam) % fam);
                    if (rng() % 2) e.push_back({a, b}); else e.push_back({b, a});   // a list names a pair either way round
                }
                Launch L = list_launch(e);
                for (uint64_t i = 0; i < K; i++)
                    if (e[i].first != e[i].second && e[i].first % fam == e[i].second % fam && (double)(rng() % 1000000) < dens * 1e6) L.set(i);
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
    if (c == "path") case_path();
    else if (c == "band") case_band();
    else if (c == "star") case_star();
    else if (c == "clique") case_clique();
    else if (c == "density") case_density();
    else if (c == "blocks") case_blocks();
    else if (c == "overflow") case_overflow();
    else if (c == "small") case_small();
    else if (c == "fuzz" && argc > 3) fuzz(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
    else { fprintf(stderr, "usage: cluster_greedy_emu path|band|star|clique|density|blocks|overflow|small | fuzz <seed> <n>\n"); return 2; }
    if (failures) { printf("%d case(s) FAILED\n", failures); return 1; }
    printf("all cases agree\n");
    return 0;
}
