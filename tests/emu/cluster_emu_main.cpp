// cluster_emu_main.cpp -- runs mash_amd/csrc/cluster.hip, unchanged, through its launchers (cl_init_kernel, cl_union_kernel over
// ballot words in list mode and in flat triangle mode, cl_label_kernel) on the CPU (tools/hipemu) and compares labels and the
// number of clusters with a sequential union-find over the same edges.
// TEST INFRASTRUCTURE (tests/test_cluster_emu.py); built with g++.  The emulator runs workgroups one after another: what is
// pinned here is the arithmetic (word / bit / pair indices, pair_rc, the walks, the links), not the races between workgroups.
//
//   cluster_emu <case>            cases: path star clique bridge density ragged blocks small
//   cluster_emu fuzz <seed> <n>   n random jobs
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <cmath>
#include <random>
#include <string>
#include <vector>

#include "../../mash_amd/csrc/cluster.hip"

using namespace mg;

typedef std::pair<uint32_t, uint32_t> Edge;      // {row, col}

// one union launch: a list of pairs with a mask, or rows [first_row, row_end) of the flat triangle with a mask
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

static void check(const char *name, uint32_t n, const std::vector<Launch> &launches)
{
    // the definition: components by a sequential union-find, label = smallest member
    std::vector<uint32_t> p(n);
    for (uint32_t i = 0; i < n; i++) p[i] = i;
    auto find = [&](uint32_t x) { while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; } return x; };
    std::vector<Edge> edges;
    for (const Launch &L : launches) edges_of(L, edges);
    for (const Edge &e : edges) {
        const uint32_t a = find(e.first), b = find(e.second);
        if (a != b) p[std::max(a, b)] = std::min(a, b);
    }
    std::vector<uint32_t> want(n);
    uint64_t want_roots = 0;
    for (uint32_t i = 0; i < n; i++) { want[i] = find(i); want_roots += want[i] == i; }

    std::vector<uint32_t> parent(n + 1, 0xDEADBEEFu), label(n + 1, 0xDEADBEEFu);
    unsigned long long roots = ~0ull;
    bool ok = launch_cluster_init(parent.data(), n, nullptr) == hipSuccess;
    for (const Launch &L : launches) {
        FinishArgs a{};
        a.pairs = L.pairs;
        a.first_row = L.first_row;
        a.triangle = 1;
        a.masks = const_cast<unsigned long long *>(L.masks.data());
        a.list_rc = L.rc.empty() ? nullptr : L.rc.data();
        ok = ok && launch_cluster_union(a, parent.data(), n, nullptr) == hipSuccess;
        for (uint32_t i = 0; i < n; i++) ok = ok && parent[i] <= i;
    }
    ok = ok && launch_cluster_label(parent.data(), n, label.data(), &roots, nullptr) == hipSuccess;
    ok = ok && parent[n] == 0xDEADBEEFu && label[n] == 0xDEADBEEFu;          // nothing written behind the rows
    uint64_t bad = 0;
    for (uint32_t i = 0; i < n; i++) bad += label[i] != want[i];
    if (!ok || bad || roots != want_roots) {
        failures++;
        printf("FAIL %s: n %u edges %zu: %llu labels differ, clusters %llu want %llu%s\n", name, n, edges.size(), (unsigned long long)bad, roots,
               (unsigned long long)want_roots, ok ? "" : " (launch or invariant)");
    } else {
        printf("ok   %s: n %u edges %zu clusters %llu\n", name, n, edges.size(), roots);
    }
}

static Launch list_all(const std::vector<Edge> &e)
{
    Launch L = list_launch(e);
    for (uint64_t i = 0; i < L.pairs; i++) L.set(i);
    return L;
}

static void case_path()
{
    const uint32_t n = 5000;
    std::vector<Edge> e;
    for (uint32_t i = n - 1; i >= 1; i--) e.push_back({i, i - 1});           // descending: every link hangs a root under a root
    check("path, list, descending", n, {list_all(e)});
    std::reverse(e.begin(), e.end());
    check("path, list, ascending", n, {list_all(e)});
    Launch F = flat_launch(0, n);
    for (uint32_t i = 1; i < n; i++) flat_set(F, i, i - 1);
    check("path, flat", n, {F});
}

static void case_star()
{
    const uint32_t n = 3000, c = 1234;
    std::vector<Edge> e;
    for (uint32_t i = n; i-- > 0;)
        if (i != c) e.push_back({std::max(i, c), std::min(i, c)});
    check("star around 1234, list", n, {list_all(e)});
    Launch F = flat_launch(0, n);
    for (const Edge &x : e) flat_set(F, x.first, x.second);
    check("star around 1234, flat", n, {F});
    std::vector<Edge> z;
    for (uint32_t i = 1; i < n; i++) z.push_back({i, 0});
    check("star around 0, list", n, {list_all(z)});
}

static void case_clique()
{
    const uint32_t n = 2000;
    Launch F = flat_launch(0, n);
    for (uint64_t i = 0; i < F.pairs; i++) F.set(i);
    check("clique of 2000, flat order", n, {F});
}

static void case_bridge()
{
    const uint32_t n = 6001;                                                 // two components of 3000 rows, interleaved; row 6000 alone
    std::mt19937_64 rng(7);
    std::vector<Edge> e;
    for (uint32_t i = 2; i < 6000; i++) {
        const uint32_t j = i % 2 + 2 * (uint32_t)(rng() % (i / 2));        // an earlier row of the same parity
        e.push_back({i, j});
    }
    for (int k = 0; k < 20000; k++) {
        uint32_t a = (uint32_t)(rng() % 6000), b = (uint32_t)(rng() % 6000);
        if (a == b || (a ^ b) & 1) continue;
        e.push_back({std::max(a, b), std::min(a, b)});
    }
    check("two components, no bridge", n, {list_all(e)});
    e.push_back({5999, 5998});
    check("two components joined by the last edge", n, {list_all(e)});
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
    for (uint32_t w = 0; w < 65 * 5; w++) {                                  // word w carries w % 65 bits, 0 .. 64
        std::vector<int> bits(64);
        for (int b = 0; b < 64; b++) bits[b] = b;
        std::shuffle(bits.begin(), bits.end(), rng);
        for (uint32_t k = 0; k < w % 65; k++) L.set((uint64_t)w * 64 + bits[k]);
    }
    check("mask words of every density, list", n, {L});
    Launch F = flat_launch(0, 700);                                          // 244 650 pairs
    for (uint64_t w = 0; w < F.masks.size(); w++) {
        const uint64_t left = F.pairs - w * 64;
        unsigned long long m = 0;
        for (uint32_t k = 0; k < (w * 7) % 65; k++) m |= 1ull << (rng() % 64);
        if (w % 3) m = w % 5 ? 0 : m & rng() & rng() & rng();
        F.masks[w] = left >= 64 ? m : m & ((1ull << left) - 1);
    }
    check("mask words of every density, flat", 700, {F});
}

static void case_ragged()
{
    std::mt19937_64 rng(13);
    for (uint32_t K : {1u, 37u, 63u, 64u, 65u, 1037u, 4097u, 70001u}) {
        const uint32_t n = 900;
        std::vector<Edge> e;
        for (uint32_t i = 0; i < K; i++) {
            const uint32_t a = 1 + (uint32_t)(rng() % (n - 1));
            e.push_back({a, (uint32_t)(rng() % a)});
        }
        Launch L = list_launch(e);
        for (uint32_t i = 0; i < K; i++)
            if (rng() % 100 < (K > 5000 ? 1 : 40) || i + 1 == K) L.set(i);
        check(("list of " + std::to_string(K) + " pairs").c_str(), n, {L});
    }
    for (uint32_t rows : {2u, 3u, 12u, 13u, 129u}) {
        Launch F = flat_launch(0, rows);
        for (uint64_t i = 0; i < F.pairs; i++)
            if (i % 3 != 1) F.set(i);
        check(("flat triangle of " + std::to_string(rows) + " rows").c_str(), rows, {F});
    }
}

static void case_blocks()
{
    // row blocks of one triangle, `parent` persistent across them; a component that only closes in the last block
    const uint32_t n = 1500;
    std::mt19937_64 rng(17);
    std::vector<Launch> v;
    for (auto rb : {std::make_pair(0u, 1u), std::make_pair(1u, 700u), std::make_pair(700u, 701u), std::make_pair(701u, 1499u), std::make_pair(1499u, 1500u)}) {
        Launch F = flat_launch(rb.first, rb.second);
        for (uint32_t r = std::max(rb.first, 1u); r < rb.second; r++)
            for (int k = 0; k < 2; k++) {
                const uint32_t c = (uint32_t)(rng() % r);
                if ((r % 7) == (c % 7) && r != 1499) flat_set(F, r, c);      // seven families by residue
            }
        if (rb.second == 1500) { flat_set(F, 1499, 3); flat_set(F, 1499, 4); flat_set(F, 1499, 1498); }
        v.push_back(F);
    }
    check("five row blocks, one parent", n, v);
}

static void case_small()                                                     // (also the ThreadSanitizer build's case)
{
    check("no rows", 0, {});
    check("one row", 1, {});
    check("no edge", 300, {list_launch({{5, 1}, {7, 2}})});
    std::vector<Edge> e;
    for (uint32_t i = 299; i >= 1; i--) e.push_back({i, (i * 7) % i});
    for (uint32_t i = 1; i < 300; i++) e.push_back({i, i / 2});
    Launch L = list_all(e);
    check("300 rows, a list", 300, {L});
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
                    e.push_back({a, b});
                }
                Launch L = list_launch(e);
                for (uint64_t i = 0; i < K; i++)
                    if (e[i].first % fam == e[i].second % fam && (double)(rng() % 1000000) < dens * 1e6) L.set(i);
                v.push_back(L);
            }
        }
        check(("fuzz " + std::to_string(j)).c_str(), n, v);
    }
}

int main(int argc, char **argv)
{
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "path") case_path();
    else if (c == "star") case_star();
    else if (c == "clique") case_clique();
    else if (c == "bridge") case_bridge();
    else if (c == "density") case_density();
    else if (c == "ragged") case_ragged();
    else if (c == "blocks") case_blocks();
    else if (c == "small") case_small();
    else if (c == "fuzz" && argc > 3) fuzz(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
    else { fprintf(stderr, "usage: cluster_emu path|star|clique|bridge|density|ragged|blocks|small | fuzz <seed> <n>\n"); return 2; }
    if (failures) { printf("%d case(s) FAILED\n", failures); return 1; }
    printf("all cases agree\n");
    return 0;
}
