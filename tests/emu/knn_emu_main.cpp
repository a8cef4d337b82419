// knn_emu_main.cpp -- runs the mirror of mash_amd/csrc/knn.hip (degree pass, scan, scatter) and the keyed selection of topk.hip
// (launch_topk_select_keyed: both kernels) through their launch functions on host fibers (tools/hipemu) and compares every row's
// list with a std::stable_sort statement of the definition of `mash triangle -N`: the eligible pairs that contain the row, best
// first by the exact fraction (compared in 128-bit integers here, so the check does not share the kernel's arithmetic), equal
// fractions by ascending neighbour, the first k.  The scatter's order inside a segment is unspecified, so every job is also run
// with its list entries in a shuffled order: the answer must be the same.
// TEST INFRASTRUCTURE (tests/test_knn_emu.py); built with g++.
//
//   knn_emu <case>            cases: equal straddle ends degrees bits
//   knn_emu fuzz <seed> <n>   n random jobs
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../../mash_amd/csrc/topk.hip"
#include "../../mash_amd/csrc/knn.hip"

using namespace mg;

struct Entry { uint32_t row, col, numer, denom; bool on; };     // col < row

struct Job {
    uint32_t n = 0;
    std::vector<Entry> list;                                   // reference order: rows ascending, a row's columns ascending
};

struct Nb { uint32_t nbr, numer, denom; };

// the definition
static std::vector<std::vector<Nb>> expected(const Job &j, uint32_t k)
{
    std::vector<std::vector<Nb>> rows(j.n);
    for (const Entry &e : j.list)
        if (e.on) {
            rows[e.row].push_back({e.col, e.numer, e.denom});
            rows[e.col].push_back({e.row, e.numer, e.denom});
        }
    for (auto &v : rows) {
        std::sort(v.begin(), v.end(), [](const Nb &a, const Nb &b) { return a.nbr < b.nbr; });
        std::stable_sort(v.begin(), v.end(), [](const Nb &a, const Nb &b) {
            const unsigned __int128 l = (unsigned __int128)a.numer * (b.denom ? b.denom : 1u), r = (unsigned __int128)b.numer * (a.denom ? a.denom : 1u);
            return l > r;
        });
        if (v.size() > k) v.resize(k);
    }
    return rows;
}

static int failures = 0;

static void fail(const char *what, uint32_t k, const char *order, const std::string &msg)
{
    if (failures < 12) printf("%s k=%u (%s order): %s\n", what, k, order, msg.c_str());
    failures++;
}

static void run(const Job &j, const std::vector<Entry> &list, uint32_t k, const char *what, const char *order)
{
    const uint64_t K = list.size();
    std::vector<uint2> rc(K + 1), cnt(K + 1);
    std::vector<unsigned long long> masks(K / 64 + 2, 0);
    uint64_t eligible = 0;
    for (uint64_t i = 0; i < K; i++) {
        rc[i] = make_uint2(list[i].row, list[i].col);
        cnt[i] = make_uint2(list[i].numer, list[i].denom);
        if (list[i].on) { masks[i >> 6] |= 1ull << (i & 63); eligible++; }
    }
    const uint32_t GUARD = 0xDEADBEEFu;
    std::vector<uint32_t> deg((size_t)j.n + 2, GUARD), base((size_t)j.n + 2, GUARD), cur((size_t)j.n + 1, GUARD), bsum(knn_scan_blocks(j.n) + 1, GUARD);
    std::vector<uint2> sym_counts(2 * eligible + 1, make_uint2(GUARD, GUARD));
    std::vector<uint32_t> sym_nbr(2 * eligible + 1, GUARD);
    KnnMirror m{};
    m.rc = rc.data();
    m.cnt = cnt.data();
    m.masks = masks.data();
    m.K = K;
    m.n = j.n;
    m.deg = deg.data();
    m.base = base.data();
    m.cur = cur.data();
    m.block_sum = bsum.data();
    m.sym_counts = sym_counts.data();
    m.sym_nbr = sym_nbr.data();
    if (launch_knn_degree(m, nullptr) != hipSuccess || launch_knn_scan(m, nullptr) != hipSuccess || launch_knn_scatter(m, nullptr) != hipSuccess) {
        fail(what, k, order, "a mirror launch was refused");
        return;
    }
    // the mirror: degrees, offsets, nothing written past its arrays, every segment full
    const std::vector<std::vector<Nb>> all = expected(j, 0xFFFFFFFFu);
    uint32_t at = 0;
    for (uint32_t r = 0; r < j.n; r++) {
        if (deg[r] != all[r].size() || base[r] != at || cur[r] != deg[r]) { fail(what, k, order, "degree / offset / cursor of row " + std::to_string(r)); return; }
        at += deg[r];
    }
    if (deg[j.n] != 0 || base[j.n] != 2 * eligible || deg[j.n + 1] != GUARD || base[j.n + 1] != GUARD || cur[j.n] != GUARD || bsum.back() != GUARD ||
        sym_nbr[2 * eligible] != GUARD || sym_counts[2 * eligible].x != GUARD) {
        fail(what, k, order, "the mirror's ends");
        return;
    }
    for (uint64_t i = 0; i < 2 * eligible; i++)
        if (sym_nbr[i] == GUARD) { fail(what, k, order, "a place of a segment was never written"); return; }
    // the selection
    std::vector<uint32_t> sel((size_t)j.n * k, GUARD), row_n(j.n, GUARD), seen(1u << 17, 0), want_seen(1u << 17, 0);
    TopkArgs a{};
    a.counts = sym_counts.data();
    a.seg_base = base.data();
    a.seg_cnt = deg.data();
    a.nrows = j.n;
    a.k = k;
    a.sel = sel.data();
    a.row_n = row_n.data();
    a.denom_seen = seen.data();
    a.s = (uint32_t)seen.size() - 1;
    a.key = sym_nbr.data();
    if (launch_topk_select_keyed(a, nullptr) != hipSuccess) { fail(what, k, order, "the selection was refused"); return; }
    const std::vector<std::vector<Nb>> want = expected(j, k);
    for (uint32_t r = 0; r < j.n; r++) {
        const std::vector<Nb> &e = want[r];
        bool ok = row_n[r] == e.size();
        for (size_t i = 0; ok && i < e.size(); i++) {
            const uint32_t x = sel[(size_t)r * k + i];
            ok = x >= base[r] && x < base[r] + deg[r] && sym_nbr[x] == e[i].nbr && sym_counts[x].x == e[i].numer && sym_counts[x].y == e[i].denom;
        }
        for (const Nb &x : e) want_seen[x.denom] = 1;
        if (!ok) fail(what, k, order, "row " + std::to_string(r) + ": " + std::to_string(row_n[r]) + " selected, " + std::to_string(e.size()) + " expected");
    }
    if (seen != want_seen) fail(what, k, order, "denominators flagged differ");
}

static std::mt19937_64 shuffler(7);

static void check(const Job &j, uint32_t k, const char *what)
{
    run(j, j.list, k, what, "reference");
    std::vector<Entry> p = j.list;
    std::shuffle(p.begin(), p.end(), shuffler);
    run(j, p, k, what, "shuffled");
}

static const uint32_t KS[] = {1, 3, 10, 100, 1024};

static void check_all_k(const Job &j, const char *what) { for (uint32_t k : KS) check(j, k, what); }

// all fractions equal -- 3/7 spelled 3/7, 6/14, 300/700 -- on the complete graph: pure neighbour order across the diagonal
static void case_equal()
{
    Job j;
    j.n = 150;
    for (uint32_t r = 1; r < j.n; r++)
        for (uint32_t c = 0; c < r; c++) {
            const uint32_t m = (r + c) % 3 == 0 ? 1 : (r + c) % 3 == 1 ? 2 : 100;
            j.list.push_back({r, c, 3 * m, 7 * m, true});
        }
    check_all_k(j, "equal");
}

// three hubs (first, middle, last row) joined to every other row: around a hub, groups of 7 equal fractions (g + 1) / 5000 spelled
// with different denominators and dealt to the neighbours at random -- the 1st, 3rd, 10th, 100th and 1024th place all lie inside a
// group, and a group's members lie on both sides of the middle hub
static void case_straddle(std::mt19937_64 &rng)
{
    Job j;
    j.n = 2803;
    const uint32_t hubs[3] = {0, 1400, 2802};
    std::vector<Entry> v;
    for (uint32_t h : hubs) {
        std::vector<uint2> f;
        for (uint32_t g = 0; g < 401; g++)
            for (uint32_t m = 1; m <= 7; m++) f.push_back(make_uint2((g + 1) * m, 5000 * m));
        std::shuffle(f.begin(), f.end(), rng);
        uint32_t x = 0;
        for (uint32_t o = 0; o < j.n; o++) {
            if (o == h || (o == 0 && h) || (o == 1400 && h == 2802)) continue;        // (hub-hub pairs once, by the earlier hub)
            v.push_back({std::max(h, o), std::min(h, o), f[x].x, f[x].y, true});
            x++;
        }
    }
    std::sort(v.begin(), v.end(), [](const Entry &a, const Entry &b) { return a.row != b.row ? a.row < b.row : a.col < b.col; });
    j.list = v;
    check_all_k(j, "straddle");
}

// row 0 has a mirrored half only, row n - 1 an own half only, and the rows between them see just those two; row 5 sees nobody
static void case_ends(std::mt19937_64 &rng)
{
    Job j;
    j.n = 200;
    for (uint32_t r = 1; r < j.n; r++) {
        if (r == 5) continue;
        const uint32_t d = 1 + (uint32_t)(rng() % 50);
        j.list.push_back({r, 0, (uint32_t)(rng() % (d + 1)), d, true});
        if (r == j.n - 1)
            for (uint32_t c = 1; c < r; c++)
                if (c != 5) { const uint32_t e = 1 + (uint32_t)(rng() % 50); j.list.push_back({r, c, (uint32_t)(rng() % (e + 1)), e, true}); }
    }
    std::sort(j.list.begin(), j.list.end(), [](const Entry &a, const Entry &b) { return a.row != b.row ? a.row < b.row : a.col < b.col; });
    check_all_k(j, "ends");
}

// hubs of degree 1, 63, 64, 65, 1024, 1025 and 2500 (the wave kernel, the long kernel, one chunk, more than the LDS buffer) among
// 2600 leaves that see only hubs (degrees 0 .. 7); the hubs sit at the start, in the middle and at the end of the table
static void case_degrees(std::mt19937_64 &rng)
{
    const uint32_t want[7] = {1, 63, 64, 65, 1024, 1025, 2500};
    const uint32_t hub[7] = {0, 1, 1300, 1301, 1302, 2605, 2606};
    Job j;
    j.n = 2607;
    std::vector<uint32_t> leaves;
    for (uint32_t r = 2; r < 2605; r++)
        if (r < 1300 || r > 1302) leaves.push_back(r);
    for (int h = 0; h < 7; h++) {
        std::vector<uint32_t> pick = leaves;
        std::shuffle(pick.begin(), pick.end(), rng);
        for (uint32_t i = 0; i < want[h]; i++) {
            const uint32_t o = pick[i], d = 1 + (uint32_t)(rng() % 300);
            j.list.push_back({std::max(hub[h], o), std::min(hub[h], o), (uint32_t)(rng() % (d + 1)), d, true});
        }
    }
    std::sort(j.list.begin(), j.list.end(), [](const Entry &a, const Entry &b) { return a.row != b.row ? a.row < b.row : a.col < b.col; });
    check_all_k(j, "degrees");
}

// a complete list of which only some entries are eligible: set bits at every offset of a ballot word, words without any
static void case_bits(std::mt19937_64 &rng)
{
    for (double dens : {0.5, 0.02, 0.001}) {
        Job j;
        j.n = 131;
        std::bernoulli_distribution d(dens);
        for (uint32_t r = 1; r < j.n; r++)
            for (uint32_t c = 0; c < r; c++) j.list.push_back({r, c, (uint32_t)(rng() % 65), 64, d(rng)});
        check_all_k(j, "bits");
    }
    Job j;                                                      // ... and exactly one eligible entry, at each offset in turn
    j.n = 40;
    for (uint32_t r = 1; r < j.n; r++)
        for (uint32_t c = 0; c < r; c++) j.list.push_back({r, c, 1 + (r * c) % 9, 10, false});
    for (uint32_t off = 0; off < 64; off++) {
        j.list[off + 64 * (off % 5)].on = true;
        check(j, 3, "one bit");
        j.list[off + 64 * (off % 5)].on = false;
    }
}

static void fuzz(uint64_t seed, uint32_t cases)
{
    std::mt19937_64 rng(seed);
    for (uint32_t t = 0; t < cases; t++) {
        Job j;
        j.n = 1 + (uint32_t)(rng() % (t % 4 == 0 ? 2500 : 300));
        const uint32_t s = 1 + (uint32_t)(rng() % (t % 3 == 0 ? 8 : t % 3 == 1 ? 1000 : 100000));
        const double edge = t % 4 == 0 ? 0.002 : (double)(rng() % 1000) / 999.0, on = (double)(rng() % 1000) / 999.0;
        const uint32_t zero_share = (uint32_t)(rng() % 100);
        std::bernoulli_distribution de(edge), don(on);
        for (uint32_t r = 1; r < j.n; r++)
            for (uint32_t c = 0; c < r; c++) {
                if (!de(rng)) continue;
                Entry e{r, c, 0, 0, don(rng)};
                e.denom = (rng() & 7) ? s : (uint32_t)(rng() % (s + 1));
                e.numer = (rng() % 100 < zero_share) ? 0u : (uint32_t)(rng() % (e.denom + 1));
                j.list.push_back(e);
            }
        const uint32_t k = (rng() & 1) ? 1 + (uint32_t)(rng() % 1024) : 1 + (uint32_t)(rng() % 12);
        check(j, k, ("fuzz " + std::to_string(t)).c_str());
    }
}

int main(int argc, char **argv)
{
    const std::string c = argc > 1 ? argv[1] : "";
    std::mt19937_64 rng(20261019);
    if (c == "equal") case_equal();
    else if (c == "straddle") case_straddle(rng);
    else if (c == "ends") case_ends(rng);
    else if (c == "degrees") case_degrees(rng);
    else if (c == "bits") case_bits(rng);
    else if (c == "fuzz" && argc > 3) fuzz(strtoull(argv[2], nullptr, 10), (uint32_t)atoi(argv[3]));
    else { printf("usage: knn_emu equal|straddle|ends|degrees|bits | fuzz <seed> <cases>\n"); return 2; }
    if (failures) { printf("%d FAILURES\n", failures); return 1; }
    printf("all cases agree\n");
    return 0;
}
