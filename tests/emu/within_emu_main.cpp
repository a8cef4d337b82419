// within_emu_main.cpp -- runs the kernels of mash_amd/csrc/within.hip unchanged (within_last_kernel, within_j_kernel, both forms
// of within_count_kernel) on host fibers (tools/hipemu) and compares every pair with a literal transcription of the reference's
// serial walk (containSketches, CommandContain.cpp:231-263).  The list form of the count pass is given the pairs with
// j >= j_min in matrix order, which is what the filter passes of compare.hip hand it on the device.
// TEST INFRASTRUCTURE (tests/test_within_emu.py); built with g++.
//
//   within_emu <case>            cases: sizes mixed short pad hash32 single ranges jmin disjoint
//   within_emu fuzz <seed> <n>   n random jobs
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../../mash_amd/csrc/within.hip"

using namespace mg;

static const uint64_t PAD = 0xFFFFFFFFFFFFFFFFull;

struct Table {
    uint64_t n = 0, s = 0;
    std::vector<uint64_t> h;
    std::vector<uint32_t> nh;
    void set(uint64_t row, std::vector<uint64_t> v)
    {
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        if (v.size() > s) v.resize(s);
        nh[row] = (uint32_t)v.size();
        std::copy(v.begin(), v.end(), h.begin() + row * s);
    }
    std::vector<uint64_t> row(uint64_t r) const { return std::vector<uint64_t>(h.begin() + r * s, h.begin() + r * s + nh[r]); }
};

static Table table(uint64_t n, uint64_t s)
{
    Table t;
    t.n = n; t.s = s;
    t.h.assign(n * s + 1, PAD);
    t.nh.assign(n + 1, 0);
    return t;
}

// the reference's loop, as written
static void walk(const std::vector<uint64_t> &ref, const std::vector<uint64_t> &qry, uint32_t &common_out, uint32_t &j_out)
{
    int common = 0;
    int denom = ref.size() < qry.size() ? (int)ref.size() : (int)qry.size();
    int i = 0, j = 0;
    for (int steps = 0; steps < denom && i < (int)ref.size(); steps++) {
        if (ref.at(i) < qry.at(j)) { i++; steps--; }
        else if (qry.at(j) < ref.at(i)) j++;
        else { i++; j++; common++; }
    }
    common_out = (uint32_t)common;
    j_out = (uint32_t)j;
}

static int failures = 0;
static uint64_t pairs_checked = 0, terminations[3] = {0, 0, 0};

static void check(const Table &ref, const Table &qry, uint64_t qb, uint64_t qe, uint32_t j_min, const char *what)
{
    const uint64_t pairs = (qe - qb) * ref.n;
    std::vector<uint2> counts(pairs + 1, make_uint2(0xDEADBEEFu, 0xDEADBEEFu));
    std::vector<unsigned long long> last(ref.n + 1, 0xABABABABABABABABull);
    WithinArgs a{};
    a.ref = ref.h.data(); a.qry = qry.h.data();
    a.ref_n = ref.nh.data(); a.qry_n = qry.nh.data();
    a.ref_s = ref.s; a.qry_s = qry.s;
    a.nref = ref.n; a.first_q = qb; a.pairs = pairs;
    a.ref_last = last.data();
    a.j_min = j_min;
    a.counts = counts.data();
    if (launch_within_last(a, nullptr) != hipSuccess || launch_within_j(a, nullptr) != hipSuccess) { printf("%s: launch refused\n", what); failures++; return; }
    // expectations
    std::vector<uint2> want(pairs);
    for (uint64_t q = qb; q < qe; q++)
        for (uint64_t r = 0; r < ref.n; r++) {
            const std::vector<uint64_t> R = ref.row(r), Q = qry.row(q);
            uint32_t c, j;
            walk(R, Q, c, j);
            if (R.size() && Q.size()) terminations[j < std::min(R.size(), Q.size()) ? 2 : Q.size() <= R.size() ? 0 : 1]++;
            if (Q.size() < j_min || R.size() < j_min) { c = 0; j = 0; }
            want[(q - qb) * ref.n + r] = make_uint2(c, j);
        }
    pairs_checked += pairs;
    for (uint64_t i = 0; i < pairs; i++)
        if (counts[i].x != 0 || counts[i].y != want[i].y) {
            if (failures < 10) printf("%s: j pass, pair %llu: {%u, %u}, expected {0, %u}\n", what, (unsigned long long)i, counts[i].x, counts[i].y, want[i].y);
            failures++;
        }
    if (counts[pairs].x != 0xDEADBEEFu) { printf("%s: j pass wrote past its block\n", what); failures++; }
    // the list form over the pairs a threshold keeps (j_min = 0: the pairs with j >= 1)
    std::vector<uint4> edges;
    for (uint64_t i = 0; i < pairs; i++)
        if (counts[i].y >= std::max(j_min, 1u)) edges.push_back(make_uint4((uint32_t)(qb + i / ref.n), (uint32_t)(i % ref.n), 0xDEADBEEFu, counts[i].y));
    edges.push_back(make_uint4(0, 0, 0xDEADBEEFu, 1));                    // (behind the list)
    a.edges = edges.data();
    a.nedges = edges.size() - 1;
    if (launch_within_count_list(a, nullptr) != hipSuccess) { printf("%s: launch refused\n", what); failures++; return; }
    for (uint64_t e = 0; e + 1 < edges.size(); e++) {
        const uint2 w = want[(edges[e].x - qb) * ref.n + edges[e].y];
        if (edges[e].z != w.x || edges[e].w != w.y) {
            if (failures < 10) printf("%s: list count, query %u reference %u: {%u, %u}, expected {%u, %u}\n", what, edges[e].x, edges[e].y, edges[e].z, edges[e].w, w.x, w.y);
            failures++;
        }
    }
    if (edges.back().z != 0xDEADBEEFu) { printf("%s: list count wrote past its list\n", what); failures++; }
    // the matrix form
    if (launch_within_count(a, nullptr) != hipSuccess) { printf("%s: launch refused\n", what); failures++; return; }
    for (uint64_t i = 0; i < pairs; i++)
        if (counts[i].x != want[i].x || counts[i].y != want[i].y) {
            if (failures < 10) printf("%s: matrix count, pair %llu: {%u, %u}, expected {%u, %u}\n", what, (unsigned long long)i, counts[i].x, counts[i].y, want[i].x, want[i].y);
            failures++;
        }
    if (counts[pairs].x != 0xDEADBEEFu) { printf("%s: matrix count wrote past its block\n", what); failures++; }
}

// rows drawn from one pool of `universe` values below `limit`, so that rows share hashes; a row's count is its own
static void fill(Table &t, std::mt19937_64 &rng, uint64_t universe, uint64_t limit, int ragged)
{
    std::vector<uint64_t> pool(universe);
    std::mt19937_64 prng(12345 + universe);                               // (the same pool for both tables of a job)
    for (auto &x : pool) x = limit == ~0ull ? prng() : prng() % limit;
    std::sort(pool.begin(), pool.end());
    for (uint64_t r = 0; r < t.n; r++) {
        uint64_t want = t.s;
        if (ragged == 1) want = rng() % (t.s + 1);
        if (ragged == 2) want = r % 3 == 0 ? 0 : r % 3 == 1 ? 1 : rng() % (t.s + 1);
        std::vector<uint64_t> v;
        // a row is a window of the sorted pool's order statistics or a scatter over it: both occur in sketches
        const uint64_t lo = rng() % universe, span = std::max<uint64_t>(1, rng() % universe);
        for (uint64_t i = 0; i < want * 2 && v.size() < want; i++) v.push_back(pool[(lo + rng() % span) % universe]);
        t.set(r, v);
    }
}

static void job(std::mt19937_64 &rng, uint64_t nref, uint64_t sref, uint64_t nqry, uint64_t sqry, uint64_t universe, uint64_t limit, int ragged,
                uint32_t j_min, const char *what)
{
    Table R = table(nref, sref), Q = table(nqry, sqry);
    fill(R, rng, universe, limit, ragged);
    fill(Q, rng, universe, limit, ragged);
    check(R, Q, 0, nqry, j_min, what);
}

static void case_sizes(std::mt19937_64 &rng)
{
    for (uint64_t s : {1ull, 5ull, 64ull, 65ull, 1000ull, 5000ull})
        for (uint64_t n : {1ull, 7ull, 70ull}) {
            if (s >= 1000 && n > 7) continue;
            job(rng, n, s, n + 2, s, s * 3 + 2, ~0ull, 0, 0, "sizes full rows");
            job(rng, n, s, n + 2, s, s * 3 + 2, ~0ull, 1, 0, "sizes ragged rows");
        }
}

static void case_mixed(std::mt19937_64 &rng)                               // the tables differ in sketch size, either way round
{
    job(rng, 9, 1000, 11, 64, 1500, ~0ull, 1, 0, "mixed: smaller queries");
    job(rng, 9, 64, 11, 1000, 1500, ~0ull, 1, 0, "mixed: larger queries");
    job(rng, 5, 65, 70, 1, 100, ~0ull, 0, 0, "mixed: queries of one hash");
    job(rng, 70, 1, 5, 65, 100, ~0ull, 0, 0, "mixed: references of one hash");
}

static void case_short(std::mt19937_64 &rng)                               // rows of 0, 1 and fewer than s hashes
{
    job(rng, 12, 64, 13, 64, 90, ~0ull, 2, 0, "short");
    job(rng, 12, 5, 13, 65, 40, ~0ull, 2, 0, "short, mixed sizes");
}

static void case_pad()
{
    // a real hash equal to the padding value: it is a member where a row holds it, and two short rows' padding never matches
    Table R = table(3, 4), Q = table(3, 6);
    R.set(0, {5, 9});                       // padded
    R.set(1, {5, 9, PAD});                  // PAD is a real hash here
    R.set(2, {});
    Q.set(0, {5});                          // padded
    Q.set(1, {9, PAD});                     // PAD real
    Q.set(2, {PAD});
    check(R, Q, 0, 3, 0, "pad");
    Table A = table(1, 8), B = table(1, 8);
    A.set(0, {1, 2});
    B.set(0, {1, 3});
    check(A, B, 0, 1, 0, "pad: two short rows");
}

static void case_hash32(std::mt19937_64 &rng)
{
    job(rng, 20, 64, 20, 65, 150, 1ull << 32, 1, 0, "hash32");
    job(rng, 3, 1000, 4, 1000, 2500, 1ull << 32, 0, 0, "hash32 s=1000");
}

static void case_single(std::mt19937_64 &rng)
{
    job(rng, 1, 64, 70, 64, 150, ~0ull, 1, 0, "nref = 1");
    job(rng, 70, 64, 1, 64, 150, ~0ull, 1, 0, "nqry = 1");
    job(rng, 1, 1, 1, 1, 2, ~0ull, 0, 0, "1 x 1");
}

static void case_ranges(std::mt19937_64 &rng)
{
    Table R = table(7, 65), Q = table(33, 64);
    fill(R, rng, 150, ~0ull, 1);
    fill(Q, rng, 150, ~0ull, 1);
    check(R, Q, 0, 33, 0, "ranges: all");
    check(R, Q, 5, 6, 0, "ranges: one row");
    check(R, Q, 17, 33, 0, "ranges: the tail");
    check(R, Q, 9, 9, 0, "ranges: empty");
}

static void case_jmin(std::mt19937_64 &rng)
{
    for (uint32_t jm : {1u, 2u, 12u, 40u, 64u, 65u})
        job(rng, 15, 64, 17, 64, 100, ~0ull, 1, jm, "jmin");
    job(rng, 9, 1000, 11, 64, 1500, ~0ull, 1, 50, "jmin, mixed sizes");
}

static void case_disjoint()
{
    // the reference entirely below the query (j = 0), entirely above it (j = min), and interleaved with nothing common
    Table R = table(3, 8), Q = table(2, 8);
    R.set(0, {1, 2, 3});
    R.set(1, {100, 101, 102, 103});
    R.set(2, {11, 13, 15, 17, 19});
    Q.set(0, {10, 12, 14, 16});
    Q.set(1, {10, 11, 12, 13, 14, 15, 16, 17});
    check(R, Q, 0, 2, 0, "disjoint");
}

int main(int argc, char **argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    std::mt19937_64 rng(20261021);
    if (what == "sizes") case_sizes(rng);
    else if (what == "mixed") case_mixed(rng);
    else if (what == "short") case_short(rng);
    else if (what == "pad") case_pad();
    else if (what == "hash32") case_hash32(rng);
    else if (what == "single") case_single(rng);
    else if (what == "ranges") case_ranges(rng);
    else if (what == "jmin") case_jmin(rng);
    else if (what == "disjoint") case_disjoint();
    else if (what == "fuzz" && argc > 3) {
        rng.seed(strtoull(argv[2], nullptr, 10));
        const int n = atoi(argv[3]);
        for (int i = 0; i < n; i++) {
            const uint64_t sref = 1 + rng() % (rng() % 4 ? 80 : 700), sqry = 1 + rng() % (rng() % 4 ? 80 : 700);
            const uint64_t universe = 2 + rng() % (3 * std::max(sref, sqry));
            const uint32_t jm = rng() % 3 ? 0u : (uint32_t)(rng() % (std::min(sref, sqry) + 2));
            job(rng, 1 + rng() % 20, sref, 1 + rng() % 20, sqry, universe, rng() % 2 ? ~0ull : 1ull << 32, (int)(rng() % 3), jm, "fuzz");
        }
        if (!terminations[0] || !terminations[1] || !terminations[2]) { printf("fuzz: a termination never occurred\n"); failures++; }
    } else { printf("usage: within_emu <case> | fuzz <seed> <n>\n"); return 2; }
    if (failures) { printf("%d mismatches\n", failures); return 1; }
    printf("all cases agree (%llu pairs; ended by |Q| %llu, by |R| %llu, by exhaustion %llu)\n", (unsigned long long)pairs_checked,
           (unsigned long long)terminations[0], (unsigned long long)terminations[1], (unsigned long long)terminations[2]);
    return 0;
}
