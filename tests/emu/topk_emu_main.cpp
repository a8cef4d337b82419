// topk_emu_main.cpp -- runs the selection kernels of mash_amd/csrc/topk.hip through launch_topk_select (topk_select_kernel:
// streaming, ballots, the bitonic prune, the bound, for rows of more than 64 pairs; topk_select_short_kernel: a wave per row of
// up to 64 pairs -- the short lists of `short` and `bits`, the short lists and narrow matrices of the fuzz jobs) on host fibers
// (tools/hipemu) and compares every row's list with a std::stable_sort statement of the definition: eligible pairs, best first by the exact fraction (compared in 128-bit integers here, so the check does not share
// the kernel's arithmetic), equal fractions in column order, the first k.
// TEST INFRASTRUCTURE (tests/test_topk_emu.py); built with g++.
//
//   topk_emu <case>            cases: ties cut short bits long farey
//   topk_emu fuzz <seed> <n>   n random jobs
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../../mash_amd/csrc/topk.hip"

using namespace mg;

struct Job {
    std::vector<uint2> counts;
    std::vector<unsigned long long> masks;       // empty: every pair eligible
    std::vector<uint32_t> base, cnt;             // empty: a matrix of nrows x ncols
    uint32_t nrows = 0, ncols = 0;
};

static bool eligible(const Job &j, uint64_t idx) { return j.masks.empty() || ((j.masks[idx >> 6] >> (idx & 63)) & 1ull); }

// the definition
static std::vector<uint32_t> expected_row(const Job &j, uint32_t row, uint32_t k)
{
    const uint64_t begin = j.base.empty() ? (uint64_t)row * j.ncols : j.base[row];
    const uint32_t n = j.cnt.empty() ? j.ncols : j.cnt[row];
    std::vector<uint32_t> v;
    for (uint32_t p = 0; p < n; p++)
        if (eligible(j, begin + p)) v.push_back((uint32_t)(begin + p));
    std::stable_sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) {
        const uint2 a = j.counts[x], b = j.counts[y];
        const unsigned __int128 l = (unsigned __int128)a.x * (b.y ? b.y : 1u), r = (unsigned __int128)b.x * (a.y ? a.y : 1u);
        return l > r;
    });
    if (v.size() > k) v.resize(k);
    return v;
}

static int failures = 0;

static void check(const Job &j, uint32_t k, const char *what)
{
    std::vector<uint32_t> sel((size_t)j.nrows * k, 0xDEADBEEFu), row_n(j.nrows, 0xDEADBEEFu), seen(1u << 17, 0);
    TopkArgs a{};
    a.counts = j.counts.data();
    a.masks = j.masks.empty() ? nullptr : j.masks.data();
    a.seg_base = j.base.empty() ? nullptr : j.base.data();
    a.seg_cnt = j.cnt.empty() ? nullptr : j.cnt.data();
    a.ncols = j.ncols;
    a.nrows = j.nrows;
    a.k = k;
    a.sel = sel.data();
    a.row_n = row_n.data();
    a.denom_seen = seen.data();
    a.s = (uint32_t)seen.size() - 1;
    if (launch_topk_select(a, nullptr) != hipSuccess) { printf("%s k=%u: launch refused\n", what, k); failures++; return; }
    std::vector<uint32_t> want_seen(seen.size(), 0);
    for (uint32_t r = 0; r < j.nrows; r++) {
        const std::vector<uint32_t> e = expected_row(j, r, k);
        bool ok = row_n[r] == e.size();
        for (size_t i = 0; ok && i < e.size(); i++) ok = sel[(size_t)r * k + i] == e[i];
        for (uint32_t x : e) want_seen[j.counts[x].y] = 1;
        if (!ok) {
            if (failures < 10) printf("%s k=%u row %u: %u selected, %zu expected\n", what, k, r, row_n[r], e.size());
            failures++;
        }
    }
    if (seen != want_seen) { printf("%s k=%u: denominators flagged differ\n", what, k); failures++; }
}

static const uint32_t KS[] = {1, 3, 10, 100, 1024};

static void check_all_k(const Job &j, const char *what) { for (uint32_t k : KS) check(j, k, what); }

static void set_bits(Job &j, std::mt19937_64 &rng, double density)
{
    j.masks.assign((j.counts.size() + 63) / 64 + 1, 0);
    std::bernoulli_distribution d(density);
    for (uint64_t i = 0; i < j.counts.size(); i++)
        if (d(rng)) j.masks[i >> 6] |= 1ull << (i & 63);
}

static Job matrix(uint32_t nrows, uint32_t ncols) { Job j; j.nrows = nrows; j.ncols = ncols; j.counts.resize((size_t)nrows * ncols); return j; }

static Job lists(const std::vector<uint32_t> &cnt, uint32_t lead)
{
    Job j;
    j.nrows = (uint32_t)cnt.size();
    j.cnt = cnt;
    uint32_t at = lead;                                     // (lists start anywhere in the entry array)
    for (uint32_t c : cnt) { j.base.push_back(at); at += c; }
    j.counts.resize(at);
    return j;
}

static void case_ties()
{
    Job j = matrix(3, 3000);                               // all fractions equal: 3/7 written as 3/7, 6/14, 300/700; a row of 0/x; a row of 0/0
    for (uint32_t c = 0; c < 3000; c++) {
        const uint32_t m = c % 3 == 0 ? 1 : c % 3 == 1 ? 2 : 100;
        j.counts[c] = make_uint2(3 * m, 7 * m);
        j.counts[3000 + c] = make_uint2(0, 1 + c % 50);
        j.counts[6000 + c] = make_uint2(0, 0);
    }
    check_all_k(j, "ties");
}

static void case_cut(std::mt19937_64 &rng)
{
    // groups of 7 equal fractions (g+1)/(5000) spelled with different denominators, shuffled: the 1st, 3rd, 10th, 100th and 1024th
    // place all lie inside a group, so every tested k cuts through a tie
    Job j = matrix(2, 7 * 400);
    for (uint32_t r = 0; r < 2; r++) {
        std::vector<uint2> v;
        for (uint32_t g = 0; g < 400; g++)
            for (uint32_t m = 1; m <= 7; m++) v.push_back(make_uint2((g + 1) * m, 5000 * m));
        std::shuffle(v.begin(), v.end(), rng);
        std::copy(v.begin(), v.end(), j.counts.begin() + (size_t)r * v.size());
    }
    check_all_k(j, "cut");
}

static void case_short(std::mt19937_64 &rng)
{
    Job j = lists({0, 1, 2, 5, 63, 64, 65, 0, 900, 1500}, 37);
    for (auto &c : j.counts) { c.y = 1 + (uint32_t)(rng() % 200); c.x = (uint32_t)(rng() % (c.y + 1)); }
    check_all_k(j, "short lists");
    set_bits(j, rng, 0.1);
    check_all_k(j, "short lists, masked");
    Job m = matrix(4, 5000);
    for (auto &c : m.counts) { c.y = 1000; c.x = (uint32_t)(rng() % 1001); }
    m.masks.assign((m.counts.size() + 63) / 64 + 1, 0);    // row 0: nobody, row 1: one pair, rows 2 and 3: a few
    m.masks[(5000 + 4321) >> 6] |= 1ull << ((5000 + 4321) & 63);
    for (uint32_t i = 0; i < 9; i++) { const uint64_t x = 10000 + 500 * i + 3; m.masks[x >> 6] |= 1ull << (x & 63); }
    for (uint32_t i = 0; i < 99; i++) { const uint64_t x = 15000 + 50 * i; m.masks[x >> 6] |= 1ull << (x & 63); }
    check_all_k(m, "short matrix");
}

static void case_bits(std::mt19937_64 &rng)
{
    for (double dens : {0.5, 0.02, 0.001}) {
        Job j = matrix(3, 4097);                           // (rows start at every bit offset)
        for (auto &c : j.counts) { c.y = 64; c.x = (uint32_t)(rng() % 65); }
        set_bits(j, rng, dens);
        check_all_k(j, "bits matrix");
        Job l = lists({3001, 17, 2049, 1024}, 5);
        for (auto &c : l.counts) { c.y = 64; c.x = (uint32_t)(rng() % 65); }
        set_bits(l, rng, dens);
        check_all_k(l, "bits lists");
    }
}

static void case_long(std::mt19937_64 &rng)
{
    Job j = matrix(3, 20011);                              // ten buffers long: ascending (every chunk beats the bound), descending, random
    for (uint32_t c = 0; c < 20011; c++) {
        j.counts[c] = make_uint2(c, 20011);
        j.counts[20011 + c] = make_uint2(20010 - c, 20011);
        const uint32_t d = 1 + (uint32_t)(rng() % 100000);
        j.counts[2 * 20011 + c] = make_uint2((uint32_t)(rng() % (d + 1)), d);
    }
    check_all_k(j, "long");
    set_bits(j, rng, 0.3);
    check_all_k(j, "long, masked");
}

static void case_farey(std::mt19937_64 &rng)
{
    // neighbours no float32 and no 32-bit quotient separates, with mixed denominators, among full-size sketch sizes
    std::vector<uint2> v = {make_uint2(4999, 9999), make_uint2(5000, 10001), make_uint2(5000, 10000), make_uint2(49999, 99999),
                            make_uint2(50000, 100001), make_uint2(50000, 100000), make_uint2(0, 0), make_uint2(0, 100000),
                            make_uint2(1, 4294967295u), make_uint2(1, 4294967294u), make_uint2(4294967294u, 4294967295u),
                            make_uint2(4294967293u, 4294967294u), make_uint2(4294967295u, 4294967295u)};
    for (uint32_t d = 65530; d < 65560; d++) { v.push_back(make_uint2(d / 2, d)); v.push_back(make_uint2(d / 2 + 1, d + 1)); }
    for (uint32_t i = 0; i < 40; i++) { const uint32_t d = 2000000000u + (uint32_t)(rng() % 1000); v.push_back(make_uint2(d / 3 + (uint32_t)(rng() % 3), d)); }
    Job j = matrix(4, (uint32_t)v.size() * 3);
    for (uint32_t r = 0; r < 4; r++) {
        std::vector<uint2> w;
        for (int rep = 0; rep < 3; rep++) w.insert(w.end(), v.begin(), v.end());
        std::shuffle(w.begin(), w.end(), rng);
        std::copy(w.begin(), w.end(), j.counts.begin() + (size_t)r * w.size());
    }
    Job big = matrix(1, 6000);                             // ... and spread over several chunks
    for (auto &c : big.counts) { const uint32_t d = 99990 + (uint32_t)(rng() % 20); c = make_uint2(d / 2 + (uint32_t)(rng() % 2), d); }
    for (uint32_t k : KS) {
        // (denominators here exceed the flag array of check(): run without it)
        for (const Job *job : {&j, &big}) {
            std::vector<uint32_t> sel((size_t)job->nrows * k), row_n(job->nrows);
            TopkArgs a{};
            a.counts = job->counts.data();
            a.ncols = job->ncols;
            a.nrows = job->nrows;
            a.k = k;
            a.sel = sel.data();
            a.row_n = row_n.data();
            launch_topk_select(a, nullptr);
            for (uint32_t r = 0; r < job->nrows; r++) {
                const std::vector<uint32_t> e = expected_row(*job, r, k);
                bool ok = row_n[r] == e.size();
                for (size_t i = 0; ok && i < e.size(); i++) ok = sel[(size_t)r * k + i] == e[i];
                if (!ok) { printf("farey k=%u row %u differs\n", k, r); failures++; }
            }
        }
    }
}

static void fuzz(uint64_t seed, uint32_t cases)
{
    std::mt19937_64 rng(seed);
    for (uint32_t t = 0; t < cases; t++) {
        const uint32_t s = 1 + (uint32_t)(rng() % (t % 3 == 0 ? 8 : t % 3 == 1 ? 1000 : 100000));
        Job j;
        if (rng() & 1) j = matrix(1 + (uint32_t)(rng() % 4), 1 + (uint32_t)(rng() % 5000));
        else {
            std::vector<uint32_t> cnt(1 + rng() % 6);
            for (auto &c : cnt) c = (uint32_t)(rng() % ((rng() & 3) ? 300 : 5000));
            j = lists(cnt, (uint32_t)(rng() % 100));
        }
        const uint32_t zero_share = (uint32_t)(rng() % 100);
        for (auto &c : j.counts) {
            c.y = (rng() & 7) ? s : (uint32_t)(rng() % (s + 1));
            c.x = (rng() % 100 < zero_share) ? 0u : (uint32_t)(rng() % (c.y + 1));
        }
        if (rng() % 3) set_bits(j, rng, (double)(rng() % 1000) / 999.0);
        const uint32_t k = (rng() & 1) ? 1 + (uint32_t)(rng() % 1024) : 1 + (uint32_t)(rng() % 12);
        check(j, k, ("fuzz " + std::to_string(t)).c_str());
    }
}

int main(int argc, char **argv)
{
    const std::string c = argc > 1 ? argv[1] : "";
    std::mt19937_64 rng(20261017);
    if (c == "ties") case_ties();
    else if (c == "cut") case_cut(rng);
    else if (c == "short") case_short(rng);
    else if (c == "bits") case_bits(rng);
    else if (c == "long") case_long(rng);
    else if (c == "farey") case_farey(rng);
    else if (c == "fuzz" && argc > 3) fuzz(strtoull(argv[2], nullptr, 10), (uint32_t)atoi(argv[3]));
    else { printf("usage: topk_emu ties|cut|short|bits|long|farey | fuzz <seed> <cases>\n"); return 2; }
    if (failures) { printf("%d FAILURES\n", failures); return 1; }
    printf("all cases agree\n");
    return 0;
}
