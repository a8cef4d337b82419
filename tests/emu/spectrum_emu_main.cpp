// spectrum_emu_main.cpp -- runs the kernels of `mash triangle -H` / `mash dist -H` (mash_amd/csrc/spectrum.hip), unchanged, through
// their launchers on the CPU (tools/hipemu): sp_marked_kernel over ballot words in list mode and in flat triangle mode,
// sp_all_kernel over every count of a block, sp_list_kernel with both binnings -- each in the combining variant (LDS bins where
// 4 (s + 1) bytes fit in 64 KiB, memory beyond) and in the plain one.  The judge is a sequential restatement written here: one loop
// over the entries a launch names and a std::map.  Which pairs a launch names is stated by the definition of the layouts
// (entries_of), not by pair_rc.  The driver does what the host does: the bins live across the launches of a job and are cleared once;
// when the table of the other denominators overflows it is enlarged four times over, every bin cleared, and the job run again from
// its first launch.
// TEST INFRASTRUCTURE (tests/test_spectrum_emu.py); built with g++.  The emulator runs workgroups one after another: what is pinned
// here is the arithmetic (which lanes combine, the homes of a key, the clipping, the bounds, the regrow), not the races between
// workgroups on one bin -- those run on the device only (tests/test_spectrum_gpu.py).
//
//   spectrum_emu <case>            cases: small lengths words space pieces lists sizes hot denoms regrow
//   spectrum_emu fuzz <seed> <n>   n random jobs
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../mash_amd/csrc/spectrum.hip"

using namespace mg;

typedef unsigned long long u64;

static uint64_t tri(uint64_t r) { return r ? r * (r - 1) / 2 : 0; }

enum Kind { MARKED, ALL, LIST };

// one launch of a job
struct Launch {
    Kind kind = MARKED;
    std::vector<uint2> rc;                       // list mode (empty: flat triangle from first_row on)
    std::vector<uint2> counts;                   // {numer, denom} of every pair of the launch, marked or not
    uint64_t first_row = 0, pairs = 0;
    std::vector<u64> masks;                      // MARKED
    PairSpace sp{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u};
    void set(uint64_t idx) { masks[idx >> 6] |= 1ull << (idx & 63); }
    bool get(uint64_t idx) const { return (masks[idx >> 6] >> (idx & 63)) & 1ull; }
};

struct Job {
    uint32_t s = 64;
    std::vector<Launch> launches;
    std::vector<uint32_t> nh_row, nh_col;        // LIST: the hash counts the rule denominators come from
    uint64_t slots = 1024;                       // the table's first size
};

static Launch flat_launch(Kind kind, uint64_t first_row, uint64_t row_end, uint2 fill)
{
    Launch L;
    L.kind = kind;
    L.first_row = first_row;
    L.pairs = tri(row_end) - tri(first_row);
    L.masks.assign((L.pairs + 63) / 64, 0);
    L.counts.assign(L.pairs, fill);
    return L;
}

static Launch list_launch(Kind kind, const std::vector<uint2> &rc, const std::vector<uint2> &counts)
{
    Launch L;
    L.kind = kind;
    L.rc = rc;
    L.counts = counts;
    L.pairs = rc.size();
    L.masks.assign((L.pairs + 63) / 64, 0);
    return L;
}

typedef std::map<u64, u64> BinMap;
static u64 key_of(uint32_t numer, uint32_t denom) { return (u64)numer << 32 | denom; }

// the judge: what a job's launches add up to, by the definition of the layouts
struct Answer { BinMap bins, rule; u64 listed_zero = 0, other = 0; };

static Answer judge(const Job &J)
{
    Answer w;
    for (const Launch &L : J.launches) {
        uint64_t row = L.first_row ? L.first_row : 1, col = 0;
        for (uint64_t i = 0; i < L.pairs; i++) {
            uint64_t r = row, c = col;
            if (!L.rc.empty()) { r = L.rc[i].x; c = L.rc[i].y; }
            else if (++col == row) { row++; col = 0; }
            if (L.kind == MARKED && !(L.get(i) && r < L.sp.rows && c < L.sp.cols)) continue;
            w.bins[key_of(L.counts[i].x, L.counts[i].y)]++;
            if (L.counts[i].y != J.s) w.other++;
            if (L.kind != LIST) continue;
            const uint64_t a = std::min<uint64_t>(J.nh_row[r], J.s), b = std::min<uint64_t>(J.nh_col[c], J.s);
            w.rule[std::min<uint64_t>(J.s, a + b)]++;
            w.listed_zero += L.counts[i].x == 0;
        }
    }
    return w;
}

static int failures = 0;
constexpr u64 GUARD64 = 0xDEADBEEFDEADBEEFull;

struct Ran { BinMap bins, rule; u64 listed_zero = 0; uint64_t regrows = 0; bool ok = true; };

// the device side, as host_spectrum.cpp drives it
static Ran run(const Job &J, bool plain)
{
    Ran out;
    uint64_t slots = J.slots;
    for (;;) {
        std::vector<u64> full((size_t)J.s + 2, 0), rule((size_t)J.s + 2, 0), keys(slots + 1, CF_NONE), vals(slots + 1, 0), ctl(3, 0);
        full[J.s + 1] = rule[J.s + 1] = keys[slots] = vals[slots] = ctl[2] = GUARD64;
        const SpectrumBins b{full.data(), keys.data(), vals.data(), slots, reinterpret_cast<uint32_t *>(ctl.data() + 1), J.s};
        for (const Launch &L : J.launches) {
            hipError_t e = hipSuccess;
            if (L.kind == ALL) {
                e = launch_spectrum_all(L.counts.data(), L.pairs, b, nullptr, plain);
            } else if (L.kind == LIST) {
                e = launch_spectrum_list(L.counts.data(), L.rc.data(), L.pairs, J.nh_row.data(), J.nh_col.data(), b, rule.data(), ctl.data(), nullptr, plain);
            } else {
                FinishArgs a{};
                a.counts = L.counts.data();
                a.pairs = L.pairs;
                a.first_row = L.first_row;
                a.triangle = 1;
                a.s = J.s;
                a.masks = const_cast<u64 *>(L.masks.data());
                a.list_rc = L.rc.empty() ? nullptr : L.rc.data();
                e = launch_spectrum_marked(a, L.sp, b, nullptr, plain);
            }
            if (e != hipSuccess) { out.ok = false; return out; }
        }
        if (full[J.s + 1] != GUARD64 || rule[J.s + 1] != GUARD64 || keys[slots] != GUARD64 || vals[slots] != GUARD64 || ctl[2] != GUARD64) {
            printf("FAIL a guard word was overwritten\n");
            out.ok = false;
            return out;
        }
        if ((uint32_t)ctl[1]) {
            if (slots > (1ull << 24)) { out.ok = false; return out; }
            slots *= 4;
            out.regrows++;
            continue;
        }
        for (uint64_t x = 0; x <= J.s; x++) {
            if (full[x]) out.bins[key_of((uint32_t)x, J.s)] += full[x];
            if (rule[x]) out.rule[x] += rule[x];
        }
        for (uint64_t i = 0; i < slots; i++) {
            if (keys[i] == CF_NONE) { if (vals[i]) out.ok = false; continue; }
            if ((uint32_t)keys[i] == J.s && (keys[i] >> 32) <= J.s) out.ok = false;      // a key with a home in full[] never enters the table
            if (vals[i]) out.bins[keys[i]] += vals[i];
        }
        out.listed_zero = ctl[0];
        return out;
    }
}

static void check(const std::string &name, const Job &J, int want_regrows = -1)
{
    const Answer w = judge(J);
    u64 entries = 0;
    for (const auto &kv : w.bins) entries += kv.second;
    bool good = true;
    uint64_t regrows = 0;
    for (int plain = 0; plain < 2; plain++) {
        const Ran r = run(J, plain != 0);
        if (!r.ok || r.bins != w.bins || r.rule != w.rule || r.listed_zero != w.listed_zero) {
            good = false;
            printf("FAIL %s (%s): %zu bins against %zu, rule %zu against %zu, listed_zero %llu against %llu%s\n", name.c_str(), plain ? "plain" : "combined",
                   r.bins.size(), w.bins.size(), r.rule.size(), w.rule.size(), r.listed_zero, w.listed_zero, r.ok ? "" : ", the run itself failed");
        }
        regrows = r.regrows;
    }
    if (want_regrows == 0 && regrows) { good = false; printf("FAIL %s: the table regrew\n", name.c_str()); }
    if (want_regrows > 0 && !regrows) { good = false; printf("FAIL %s: the table did not regrow\n", name.c_str()); }
    if (!good) { failures++; return; }
    printf("ok %s: %llu entries in %zu bins, %llu with another denominator, %llu regrows\n", name.c_str(), entries, w.bins.size(), w.other, (u64)regrows);
}

// counts that must never reach a bin: beside clear bits, behind the pair space
static uint2 junk(uint64_t idx, uint32_t s) { return make_uint2((uint32_t)(idx * 7 % 5), s - 1 - (uint32_t)(idx % 3)); }

static Job one(uint32_t s, Launch L)
{
    Job J;
    J.s = s;
    J.launches.push_back(std::move(L));
    return J;
}

static void junk_fill(Launch &L, uint32_t s)
{
    for (uint64_t i = 0; i < L.pairs; i++) L.counts[i] = junk(i, s);
}

static void mark(Launch &L, uint64_t idx, uint32_t numer, uint32_t denom)
{
    L.set(idx);
    L.counts[idx] = make_uint2(numer, denom);
}

static void case_small()
{
    Launch L = flat_launch(MARKED, 0, 12, make_uint2(0, 64));
    junk_fill(L, 64);
    for (uint64_t i = 0; i < L.pairs; i += 3) mark(L, i, (uint32_t)(i % 5) * 8, 64);
    mark(L, 1, 3, 31);
    mark(L, 64, 3, 31);
    check("66 pairs of 12 rows, a third marked, one key twice in the table", one(64, L));
    Launch A = flat_launch(ALL, 0, 12, make_uint2(0, 64));
    for (uint64_t i = 0; i < A.pairs; i += 4) A.counts[i] = make_uint2((uint32_t)(i % 7), 64);
    A.counts[5] = make_uint2(0, 0);
    check("every count of 66 pairs", one(64, A));
}

static void case_lengths()
{
    for (uint64_t rows : {2, 3, 11, 12, 13, 23, 24, 91, 92, 200}) {          // 1, 3, 55, 66, 78, 253, 276, 4095, 4186, 19900 pairs
        for (Kind kind : {MARKED, ALL}) {
            Launch L = flat_launch(kind, 0, rows, make_uint2(1, 64));
            if (kind == MARKED) junk_fill(L, 64);
            for (uint64_t i = 0; i < L.pairs; i++) {
                if (kind == MARKED) { if (i % 2 == 0 || i + 1 == L.pairs) mark(L, i, (uint32_t)(i % 65), 64); }
                else L.counts[i] = make_uint2((uint32_t)(i % 65), 64);
            }
            check(std::string(kind == MARKED ? "marked" : "all") + ", " + std::to_string(L.pairs) + " pairs", one(64, L));
        }
    }
}

static void case_words()
{
    {   // the first words of a flat triangle: one word spans rows 1 .. 11
        Launch L = flat_launch(MARKED, 0, 40, make_uint2(0, 64));
        junk_fill(L, 64);
        for (uint64_t i = 0; i < 192; i++) mark(L, i, (uint32_t)(i % 9), 64);
        check("the first three words of a flat triangle, all set", one(64, L));
    }
    {   // a single set bit in a word's last lane, and in the last word's last pair
        Launch L = flat_launch(MARKED, 0, 40, make_uint2(0, 64));
        junk_fill(L, 64);
        mark(L, 63, 17, 64);
        mark(L, 64 * 5 + 63, 9, 33);
        mark(L, L.pairs - 1, 64, 64);
        check("single set bits in last lanes", one(64, L));
    }
    {   // a block that starts at a later row
        Launch L = flat_launch(MARKED, 37, 61, make_uint2(0, 64));
        junk_fill(L, 64);
        for (uint64_t i = 0; i < L.pairs; i += 5) mark(L, i, (uint32_t)(i % 64), 64);
        check("rows 37 .. 60 of a flat triangle", one(64, L));
    }
    {   // a word with fewer entries than the rounds take, and one with exactly as many
        Launch L = flat_launch(MARKED, 0, 30, make_uint2(0, 64));
        junk_fill(L, 64);
        for (uint64_t i = 0; i < 7; i++) mark(L, i * 9, 5, 64);
        for (uint64_t i = 0; i < 8; i++) mark(L, 64 + i * 8, 5, 64);
        check("words of 7 and of 8 entries of one key", one(64, L));
    }
}

static void case_space()
{
    {   // flat: rows and columns of the pair space cut set bits away
        Launch L = flat_launch(MARKED, 0, 50, make_uint2(0, 64));
        for (uint64_t i = 0; i < L.pairs; i++) mark(L, i, (uint32_t)(i % 11), i % 4 ? 64u : 40u);
        L.sp = PairSpace{30u, 20u, 0u, 0u};
        check("flat triangle of 50 rows, pair space 30 x 20", one(64, L));
        L.sp = PairSpace{0xFFFFFFFFu, 7u, 100u, 5u};
        check("flat triangle of 50 rows, pair space any x 7", one(64, L));
    }
    {   // list: rows unsorted, some outside
        std::vector<uint2> rc, cnt;
        for (uint32_t i = 0; i < 300; i++) { rc.push_back(make_uint2((i * 37) % 90, (i * 11) % 80)); cnt.push_back(make_uint2(i % 13, i % 5 ? 64u : 50u)); }
        Launch L = list_launch(MARKED, rc, cnt);
        for (uint64_t i = 0; i < L.pairs; i++) if (i % 7) L.set(i);
        L.sp = PairSpace{60u, 60u, 0u, 0u};
        check("list of 300 pairs, pair space 60 x 60", one(64, L));
    }
}

static void case_pieces()
{
    for (int pieces : {2, 5}) {
        Job J;
        J.s = 64;
        const uint64_t rows = 120;
        for (int p = 0; p < pieces; p++) {
            const uint64_t r0 = p ? rows * p / pieces : 0, r1 = rows * (p + 1) / pieces;
            Launch L = flat_launch(p % 2 ? ALL : MARKED, r0, r1, make_uint2(0, 64));
            for (uint64_t i = 0; i < L.pairs; i++) {
                const uint2 c = make_uint2((uint32_t)((i + p) % 17), (i + p) % 6 ? 64u : 48u);
                if (L.kind == ALL) L.counts[i] = c;
                else if (i % 3 != 1) mark(L, i, c.x, c.y);
                else L.counts[i] = junk(i, 64);
            }
            J.launches.push_back(L);
        }
        check(std::to_string(pieces) + " pieces over one set of bins, marked and whole by turns", J);
    }
}

static Job list_job(uint32_t s, uint32_t rows, uint32_t per_row, uint32_t seed, bool short_rows)
{
    std::mt19937 rng(seed);
    Job J;
    J.s = s;
    J.nh_row.resize(rows);
    for (uint32_t i = 0; i < rows; i++) J.nh_row[i] = !short_rows || rng() % 4 ? s + (rng() % 2) * 5 : rng() % s;     // (more than s hashes: clamped)
    J.nh_col = J.nh_row;
    std::vector<uint2> rc, cnt;
    for (uint32_t i = 1; i < rows; i++) {
        for (uint32_t k = 0; k < per_row && k < i; k++) {
            const uint32_t j = (i * 7 + k * 13) % i;
            const uint64_t d = std::min<uint64_t>(s, (uint64_t)std::min(J.nh_row[i], s) + std::min(J.nh_row[j], s));
            rc.push_back(make_uint2(i, j));
            cnt.push_back(make_uint2(d ? (uint32_t)(rng() % 9 == 0 ? 0 : rng() % (d + 1)) : 0u, (uint32_t)d));
        }
    }
    J.launches.push_back(list_launch(LIST, rc, cnt));
    return J;
}

static void case_lists()
{
    check("list form, full rows: every rule denominator is s", list_job(64, 80, 5, 1, false));
    check("list form, short rows: both binnings differ", list_job(64, 150, 9, 2, true));
    check("list form, s = 1000", list_job(1000, 90, 20, 3, true));
    Job J = list_job(64, 3, 1, 4, false);
    check("list form, two entries", J);
}

static void case_sizes()
{
    for (uint32_t s : {64u, 1000u, 16383u, 16384u, 20000u}) {            // LDS bins up to 16 383, memory beyond
        Launch L = flat_launch(MARKED, 0, 70, make_uint2(0, s));
        junk_fill(L, s);
        for (uint64_t i = 0; i < L.pairs; i++)
            if (i % 3) mark(L, i, i % 50 == 0 ? s : (uint32_t)(i * 2654435761u % (s + 1)), i % 10 == 3 ? s - 1 : s);
        check("marked, s = " + std::to_string(s), one(s, L));
        Launch A = flat_launch(ALL, 0, 70, make_uint2(0, s));
        for (uint64_t i = 0; i < A.pairs; i += 2) A.counts[i] = make_uint2((uint32_t)(i * 40503u % (s + 1)), s);
        A.counts[7] = make_uint2(s, s);
        check("all, s = " + std::to_string(s), one(s, A));
    }
}

static void case_hot()
{
    {   // every entry in s/s
        Launch L = flat_launch(MARKED, 0, 150, make_uint2(1000, 1000));
        for (uint64_t i = 0; i < L.pairs; i++) L.set(i);
        check("every marked entry in s/s", one(1000, L));
        Launch A = flat_launch(ALL, 0, 150, make_uint2(1000, 1000));
        check("every count s/s", one(1000, A));
    }
    {   // every entry in 0/s, no masks
        Launch A = flat_launch(ALL, 0, 150, make_uint2(0, 1000));
        check("every count 0/s", one(1000, A));
        A.counts[4000] = make_uint2(3, 1000);
        A.counts[4001] = make_uint2(0, 999);
        check("every count 0/s but two", one(1000, A));
    }
    {   // every entry in one key of the table
        Launch A = flat_launch(ALL, 0, 100, make_uint2(20, 40));
        check("every count 20/40", one(64, A), 0);
    }
}

static void case_denoms()
{
    static const uint32_t denoms[4] = {63, 64, 32, 0};
    Launch L = flat_launch(MARKED, 0, 90, make_uint2(0, 64));
    junk_fill(L, 64);
    for (uint64_t i = 0; i < L.pairs; i++) {
        const uint32_t d = denoms[(i / 3) % 4];
        if (i % 5 != 2) mark(L, i, d ? (uint32_t)(i % (d + 1)) : 0u, d);
    }
    check("denominators 63, 64, 32 and 0 mixed, marked", one(64, L));
    Launch A = flat_launch(ALL, 0, 90, make_uint2(0, 64));
    for (uint64_t i = 0; i < A.pairs; i++) {
        const uint32_t d = denoms[(i * 5 / 7) % 4];
        A.counts[i] = make_uint2(d ? (uint32_t)((i * 3) % (d + 1)) : 0u, d);
    }
    check("denominators 63, 64, 32 and 0 mixed, all", one(64, A));
}

static void case_regrow()
{
    Launch A = flat_launch(ALL, 0, 100, make_uint2(0, 64));
    for (uint64_t i = 0; i < A.pairs; i++) A.counts[i] = make_uint2((uint32_t)(i % 30), 30 + (uint32_t)(i % 29));
    Job J = one(64, A);
    J.slots = 4;
    check("a table started at 4 slots for some hundred keys", J, 1);
    J.launches.push_back(J.launches[0]);
    check("the same in two pieces: the second run starts from the first piece", J, 1);
    Launch B = flat_launch(ALL, 0, 20, make_uint2(1, 2));
    for (uint64_t i = 0; i < 4; i++) B.counts[i] = make_uint2((uint32_t)i, 5);
    Job K = one(64, B);
    K.slots = 4;
    check("five keys in 4 slots", K, 1);
    B.counts[3] = make_uint2(1, 2);
    Job K4 = one(64, B);
    K4.slots = 4;
    check("four keys fill 4 slots exactly", K4, 0);
}

static void fuzz(uint32_t seed, int n)
{
    std::mt19937 rng(seed);
    for (int t = 0; t < n; t++) {
        static const uint32_t sizes[5] = {64, 64, 200, 1000, 20000};
        Job J;
        J.s = sizes[rng() % 5];
        J.slots = rng() % 2 ? 4 : rng() % 2 ? 64 : 1024;
        const bool others = rng() % 3 != 0;                         // denominators below s among the counts
        const uint32_t spread = others ? 1 + rng() % 40 : 0;
        auto counts = [&](uint32_t) {
            const uint32_t d = spread && rng() % 4 == 0 ? J.s - 1 - rng() % spread : J.s;
            const uint32_t hot = rng() % 3;
            return make_uint2(hot == 0 ? 0u : hot == 1 ? rng() % (d + 1) : d / 2, d);
        };
        const int launches = 1 + rng() % 3;
        const int form = rng() % 3;
        if (form == 2) {
            J = list_job(J.s, 20 + rng() % 200, 1 + rng() % 12, rng(), others);
            J.slots = rng() % 2 ? 4 : 1024;
        } else {
            const uint64_t rows = 2 + rng() % 250;
            for (int p = 0; p < launches; p++) {
                const uint64_t r0 = p ? rows * p / launches : 0, r1 = rows * (p + 1) / launches;
                if (tri(r1) == tri(r0)) continue;
                Launch L = flat_launch(form ? ALL : MARKED, r0, r1, make_uint2(0, J.s));
                const uint32_t density = 1 + rng() % 8;
                for (uint64_t i = 0; i < L.pairs; i++) {
                    const uint2 c = counts(0);
                    if (L.kind == ALL) L.counts[i] = c;
                    else if (rng() % density == 0) mark(L, i, c.x, c.y);
                    else L.counts[i] = junk(i, J.s);
                }
                if (L.kind == MARKED && rng() % 4 == 0) L.sp = PairSpace{(uint32_t)(rng() % (rows + 1)), (uint32_t)(rng() % (rows + 1)), 0u, 0u};
                J.launches.push_back(L);
            }
        }
        check("fuzz " + std::to_string(t) + " (s = " + std::to_string(J.s) + ", form " + std::to_string(form) + ")", J);
    }
}

int main(int argc, char **argv)
{
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "small") case_small();
    else if (c == "lengths") case_lengths();
    else if (c == "words") case_words();
    else if (c == "space") case_space();
    else if (c == "pieces") case_pieces();
    else if (c == "lists") case_lists();
    else if (c == "sizes") case_sizes();
    else if (c == "hot") case_hot();
    else if (c == "denoms") case_denoms();
    else if (c == "regrow") case_regrow();
    else if (c == "fuzz" && argc > 3) fuzz((uint32_t)strtoul(argv[2], nullptr, 10), atoi(argv[3]));
    else { fprintf(stderr, "usage: spectrum_emu <case> | fuzz <seed> <n>\n"); return 2; }
    if (failures) { printf("%d FAILED\n", failures); return 1; }
    printf("all cases agree\n");
    return 0;
}
