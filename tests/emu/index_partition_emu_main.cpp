// index_partition_emu_main.cpp -- K3 (index_build.hip: the tile partition) on host threads (tools/hipemu), both bodies: the
// ranks taken in registers (ix_tile_partition_kernel) and the LSD sort in LDS (ix_tile_partition_lsd_kernel).  Stage 1 of the
// build (K0 - K3) runs once per body; pk and the slot image (the position image as K3 leaves it) must be equal word for word,
// between the bodies and to a std::stable_sort statement: by bucket, then row, then position.
// TEST INFRASTRUCTURE (tests/test_index_partition_emu.py); built with g++.
//
//   index_partition_emu table <map> <windows>     map: identity | reversal | random;  windows: one | several
//   index_partition_emu long | runs | bw1 | bw2 | bw512 | one_tile                     exit status 0 = as expected
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <random>
#include <string>

#include "../../mash_amd/csrc/index_build.hip"

using namespace mg;

struct Case {
    IxPlan plan;
    uint32_t n = 0;
    uint64_t stride = 0;
    std::vector<uint64_t> H;          // n x stride, ascending rows, padding ~0 (the TABLE's order)
    std::vector<uint32_t> cnt;        // the table rows' entry counts
    std::vector<uint32_t> pi;         // index row a is table row pi[a] (empty: identity)
};

struct Out {
    std::vector<unsigned char> lb, cnt, start, big;
    std::vector<uint64_t> pk;
    std::vector<uint32_t> img;
    uint32_t flags[4] = {0, 0, 0, 0};
    Out(const IxPlan &p, uint32_t n)
        : lb(p.lb_bytes + 16, 0xAB), cnt(p.cnt_bytes + 16, 0xAB), start(p.start_bytes + 16, 0xAB), big(p.big_bytes + 16, 0xAB), pk((size_t)p.g.E + 2, 0xDEADDEADDEADull),
          img((size_t)n * p.g.rs + 4, 0xDEADu)
    {}
};

static int run_case(const char *name, const Case &c)
{
    const IxGeom &g = c.plan.g;
    const uint32_t n = c.n;
    std::vector<uint32_t> off(n + 1, 0);
    for (uint32_t a = 0; a < n; a++) off[a + 1] = off[a] + c.cnt[c.pi.empty() ? a : c.pi[a]];
    if (off[n] != g.E) { printf("%s: the plan speaks of %u entries, the table holds %u\n", name, g.E, off[n]); return 1; }
    const uint32_t *rowmap = c.pi.empty() ? nullptr : c.pi.data();
    // the statement: every entry in (row, position) order, sorted by bucket and by nothing else
    struct Ent { uint32_t bucket, row, pos; uint64_t word; };
    std::vector<Ent> ent;
    ent.reserve(g.E);
    const uint64_t lowmask = (1ull << g.shift) - 1ull;
    for (uint32_t a = 0; a < n; a++) {
        const uint32_t tr = c.pi.empty() ? a : c.pi[a];
        for (uint32_t p = 0; p < c.cnt[tr]; p++) {
            const uint64_t v = c.H[(size_t)tr * c.stride + p];
            ent.push_back(Ent{(uint32_t)(v >> g.shift), a, p, ((v & lowmask) << g.rb) | a});
        }
    }
    std::stable_sort(ent.begin(), ent.end(), [](const Ent &x, const Ent &y) { return x.bucket < y.bucket; });
    Out want(c.plan, n);
    uint32_t fullest_piece = 0, longest = 0;
    for (uint32_t i = 0; i < ent.size(); i++) {
        want.pk[i] = ent[i].word;
        want.img[(size_t)ent[i].row * g.rs + ent[i].pos] = i;
    }
    for (uint32_t a = 0; a < n; a++) longest = std::max(longest, off[a + 1] - off[a]);
    int bad = 0;
    Out o[2] = {Out(c.plan, n), Out(c.plan, n)};
    static const char *body[2] = {"lsd", "rank"};
    for (int b = 0; b < 2; b++) {
        const hipError_t e = index_build_mapped(c.plan, c.H.data(), rowmap, off.data(), o[b].lb.data(), o[b].cnt.data(), o[b].start.data(), o[b].big.data(), o[b].pk.data(),
                                                nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, o[b].img.data(), nullptr, nullptr, nullptr, nullptr, o[b].flags, nullptr,
                                                nullptr, 1, nullptr, b == 0 ? IX_PART_LSD : IX_PART_RANK);
        if (e != hipSuccess) { printf("%s: the build (%s) failed\n", name, body[b]); return 1; }
        if (o[b].pk != want.pk) { printf("  %s: pk differs from the statement\n", body[b]); bad++; }
        if (o[b].img != want.img) { printf("  %s: the slot image differs from the statement\n", body[b]); bad++; }
    }
    if (o[0].pk != o[1].pk || o[0].img != o[1].img) { printf("  the bodies differ\n"); bad++; }
    {   // (what the case is: the fullest tile, in entries)
        const uint32_t *cn = reinterpret_cast<const uint32_t *>(o[1].cnt.data()), *st = reinterpret_cast<const uint32_t *>(o[1].start.data());
        for (uint32_t blk = 0; blk < g.nblk; blk++)
            for (uint32_t w = 0; w < g.NW; w++) {
                const uint32_t b0 = w * g.BW, b1 = b0 + g.BW;      // the block's entries of the window: from its prefixes
                uint32_t t = 0;
                for (uint32_t b = b0; b < b1; b++) {
                    const uint32_t nx = blk + 1 < g.nblk ? cn[(size_t)(blk + 1) * g.Bp + b] : st[b + 1] - st[b];
                    t += nx - cn[(size_t)blk * g.Bp + b];
                }
                fullest_piece = std::max(fullest_piece, t);
            }
    }
    printf("%s: n %u E %u shift %u BW %u NW %u passes %u, fullest tile %u entries (%u at a time), longest row %u: %s\n", name, n, g.E, g.shift, g.BW, g.NW, g.npass,
           fullest_piece, IX_PCAP, longest, bad ? "MISMATCH" : "equal");
    return bad ? 1 : 0;
}

// ---- n = 1 100 rows (two full blocks of 512 and a ragged third), s = 96 in rows of stride 104; full, short and empty rows; one
// value held by 300 rows; the plan is index_plan's
static int table_case(const std::string &map, const std::string &windows)
{
    const uint32_t N = 1100, S = 96;
    Case c;
    c.n = N;
    c.stride = 104;
    c.H.assign((size_t)N * c.stride, ~0ull);
    c.cnt.assign(N, 0);
    std::mt19937_64 rng(20251019);
    const uint64_t top = 1ull << 53, common = (1ull << 52) + 12345u;
    for (uint32_t r = 0; r < N; r++) {
        uint32_t k = S;
        if (r % 11 == 5) k = 0;
        else if (r % 7 == 3) k = 1 + (uint32_t)(rng() % (S - 1));
        std::vector<uint64_t> v;
        if (k && r < 900 && r % 3 == 0) v.push_back(common);
        while (v.size() < k) v.push_back(rng() % top);
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        c.cnt[r] = (uint32_t)v.size();
        std::copy(v.begin(), v.end(), c.H.begin() + (size_t)r * c.stride);
    }
    if (map != "identity") {
        c.pi.resize(N);
        for (uint32_t a = 0; a < N; a++) c.pi[a] = N - 1 - a;
        if (map == "random") {
            std::mt19937_64 r2(7);
            std::shuffle(c.pi.begin(), c.pi.end(), r2);
        } else if (map != "reversal") {
            printf("unknown map %s\n", map.c_str());
            return 2;
        }
    }
    uint64_t maxv = 0;
    double dens0 = 0;
    uint32_t E = 0;
    for (uint32_t r = 0; r < N; r++)
        if (c.cnt[r]) {
            const uint64_t last = c.H[(size_t)r * c.stride + c.cnt[r] - 1];
            maxv = std::max(maxv, last);
            dens0 += (double)c.cnt[r] / ((double)last + 1.0);
            E += c.cnt[r];
        }
    // one window: a bucket so wide that it holds every value (a tile of a full block is 49 000 entries, 14 pieces)
    c.plan = index_plan(N, E, S, ((S + 3u) & ~3u) + 4u, c.stride, maxv, windows == "one" ? dens0 * 1e-4 : dens0, true);
    if (!c.plan.ok) { printf("plan refused: %s\n", c.plan.why); return 1; }
    if ((windows == "one") != (c.plan.g.NW == 1)) { printf("%u windows, asked for %s\n", c.plan.g.NW, windows.c_str()); return 1; }
    return run_case(("table " + map + " " + windows).c_str(), c);
}

// ---- hand-made geometries: NW windows of 2^bw_log buckets of 2^shift values
static void geometry(Case &c, uint32_t n, uint64_t stride, uint32_t shift, uint32_t bw_log, uint32_t NW)
{
    c.n = n;
    c.stride = stride;
    c.H.assign((size_t)n * stride, ~0ull);
    c.cnt.assign(n, 0);
    IxGeom &g = c.plan.g;
    g = IxGeom{};
    g.n = n;
    g.nblk = (n + IX_RB - 1u) / IX_RB;
    g.shift = shift;
    g.bw_log = bw_log;
    g.BW = 1u << bw_log;
    g.NW = NW;
    g.Bp = NW * g.BW;
    g.rb = 1;
    while ((1u << g.rb) < n) g.rb++;
    g.npass = (bw_log + 3u) / 4u;
    g.wgrp = 8;
    g.nseq = (NW + 7u) / 8u * 8u * g.nblk;
    g.rs = (uint32_t)stride + 4u;
    g.stride = stride;
}

static void finish(Case &c)
{
    IxGeom &g = c.plan.g;
    uint32_t E = 0;
    for (uint32_t r = 0; r < c.n; r++) {
        uint64_t *row = &c.H[(size_t)r * c.stride];
        std::sort(row, row + c.cnt[r]);
        E += c.cnt[r];
    }
    g.E = E;
    c.plan.ok = true;
    c.plan.lb_bytes = (size_t)c.n * (g.NW + 1u) * 2u;
    c.plan.cnt_bytes = (size_t)g.nblk * g.Bp * 4u;
    c.plan.start_bytes = ((size_t)g.Bp + 1u) * 4u;
    c.plan.pk_bytes = (size_t)E * 8u;
    c.plan.big_bytes = ((size_t)E / IX_CAP + 2u) * 4u;
}

// `k` values of row r in bucket b (global), distinct by a running serial
static void put(Case &c, uint32_t r, uint32_t b, uint32_t k, std::mt19937_64 &rng)
{
    const uint32_t shift = c.plan.g.shift;
    for (uint32_t x = 0; x < k; x++) {
        if (c.cnt[r] >= c.stride) { printf("row %u is full\n", r); abort(); }
        const uint32_t at = c.cnt[r]++;
        c.H[(size_t)r * c.stride + at] = ((uint64_t)b << shift) | (((rng() << 13) | at) & ((1ull << shift) - 1ull));
    }
}

// rows that cross a step (more than 64 entries in a window), a wave's share and a piece (more than IX_PCAP / 8, more than
// IX_PCAP); a window without entries; a last block of one row
static int long_case()
{
    Case c;
    geometry(c, 513, 4608, 30, 4, 4);            // windows 0 .. 3 of 16 buckets; window 3 stays empty
    std::mt19937_64 rng(11);
    for (uint32_t r = 0; r < c.n; r++) {
        if (r % 13 == 4) continue;               // (an empty row)
        for (uint32_t x = 0; x < 3 + r % 5; x++) put(c, r, (uint32_t)(rng() % 48u), 1, rng);
    }
    for (uint32_t x = 0; x < 100; x++) put(c, 5, 16 + (uint32_t)(rng() % 16u), 1, rng);          // crosses a step
    for (uint32_t x = 0; x < 700; x++) put(c, 40, 16 + (uint32_t)(rng() % 16u), 1, rng);         // crosses a wave's share
    for (uint32_t x = 0; x < 4100; x++) put(c, 300, 32 + (uint32_t)(rng() % 16u), 1, rng);       // crosses a piece, and then some
    put(c, 301, 35, 600, rng);                                                                  // (one bucket, a long row)
    put(c, 512, 17, 70, rng);                                                                   // the block of one row
    finish(c);
    return run_case("long", c);
}

// window 0: every entry of the tile in ONE bucket (9 per row: 4 608 entries, two pieces); window 1: a run of one bucket of
// 8 per row between single entries of two others -- the run crosses the waves' shares and the piece
static int runs_case()
{
    Case c;
    geometry(c, 1000, 32, 30, 4, 2);
    std::mt19937_64 rng(12);
    for (uint32_t r = 0; r < c.n; r++) {
        put(c, r, 5, 9, rng);
        put(c, r, 16 + 2, 1, rng);
        put(c, r, 16 + 3, 8, rng);
        put(c, r, 16 + 9, 1, rng);
    }
    finish(c);
    return run_case("runs", c);
}

// buckets per window: 1, 2, 512
static int bw_case(uint32_t bw_log)
{
    Case c;
    const uint32_t NW = bw_log == 9 ? 2 : 5;
    geometry(c, 700, 40, 30, bw_log, NW);
    std::mt19937_64 rng(13 + bw_log);
    for (uint32_t r = 0; r < c.n; r++) {
        const uint32_t k = r % 9 == 2 ? 0 : 5 + (uint32_t)(rng() % 30u);
        for (uint32_t x = 0; x < k; x++) put(c, r, (uint32_t)(rng() % c.plan.g.Bp), 1, rng);
    }
    finish(c);
    return run_case(bw_log == 0 ? "bw1" : bw_log == 1 ? "bw2" : "bw512", c);
}

// ONE tile (what the ThreadSanitizer build runs: work-items as OS threads): 300 rows, 8 buckets, short rows, a row across two
// steps, a run of one bucket, an empty row
static int one_tile_case()
{
    Case c;
    geometry(c, 300, 160, 30, 3, 1);
    std::mt19937_64 rng(14);
    for (uint32_t r = 0; r < c.n; r++) {
        if (r % 17 == 3) continue;
        for (uint32_t x = 0; x < 1 + r % 6; x++) put(c, r, (uint32_t)(rng() % 8u), 1, rng);
        if (r % 4 == 0) put(c, r, 6, 3, rng);
    }
    for (uint32_t x = 0; x < 150; x++) put(c, 77, (uint32_t)(rng() % 8u), 1, rng);
    finish(c);
    return run_case("one_tile", c);
}

int main(int argc, char **argv)
{
    const std::string a = argc > 1 ? argv[1] : "one_tile";
    if (a == "table") return table_case(argc > 2 ? argv[2] : "random", argc > 3 ? argv[3] : "several");
    if (a == "long") return long_case();
    if (a == "runs") return runs_case();
    if (a == "bw1") return bw_case(0);
    if (a == "bw2") return bw_case(1);
    if (a == "bw512") return bw_case(9);
    if (a == "one_tile") return one_tile_case();
    printf("unknown case %s\n", a.c_str());
    return 2;
}
