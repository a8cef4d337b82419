// index_offsets_counts_emu_main.cpp -- the window offsets and the blocks' bucket counts from ONE read of the table
// (index_build.h: index_offsets_counts, ix_offsets_counts_kernel) on host threads (tools/hipemu), against K0 + K1:
//   * lb and cnt of the fused kernel equal those of ix_window_offsets_kernel + ix_tile_count_kernel word for word, and the whole
//     build behind them (stage bits 8 | 16) equals the build that runs K0 + K1 itself in every array;
//   * a 16-bit counter that passes 65 535 raises flags[IXF_DEGENERATE], and the counts written are right all the same;
//   * the route rule: 2 Bp bytes and 64 of scratch within 160 KB.
// TEST INFRASTRUCTURE (tests/test_index_emu_offsets_counts.py); built with g++.
//
//   index_offsets_counts_emu <map> <windows>     map: identity | reversal | random;  windows: one | several
//   index_offsets_counts_emu carry
//   index_offsets_counts_emu route                                                     exit status 0 = as expected
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <random>
#include <string>

#include "../../mash_amd/csrc/index_build.hip"

using namespace mg;

// n = 1 100 rows (two full blocks of 512 and a ragged third), s = 96 in rows of stride 104; full, short and empty rows; one value
// held by 300 rows
static const uint32_t N = 1100, S = 96;
static const uint64_t STRIDE = 104;

struct Table {
    std::vector<uint64_t> H;          // N x STRIDE, ascending rows, padding ~0
    std::vector<uint32_t> cnt;
};

static Table make_table(uint64_t seed)
{
    Table t;
    t.H.assign((size_t)N * STRIDE, ~0ull);
    t.cnt.assign(N, 0);
    std::mt19937_64 rng(seed);
    const uint64_t top = 1ull << 53, common = (1ull << 52) + 12345u;
    for (uint32_t r = 0; r < N; r++) {
        uint32_t c = S;
        if (r % 11 == 5) c = 0;
        else if (r % 7 == 3) c = 1 + (uint32_t)(rng() % (S - 1));
        std::vector<uint64_t> v;
        if (c && r < 900 && r % 3 == 0) v.push_back(common);        // 300 rows, some of them short
        while (v.size() < c) v.push_back(rng() % top);
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        t.cnt[r] = (uint32_t)v.size();
        std::copy(v.begin(), v.end(), t.H.begin() + (size_t)r * STRIDE);
    }
    return t;
}

struct Out {
    std::vector<unsigned char> lb, cnt, start, pk, tc, big, stat;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> rows, gend, gs, code, pos;
    unsigned long long inc = 0;
    uint32_t max_group = 0, groups = 0, flags[4] = {0, 0, 0, 0};
    Out(const IxPlan &p, uint32_t E, uint32_t rs)
        : lb(p.lb_bytes + 16, 0xAB), cnt(p.cnt_bytes + 16, 0xAB), start(p.start_bytes + 16, 0xAB), pk(p.pk_bytes + 16, 0xAB), tc(p.tc_bytes + 16, 0xAB),
          big(p.big_bytes + 16, 0xAB), stat(index_stat_scratch_bytes()), keys(E, 0xDEADull), rows(E, 0xDEADu), gend(E, 0xDEADu), gs(E, 0xDEADu),
          code((size_t)N * rs + 64, 0xDEADu), pos((size_t)N * rs, 0xDEADu)
    {}
};

static hipError_t build(const IxPlan &plan, const uint64_t *H, const uint32_t *rowmap, const uint32_t *off, Out &o, int stages)
{
    return index_build_mapped(plan, H, rowmap, off, o.lb.data(), o.cnt.data(), o.start.data(), o.big.data(), o.pk.data(), o.tc.data(), o.keys.data(), o.rows.data(),
                              o.gend.data(), o.gs.data(), o.code.data(), o.pos.data(), o.stat.data(), &o.inc, &o.max_group, &o.groups, o.flags, nullptr, nullptr, stages);
}

static int equal_case(const std::string &map, const std::string &windows)
{
    const Table t = make_table(20251019);
    std::vector<uint32_t> pi(N);
    for (uint32_t a = 0; a < N; a++) pi[a] = map == "reversal" ? N - 1 - a : a;
    if (map == "random") {
        std::mt19937_64 rng(7);
        std::shuffle(pi.begin(), pi.end(), rng);
    } else if (map != "identity" && map != "reversal") {
        printf("unknown map %s\n", map.c_str());
        return 2;
    }
    // the index's offsets, what the plan asks of the rows
    std::vector<uint32_t> off(N + 1, 0);
    uint64_t maxv = 0;
    double dens0 = 0;
    for (uint32_t a = 0; a < N; a++) {
        const uint32_t c = t.cnt[pi[a]];
        off[a + 1] = off[a] + c;
        if (c) {
            const uint64_t last = t.H[(size_t)pi[a] * STRIDE + c - 1];
            maxv = std::max(maxv, last);
            dens0 += (double)c / ((double)last + 1.0);
        }
    }
    const uint32_t E = off[N], rs = ((S + 3u) & ~3u) + 4u;
    // one window: a bucket so wide that it holds every value; several: the plan's own width
    const IxPlan plan = index_plan(N, E, S, rs, STRIDE, maxv, windows == "one" ? dens0 * 1e-4 : dens0, true);
    if (!plan.ok) { printf("plan refused: %s\n", plan.why); return 1; }
    if ((windows == "one") != (plan.g.NW == 1)) { printf("%u windows, asked for %s\n", plan.g.NW, windows.c_str()); return 1; }
    if (!index_offsets_counts_fits(plan.g)) { printf("the plan's %u buckets do not fit\n", plan.g.Bp); return 1; }
    const uint32_t *rowmap = map == "identity" ? nullptr : pi.data();
    int bad = 0;
    auto same = [&](const char *what, const void *a, const void *b, size_t bytes) {
        if (memcmp(a, b, bytes) != 0) { printf("  %s differ\n", what); bad++; }
    };
    // K0 + K1 on their own (counts in the table's order, as the early call has them), and the fused kernel
    Out u(plan, E, rs), k(plan, E, rs), f(plan, E, rs);
    {
        const IxGeom g = plan.g;
        const uint32_t tiles = 8u * ((g.nseq + 7u) / 8u);
        hipLaunchKernelGGL(ix_window_offsets_kernel, dim3((g.n + 3u) / 4u), dim3(256), 0, nullptr, g, t.H.data(), rowmap, (const uint32_t *)nullptr, t.cnt.data(),
                           reinterpret_cast<uint16_t *>(k.lb.data()));
        hipLaunchKernelGGL(ix_tile_count_kernel, dim3(tiles), dim3(IX_NT), 0, nullptr, g, t.H.data(), rowmap, reinterpret_cast<const uint16_t *>(k.lb.data()),
                           reinterpret_cast<uint32_t *>(k.cnt.data()));
    }
    if (index_offsets_counts(plan, t.H.data(), rowmap, t.cnt.data(), f.lb.data(), f.cnt.data(), f.flags, nullptr) != hipSuccess) {
        printf("  index_offsets_counts failed\n");
        return 1;
    }
    same("window offsets (lb) of the fused kernel and K0", f.lb.data(), k.lb.data(), f.lb.size());
    same("block counts of the fused kernel and K1", f.cnt.data(), k.cnt.data(), f.cnt.size());
    if (f.flags[IXF_DEGENERATE]) { printf("  the fused kernel raised the flag on an ordinary table\n"); bad++; }
    // the build behind the fused kernel against the build that runs K0 + K1 itself
    if (build(plan, t.H.data(), rowmap, off.data(), u, 7) != hipSuccess || build(plan, t.H.data(), rowmap, off.data(), f, 7 | 8 | 16) != hipSuccess) {
        printf("a build failed\n");
        return 1;
    }
    same("window offsets (lb)", f.lb.data(), u.lb.data(), f.lb.size());
    same("block counts (prefixes)", f.cnt.data(), u.cnt.data(), f.cnt.size());
    same("bucket starts", f.start.data(), u.start.data(), f.start.size());
    same("packed entries", f.pk.data(), u.pk.data(), f.pk.size());
    same("{code, position} by arrival", f.tc.data(), u.tc.data(), f.tc.size());
    same("values", f.keys.data(), u.keys.data(), (size_t)E * 8);
    same("rows", f.rows.data(), u.rows.data(), (size_t)E * 4);
    same("group starts", f.gs.data(), u.gs.data(), (size_t)E * 4);
    same("group ends", f.gend.data(), u.gend.data(), (size_t)E * 4);
    same("code image", f.code.data(), u.code.data(), f.code.size() * 4);
    same("position image", f.pos.data(), u.pos.data(), f.pos.size() * 4);
    same("flags", f.flags, u.flags, sizeof f.flags);
    if (f.inc != u.inc || f.max_group != u.max_group || f.groups != u.groups) { printf("  statistics differ\n"); bad++; }
    if (u.flags[IXF_DEGENERATE] || u.max_group < 250 || u.max_group > 300 || u.groups == 0) { printf("  not the index expected: largest group %u\n", u.max_group); bad++; }
    printf("map %s, %s: n %u s %u stride %llu E %u shift %u B %u BW %u NW %u fullest %u: %s\n", map.c_str(), windows.c_str(), N, S, (unsigned long long)STRIDE, E,
           plan.g.shift, plan.g.Bp, plan.g.BW, plan.g.NW, u.flags[IXF_MAXBUCKET], bad ? "MISMATCH" : "equal");
    return bad ? 1 : 0;
}

// 512 equal rows of s = 160 under a hand-made geometry (16 buckets of 2^40 values, 4 windows of 4): 130 values of every row
// in bucket 6, 30 in bucket 7 -- 66 560 entries in the LOW half of a word, which carries into the high half (bucket 7)
static int carry_case()
{
    const uint32_t n = 512, s = 160;
    IxPlan plan;
    IxGeom &g = plan.g;
    g = IxGeom{};
    g.n = n; g.nblk = 1; g.E = n * s; g.shift = 40; g.bw_log = 2; g.BW = 4; g.NW = 4; g.Bp = 16; g.rb = 9; g.npass = 1; g.wgrp = 8; g.nseq = 8; g.rs = s + 4;
    g.stride = s;
    plan.ok = true;
    std::vector<uint64_t> H((size_t)n * s);
    std::vector<uint32_t> cnt_table(n, s);
    for (uint32_t r = 0; r < n; r++)
        for (uint32_t p = 0; p < s; p++) H[(size_t)r * s + p] = p < 130 ? (6ull << 40) + 1000u * p : (7ull << 40) + 1000u * (p - 130);
    std::vector<uint16_t> lb((size_t)n * (g.NW + 1u), 0xABAB);
    std::vector<uint32_t> cnt(g.Bp, 0xABABABABu);
    uint32_t flags[4] = {0, 0, 0, 0};
    if (index_offsets_counts(plan, H.data(), nullptr, cnt_table.data(), lb.data(), cnt.data(), flags, nullptr) != hipSuccess) {
        printf("index_offsets_counts failed\n");
        return 1;
    }
    int bad = 0;
    if (flags[IXF_DEGENERATE] != 1u) { printf("  a counter passed 65 535 and flags[IXF_DEGENERATE] is %u\n", flags[IXF_DEGENERATE]); bad++; }
    for (uint32_t b = 0; b < g.Bp; b++) {
        const uint32_t want = b == 6 ? 130u * n : b == 7 ? 30u * n : 0u;
        if (cnt[b] != want) { printf("  bucket %u: %u entries counted, %u there\n", b, cnt[b], want); bad++; }
    }
    for (uint32_t r = 0; r < n; r++) {                   // windows 0, 1 at position 0; the row's only window is 1; behind it the count
        const uint16_t *o = &lb[(size_t)r * (g.NW + 1u)];
        if (o[0] != 0 || o[1] != 0 || o[2] != s || o[3] != s || o[4] != s) { printf("  row %u: window offsets %u %u %u %u %u\n", r, o[0], o[1], o[2], o[3], o[4]); bad++; break; }
    }
    printf("carry: %u rows x %u entries, buckets 6 and 7: flag %u, counted %u + %u: %s\n", n, s, flags[IXF_DEGENERATE], cnt[6], cnt[7], bad ? "MISMATCH" : "caught");
    return bad ? 1 : 0;
}

// the fused kernel where 2 Bp bytes of counters and 64 bytes of scratch fit 160 KB, K0 + K1 above
static int route_case()
{
    const uint32_t fits = (160u * 1024u - 64u) / 2u;      // 81 888 buckets
    IxPlan plan;
    plan.g = IxGeom{};
    plan.ok = true;
    int bad = 0;
    plan.g.Bp = fits;
    if (!index_offsets_counts_fits(plan.g)) { printf("  %u buckets refused\n", fits); bad++; }
    plan.g.Bp = fits + 1u;
    if (index_offsets_counts_fits(plan.g)) { printf("  %u buckets accepted\n", fits + 1u); bad++; }
    plan.g.Bp = 450000u;                                  // (a table like C5)
    if (index_offsets_counts_fits(plan.g)) { printf("  450 000 buckets accepted\n"); bad++; }
    // (above the limit nothing is launched: n = 0 rows would be no launch either way, the call has to say so itself)
    if (index_offsets_counts(plan, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != hipErrorInvalidValue) { printf("  a launch above the limit\n"); bad++; }
    printf("route: fused up to %u buckets, tiles above: %s\n", fits, bad ? "MISMATCH" : "as stated");
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    const std::string a = argc > 1 ? argv[1] : "random";
    if (a == "carry") return carry_case();
    if (a == "route") return route_case();
    return equal_case(a, argc > 2 ? argv[2] : "several");
}
