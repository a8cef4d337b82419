// index_rowmap_emu_main.cpp -- the index build THROUGH A ROW MAP on host threads (tools/hipemu): for a table T and a map pi,
// index_build_mapped on (T, pi) must leave every array word for word equal to index_build on the materialised copy
// C[a] = T[pi[a]] -- values, rows, group starts and ends, both images, the statistics and flags, the window offsets, and the
// partition's scratch (block counts, bucket starts, packed entries).  index_window_offsets (K0 ahead of the build, counts in the
// TABLE's order) must leave the same window offsets.  TEST INFRASTRUCTURE (tests/test_index_emu_rowmap.py); built with g++.
//
//   index_rowmap_emu <map> <windows>     map: identity | reversal | random;  windows: one | several;  exit status 0 = equal
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
    const uint64_t top = 1ull << 53, common = (1ull << 52) + 12345u;       // (below 2^53: one bucket can hold every value beside 11 bits of row)
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

int main(int argc, char **argv)
{
    const std::string map = argc > 1 ? argv[1] : "random", windows = argc > 2 ? argv[2] : "several";
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
    // the materialised copy, its offsets, what the plan asks of the rows
    std::vector<uint64_t> C((size_t)N * STRIDE);
    std::vector<uint32_t> off(N + 1, 0);
    uint64_t maxv = 0;
    double dens0 = 0;
    for (uint32_t a = 0; a < N; a++) {
        std::copy(t.H.begin() + (size_t)pi[a] * STRIDE, t.H.begin() + (size_t)(pi[a] + 1) * STRIDE, C.begin() + (size_t)a * STRIDE);
        const uint32_t c = t.cnt[pi[a]];
        off[a + 1] = off[a] + c;
        if (c) {
            const uint64_t last = C[(size_t)a * STRIDE + c - 1];
            maxv = std::max(maxv, last);
            dens0 += (double)c / ((double)last + 1.0);
        }
    }
    const uint32_t E = off[N], rs = ((S + 3u) & ~3u) + 4u;
    // one window: a bucket so wide that it holds every value; several: the plan's own width
    const IxPlan plan = index_plan(N, E, S, rs, STRIDE, maxv, windows == "one" ? dens0 * 1e-4 : dens0, true);
    if (!plan.ok) { printf("plan refused: %s\n", plan.why); return 1; }
    if ((windows == "one") != (plan.g.NW == 1)) { printf("%u windows, asked for %s\n", plan.g.NW, windows.c_str()); return 1; }
    Out m(plan, E, rs), u(plan, E, rs);
    if (build(plan, t.H.data(), pi.data(), off.data(), m, 7) != hipSuccess || build(plan, C.data(), nullptr, off.data(), u, 7) != hipSuccess) {
        printf("a build failed\n");
        return 1;
    }
    int bad = 0;
    auto same = [&](const char *what, const void *a, const void *b, size_t bytes) {
        if (memcmp(a, b, bytes) != 0) { printf("  %s differ\n", what); bad++; }
    };
    same("window offsets (lb)", m.lb.data(), u.lb.data(), m.lb.size());
    same("block counts", m.cnt.data(), u.cnt.data(), m.cnt.size());
    same("bucket starts", m.start.data(), u.start.data(), m.start.size());
    same("packed entries", m.pk.data(), u.pk.data(), m.pk.size());
    same("values", m.keys.data(), u.keys.data(), (size_t)E * 8);
    same("rows", m.rows.data(), u.rows.data(), (size_t)E * 4);
    same("group starts", m.gs.data(), u.gs.data(), (size_t)E * 4);
    same("group ends", m.gend.data(), u.gend.data(), (size_t)E * 4);
    same("code image", m.code.data(), u.code.data(), m.code.size() * 4);
    same("position image", m.pos.data(), u.pos.data(), m.pos.size() * 4);
    same("flags", m.flags, u.flags, sizeof m.flags);
    if (m.inc != u.inc || m.max_group != u.max_group || m.groups != u.groups) { printf("  statistics differ\n"); bad++; }
    // the unmapped build is an index at all: the value of 300 rows is one group of 300 (short rows may have lost it: at least 250)
    if (u.flags[IXF_DEGENERATE] || u.max_group < 250 || u.max_group > 300 || u.groups == 0) { printf("  not the index expected: largest group %u\n", u.max_group); bad++; }
    {   // K0 ahead of the build: counts in the table's order, the same window offsets; the build that takes them (stage bit 8)
        Out k(plan, E, rs);
        if (index_window_offsets(plan, t.H.data(), pi.data(), t.cnt.data(), k.lb.data(), nullptr) != hipSuccess) { printf("  index_window_offsets failed\n"); bad++; }
        same("window offsets made ahead", k.lb.data(), u.lb.data(), k.lb.size());
        if (build(plan, t.H.data(), pi.data(), off.data(), k, 1 | 8) != hipSuccess) { printf("  the partition behind them failed\n"); bad++; }
        same("packed entries behind them", k.pk.data(), u.pk.data(), k.pk.size());
    }
    printf("map %s, %s: n %u s %u stride %llu E %u shift %u B %u BW %u NW %u fullest %u big %u: %s\n", map.c_str(), windows.c_str(), N, S,
           (unsigned long long)STRIDE, E, plan.g.shift, plan.g.Bp, plan.g.BW, plan.g.NW, u.flags[IXF_MAXBUCKET], u.flags[IXF_NBIG], bad ? "MISMATCH" : "equal");
    return bad ? 1 : 0;
}
