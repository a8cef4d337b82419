// discover_rowflags_emu_main.cpp -- the rows' flags for discovery (SparseArgs::row_any) on host threads (tools/hipemu): the index
// of a few hundred rows is built by index_build.hip (K5 writes the flags), the dense groups' rows are encoded by
// compare_dense.hip (dn_encode_kernel<1> and <8> clip their runs and write their flags again), and after each of the two steps
// every row's flag must equal what a plain loop over the images says: an entry p < cnt with code / 2 != position.
// The table: unrelated rows; clades of 16 - 40 near-copies (dense groups); two clades with values planted across them; rows
// outside every group that share values with clade rows and with each other; a row whose only non-empty run is its last entry
// and one whose only one is its first (the first of them short: its count no multiple of 32); empty rows (what a copy of an
// earlier row is to the index); a ragged last block of rows.
// TEST INFRASTRUCTURE (tests/test_discover_rowflags_emu.py); built with g++.
//
//   discover_rowflags_emu [seed]                                                       exit status 0 = as expected
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../mash_amd/csrc/index_build.hip"
#include "../../mash_amd/csrc/compare_dense.hip"

using namespace mg;

static const uint32_t S = 100;                            // (rows of 100 entries: four pieces of 32 positions, the last one ragged)
static const uint64_t STRIDE = 104;
static const uint64_t TOP = 1ull << 53;

struct Table {
    std::vector<std::vector<uint64_t>> rows;              // ascending, distinct, at most S values each
    std::vector<std::pair<uint32_t, uint32_t>> groups;    // the clades: row intervals [g0, g1)
    std::vector<uint32_t> expect0, expect1;               // rows whose flag is known by construction, behind the encode
    std::vector<uint32_t> cleared;                        // rows flagged by K5 whose flag the encode must clear
    uint32_t last_only = 0, first_only = 0;
};

static std::vector<uint64_t> finish_row(std::vector<uint64_t> v, size_t keep)
{
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    if (v.size() > keep) v.resize(keep);
    return v;
}

static Table make_table(uint64_t seed)
{
    Table t;
    std::mt19937_64 rng(seed);
    std::set<uint64_t> used;
    auto fresh = [&](uint64_t lo, uint64_t hi) {          // a value nobody holds yet
        for (;;) {
            const uint64_t v = lo + rng() % (hi - lo);
            if (used.insert(v).second) return v;
        }
    };
    auto single = [&](size_t c) {
        std::vector<uint64_t> v;
        while (v.size() < c) v.push_back(fresh(1000, TOP));
        t.rows.push_back(finish_row(v, S));
        return (uint32_t)t.rows.size() - 1u;
    };
    // a clade: rows keep 90 % of a pool of their own and add private values -- the universe is the pool, a hundred values
    auto clade = [&](uint32_t m) {
        std::vector<uint64_t> pool;
        for (uint32_t k = 0; k < S; k++) pool.push_back(fresh(1000, TOP));
        const uint32_t g0 = (uint32_t)t.rows.size();
        for (uint32_t i = 0; i < m; i++) {
            std::vector<uint64_t> v;
            for (uint64_t x : pool)
                if (rng() % 10 != 0) v.push_back(x);
            for (uint32_t k = 0; k < 8; k++) v.push_back(fresh(1000, TOP));
            t.rows.push_back(finish_row(v, S));
        }
        t.groups.push_back({g0, (uint32_t)t.rows.size()});
    };
    for (int k = 0; k < 40; k++) t.expect0.push_back(single(S));                     // unrelated rows
    t.expect0.push_back(single(0));                                                  // an empty row
    clade(16);                                                                       // a clade on its own: every flag cleared
    for (uint32_t r = t.groups[0].first + 1; r < t.groups[0].second; r++) t.cleared.push_back(r);
    for (int k = 0; k < 30; k++) t.expect0.push_back(single(S));
    clade(40);
    for (uint32_t r = t.groups[1].first + 1; r < t.groups[1].second; r++) t.cleared.push_back(r);
    for (int k = 0; k < 300; k++) t.expect0.push_back(single(k % 9 == 4 ? 1 + rng() % (S - 1) : S));
    clade(24);                                                                       // two clades with values planted across them
    clade(33);
    {
        const auto A = t.groups[2], B = t.groups[3];
        for (int k = 0; k < 5; k++) {
            const uint64_t v = fresh(1000, TOP);
            const uint32_t a = A.first + (uint32_t)(rng() % (A.second - A.first)), b = B.first + (uint32_t)(rng() % (B.second - B.first));
            for (uint32_t r : {a, b}) {                                              // (in place of the row's largest value: counts stay)
                auto &row = t.rows[r];
                if (row.size() >= S) row.pop_back();
                row.push_back(v);
                row = finish_row(row, S);
            }
            t.expect1.push_back(b);                                                  // the later holder keeps a run outside its group
        }
    }
    // rows outside every group that share values with clade rows and with each other
    {
        const uint32_t x = single(S - 3), y = single(S - 3);
        const uint64_t both = fresh(1000, TOP);
        t.rows[x].push_back(both);
        t.rows[y].push_back(both);
        t.rows[x].push_back(t.rows[t.groups[1].first + 3][10]);
        t.rows[y].push_back(t.rows[t.groups[3].first + 2][20]);
        t.rows[x] = finish_row(t.rows[x], S);
        t.rows[y] = finish_row(t.rows[y], S);
        t.expect1.push_back(x);
        t.expect1.push_back(y);
    }
    // the only non-empty run is the row's LAST entry (a short row: 45 entries), and the row's FIRST entry
    {
        const uint32_t early = t.expect0[3];
        std::vector<uint64_t> v;
        const uint64_t big = t.rows[early].back(), small = t.rows[early].front();
        while (v.size() < 44) v.push_back(fresh(1000, big));
        v.push_back(big);
        t.rows.push_back(finish_row(v, S));
        t.last_only = (uint32_t)t.rows.size() - 1u;
        v.clear();
        v.push_back(small);
        while (v.size() < S) v.push_back(fresh(small + 1, TOP));
        t.rows.push_back(finish_row(v, S));
        t.first_only = (uint32_t)t.rows.size() - 1u;
        t.expect1.push_back(t.last_only);
        t.expect1.push_back(t.first_only);
    }
    for (int k = 0; k < 101; k++) t.expect0.push_back(single(S));                    // (the last block of 512 rows: ragged, no multiple of 8)
    return t;
}

// what discovery would find by scanning: an entry of the row with a non-empty run
static std::vector<uint32_t> scan_flags(const std::vector<uint32_t> &off, const std::vector<uint32_t> &code, const std::vector<uint32_t> &pos, uint32_t rs)
{
    const uint32_t n = (uint32_t)off.size() - 1u;
    std::vector<uint32_t> f(n, 0);
    for (uint32_t r = 0; r < n; r++)
        for (uint32_t p = 0; p < off[r + 1] - off[r]; p++)
            if ((code[(size_t)r * rs + p] >> 1) != pos[(size_t)r * rs + p]) f[r] = 1;
    return f;
}

static int compare_flags(const char *what, const std::vector<uint32_t> &got, const std::vector<uint32_t> &want)
{
    int bad = 0;
    for (size_t r = 0; r < want.size(); r++)
        if ((got[r] != 0) != (want[r] != 0) && bad++ < 8) printf("  %s: row %zu has flag %u, its images say %u\n", what, r, got[r], want[r]);
    return bad;
}

template <uint32_t EK> static void run_encode(uint32_t n, size_t smem, const uint32_t *off, const uint32_t *code, uint32_t *pos, uint32_t rs,
                                              const uint32_t *grp_of, const DenseGroup *groups, const uint32_t *ulist, const uint32_t *upos,
                                              unsigned long long *gdata, uint32_t wmax, uint16_t *ext, uint32_t xs, uint32_t *row_any)
{
    hipLaunchKernelGGL(dn_encode_kernel<EK>, dim3((n + 63u) & ~63u), dim3(256), smem, nullptr, off, code, pos, rs, grp_of, groups, ulist, upos, gdata, wmax, ext,
                       xs, n, DnEncodeOpts(1u, row_any));
}

int main(int argc, char **argv)
{
    const Table t = make_table(argc > 1 ? strtoull(argv[1], nullptr, 10) : 20261021);
    const uint32_t n = (uint32_t)t.rows.size();
    std::vector<uint64_t> H((size_t)n * STRIDE, ~0ull);
    std::vector<uint32_t> off(n + 1, 0);
    uint64_t maxv = 0;
    double dens0 = 0;
    for (uint32_t r = 0; r < n; r++) {
        const auto &row = t.rows[r];
        std::copy(row.begin(), row.end(), H.begin() + (size_t)r * STRIDE);
        off[r + 1] = off[r] + (uint32_t)row.size();
        if (!row.empty()) {
            maxv = std::max(maxv, row.back());
            dens0 += (double)row.size() / ((double)row.back() + 1.0);
        }
    }
    const uint32_t E = off[n], rs = ((S + 3u) & ~3u) + 4u;
    const IxPlan plan = index_plan(n, E, S, rs, STRIDE, maxv, dens0, true);
    if (!plan.ok) { printf("plan refused: %s\n", plan.why); return 1; }
    // ---- the index, K5 with the flags
    std::vector<unsigned char> lb(plan.lb_bytes + 16), cnt(plan.cnt_bytes + 16), start(plan.start_bytes + 16), pk(plan.pk_bytes + 16), tc(plan.tc_bytes + 16),
        big(plan.big_bytes + 16), stat(index_stat_scratch_bytes());
    std::vector<uint64_t> keys(E);
    std::vector<uint32_t> rows(E), gend(E), gs(E), code((size_t)n * rs + 64, 0xDEADu), pos((size_t)n * rs, 0xDEADu), row_any(n, 0xABABABABu);
    unsigned long long inc = 0;
    uint32_t max_group = 0, ngroups = 0, flags[4] = {0, 0, 0, 0};
    if (index_build(plan, H.data(), off.data(), lb.data(), cnt.data(), start.data(), big.data(), pk.data(), tc.data(), keys.data(), rows.data(), gend.data(), gs.data(),
                    code.data(), pos.data(), stat.data(), &inc, &max_group, &ngroups, flags, nullptr, nullptr, 7, row_any.data()) != hipSuccess ||
        flags[IXF_DEGENERATE]) {
        printf("the build failed\n");
        return 1;
    }
    int bad = 0;
    const std::vector<uint32_t> k5 = row_any;
    bad += compare_flags("behind K5", k5, scan_flags(off, code, pos, rs));
    for (uint32_t r : t.cleared)
        if (!k5[r]) { printf("  behind K5: row %u of a clade is not flagged\n", r); bad++; }
    // ---- the clades as dense groups: universes and leaders from the sorted index (a value with two holders and more inside a group)
    std::vector<uint32_t> grp_of(n, 0xFFFFFFFFu);
    std::vector<DenseGroup> groups;
    for (auto &g : t.groups) {
        DenseGroup G{};
        G.g0 = g.first;
        G.g1 = g.second;
        for (uint32_t r = G.g0; r < G.g1; r++) grp_of[r] = (uint32_t)groups.size();
        groups.push_back(G);
    }
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> uni(groups.size());      // per group {run start, leader's position}
    for (uint32_t q = 0; q < E;) {
        const uint32_t z = gend[q];
        for (uint32_t x = q; x < z;) {                      // (rows ascend inside a value: a group's holders stand side by side)
            const uint32_t g = grp_of[rows[x]];
            uint32_t y = x + 1;
            while (y < z && grp_of[rows[y]] == g) y++;
            if (g != 0xFFFFFFFFu && y - x >= 2) uni[g].push_back({q, x});
            x = y;
        }
        q = z;
    }
    std::vector<uint32_t> ulist, upos;
    uint32_t xrows = 0, wmax = 0;
    uint64_t words = 0;
    for (size_t g = 0; g < groups.size(); g++) {
        DenseGroup &G = groups[g];
        G.ustart = (uint32_t)ulist.size();
        G.u = (uint32_t)uni[g].size();
        if (G.u < 32u) { printf("  group %zu has a universe of %u values\n", g, G.u); bad++; }
        for (auto &x : uni[g]) { ulist.push_back(x.first); upos.push_back(x.second); }
        G.W = (G.u >> 6) + 1u;
        G.xrow0 = xrows;
        G.data_off = words;
        const uint64_t m = G.g1 - G.g0;
        xrows += (uint32_t)m;
        words += ((m + 127) / 128) * dense_block_words(G.W);
        wmax = std::max(wmax, G.W);
    }
    const uint32_t xs = ((S + 7u) & ~7u) + 8u;
    const size_t smem = ((size_t)28 * wmax + 9) * 4 + (size_t)wmax * 64 * 4;
    const std::vector<uint32_t> pos0 = pos;
    for (int variant = 0; variant < 2; variant++) {        // an entry per work-item; eight entries per work-item
        std::vector<unsigned long long> gdata(words + 1);
        std::vector<uint16_t> ext((size_t)xrows * xs + 1);
        pos = pos0;
        row_any = k5;
        if (variant == 0) run_encode<1>(n, smem, off.data(), code.data(), pos.data(), rs, grp_of.data(), groups.data(), ulist.data(), upos.data(), gdata.data(), wmax, ext.data(), xs, row_any.data());
        else run_encode<8>(n, smem, off.data(), code.data(), pos.data(), rs, grp_of.data(), groups.data(), ulist.data(), upos.data(), gdata.data(), wmax, ext.data(), xs, row_any.data());
        const char *what = variant ? "behind the encode (8 per item)" : "behind the encode";
        if (pos == pos0) { printf("  %s: no run was clipped\n", what); bad++; }
        bad += compare_flags(what, row_any, scan_flags(off, code, pos, rs));
        for (uint32_t r = 0; r < n; r++)
            if (grp_of[r] == 0xFFFFFFFFu && row_any[r] != k5[r]) { printf("  %s: row %u outside the groups was written\n", what, r); bad++; }
        for (uint32_t r : t.cleared)
            if (row_any[r]) { printf("  %s: row %u of a clade on its own keeps its flag\n", what, r); bad++; }
        for (uint32_t r : t.expect0)
            if (row_any[r]) { printf("  %s: row %u shares no value and is flagged\n", what, r); bad++; }
        for (uint32_t r : t.expect1)
            if (!row_any[r]) { printf("  %s: row %u has a partner outside its group and no flag\n", what, r); bad++; }
        // the verify mode's kernel: agrees now, and counts a flag turned either way
        unsigned long long diff[2] = {0, ~0ull};
        index_verify_row_flags(off.data(), code.data(), pos.data(), rs, row_any.data(), n, diff, nullptr);
        if (diff[0]) { printf("  %s: the verify kernel counts %llu rows, first %llu\n", what, diff[0], diff[1]); bad++; }
        row_any[t.last_only] = 0;                           // (a lost run: wrong results)
        row_any[t.expect0[7]] = 1;                          // (a needless scan: only slow)
        index_verify_row_flags(off.data(), code.data(), pos.data(), rs, row_any.data(), n, diff, nullptr);
        if (diff[0] != 2 || diff[1] != std::min(t.last_only, t.expect0[7])) { printf("  %s: two flags turned, the verify kernel counts %llu rows, first %llu\n", what, diff[0], diff[1]); bad++; }
    }
    uint32_t set_k5 = 0;
    for (uint32_t f : k5) set_k5 += f != 0;
    printf("n %u s %u E %u, %zu groups (widest universe %u words), %u rows flagged by K5, last-only row %u (%zu entries), first-only row %u: %s\n", n, S, E,
           groups.size(), wmax, set_k5, t.last_only, t.rows[t.last_only].size(), t.first_only, bad ? "MISMATCH" : "as the images say");
    return bad ? 1 : 0;
}
