// cluster_extend_emu_main.cpp -- runs the launchers that extend an earlier clustering (mash_amd/csrc/cluster.hip: launch_cluster_seed,
// launch_cluster_union with a base per side, launch_cluster_label; mash_amd/csrc/cluster_greedy.hip: launch_greedy_append with a base
// per side, launch_greedy_seed, the rounds, launch_greedy_assign for the new rows only), unchanged, on the CPU (tools/hipemu) and
// compares them with a sequential statement of both definitions over the same edges: ref has n rows with an earlier partition,
// qry m rows; a RECT job names pairs {query q, reference r} -> {n + q, r}, a TRI job over qry names {q, q'} -> {n + q, n + q'}.
// TEST INFRASTRUCTURE (tests/test_cluster_extend_emu.py); built with g++.  The emulator runs workgroups one after another: what is
// pinned here is the arithmetic (word / bit / pair indices, bounds before bases, the seeds, the places in the list, rep[] of the
// new rows), not the races between workgroups.
//
//   cluster_extend_emu <case>            cases: small flat list blocks bridge chain density greedy overflow
//   cluster_extend_emu fuzz <seed> <n>   n random jobs
#include "../../tools/hipemu/hipemu.h"

#include <algorithm>
#include <cmath>
#include <random>
#include <string>
#include <vector>

#include "../../mash_amd/csrc/cluster.hip"
#include "../../mash_amd/csrc/cluster_greedy.hip"

using namespace mg;

typedef std::pair<uint32_t, uint32_t> Edge;      // {row, col} of a job, or {a, b} in the concatenation's index space

// one launch: a list of pairs with a mask, or rows [first_row, row_end) of the flat rectangle (ncols columns) / flat triangle
struct Job {
    bool rect = true;
    std::vector<uint2> rc;                       // list mode (empty and !flat: a list of no pairs)
    bool flat = false;
    uint64_t first_row = 0, ncols = 0, pairs = 0;
    std::vector<unsigned long long> masks;
    void set(uint64_t idx) { masks[idx >> 6] |= 1ull << (idx & 63); }
    bool get(uint64_t idx) const { return (masks[idx >> 6] >> (idx & 63)) & 1ull; }
};

static uint64_t tri(uint64_t r) { return r ? r * (r - 1) / 2 : 0; }

static Job list_job(bool rect, const std::vector<Edge> &pairs, bool all = true)
{
    Job J;
    J.rect = rect;
    for (const Edge &e : pairs) J.rc.push_back(make_uint2(e.first, e.second));
    J.pairs = pairs.size();
    J.masks.assign((J.pairs + 63) / 64, 0);
    for (uint64_t i = 0; all && i < J.pairs; i++) J.set(i);
    return J;
}

static Job flat_rect(uint64_t q0, uint64_t q1, uint64_t ncols)
{
    Job J;
    J.flat = true;
    J.first_row = q0;
    J.ncols = ncols;
    J.pairs = (q1 - q0) * ncols;
    J.masks.assign((J.pairs + 63) / 64, 0);
    return J;
}

static Job flat_tri(uint64_t q0, uint64_t q1)
{
    Job J;
    J.rect = false;
    J.flat = true;
    J.first_row = q0;
    J.pairs = tri(q1) - tri(q0);
    J.masks.assign((J.pairs + 63) / 64, 0);
    return J;
}

static void flat_set(Job &J, uint64_t row, uint64_t col)
{
    J.set(J.rect ? (row - J.first_row) * J.ncols + col : tri(row) + col - tri(J.first_row));
}

// the pairs a job stands for, {row, col} of the job, by the definition of the layouts (not by pair_rc)
static void pairs_of(const Job &J, std::vector<Edge> &out)
{
    if (!J.flat) {
        for (uint64_t i = 0; i < J.pairs; i++)
            if (J.get(i)) out.push_back({J.rc[i].x, J.rc[i].y});
        return;
    }
    uint64_t row = J.first_row, col = 0;
    if (!J.rect && row == 0) row = 1;
    for (uint64_t i = 0; i < J.pairs; i++) {
        if (J.get(i)) out.push_back({(uint32_t)row, (uint32_t)col});
        if (++col == (J.rect ? J.ncols : row)) { row++; col = 0; }
    }
}

static FinishArgs args_of(const Job &J)
{
    FinishArgs a{};
    a.pairs = J.pairs;
    a.first_row = J.first_row;
    a.ncols = J.ncols;
    a.triangle = J.rect ? 0 : 1;
    a.masks = const_cast<unsigned long long *>(J.masks.data());
    a.list_rc = J.flat ? nullptr : J.rc.data();
    return a;
}

static int failures = 0;
constexpr uint32_t GUARD = 0xDEADBEEFu;

// a partition of n rows in the form the label / assign launches write: seed[i] <= i, seed[seed[i]] == seed[i]
static std::vector<uint32_t> earlier(uint32_t n, uint32_t links, std::mt19937_64 &rng)
{
    std::vector<uint32_t> p(n);
    for (uint32_t i = 0; i < n; i++) p[i] = i;
    auto find = [&](uint32_t x) { while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; } return x; };
    for (uint32_t k = 0; n && k < links; k++) {
        const uint32_t a = find((uint32_t)(rng() % n)), b = find((uint32_t)(rng() % n));
        if (a != b) p[std::max(a, b)] = std::min(a, b);
    }
    std::vector<uint32_t> s(n);
    for (uint32_t i = 0; i < n; i++) s[i] = find(i);
    return s;
}

struct Shape { uint64_t min_rounds = 0; bool want_regrow = false; };

// seed: the earlier result over the n old rows (both modes read it); all_reps: the greedy call gets NULL instead (every old row a
// representative); first_cap: the first capacity of the edge list (0: room for everything)
static void check(const std::string &name, uint32_t n, uint32_t m, const std::vector<uint32_t> &seed, const std::vector<Job> &jobs, bool all_reps = false,
                  uint64_t first_cap = 0, Shape shape = {})
{
    const uint32_t N = n + m;
    const PairSpace rect_sp{m, n, n, 0u}, tri_sp{m, m, n, n};
    // ---- the new edges in the concatenation's index space, per job
    std::vector<std::vector<Edge>> per_job;
    std::vector<Edge> edges;
    for (const Job &J : jobs) {
        std::vector<Edge> pr, e;
        pairs_of(J, pr);
        for (const Edge &x : pr) e.push_back({n + x.first, J.rect ? x.second : n + x.second});
        edges.insert(edges.end(), e.begin(), e.end());
        per_job.push_back(e);
    }
    bool ok = true;

    // ---- single linkage: the components of {i ~ seed[i]} + new edges by a sequential union-find, label = smallest row
    std::vector<uint32_t> p(N);
    for (uint32_t i = 0; i < N; i++) p[i] = i;
    auto find = [&](uint32_t x) { while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; } return x; };
    auto unite = [&](uint32_t a, uint32_t b) { a = find(a); b = find(b); if (a != b) p[std::max(a, b)] = std::min(a, b); };
    for (uint32_t i = 0; i < n; i++) unite(i, seed[i]);
    for (const Edge &e : edges) unite(e.first, e.second);
    std::vector<uint32_t> want_label(N);
    uint64_t want_roots = 0;
    for (uint32_t i = 0; i < N; i++) { want_label[i] = find(i); want_roots += want_label[i] == i; }

    std::vector<uint32_t> parent(N + 1, GUARD), label(N + 1, GUARD), seed_dev(seed);
    seed_dev.push_back(GUARD);
    unsigned long long roots = ~0ull;
    auto invariant = [&] {
        for (uint32_t i = 0; i < N; i++) ok = ok && parent[i] <= i;
        ok = ok && parent[N] == GUARD && seed_dev[n] == GUARD;
    };
    ok = ok && launch_cluster_seed(parent.data(), seed_dev.data(), n, N, nullptr) == hipSuccess;
    invariant();
    for (uint32_t i = 0; i < N; i++) ok = ok && parent[i] == (i < n ? seed[i] : i);
    for (const Job &J : jobs) {
        ok = ok && launch_cluster_union(args_of(J), parent.data(), J.rect ? rect_sp : tri_sp, nullptr) == hipSuccess;
        invariant();
    }
    ok = ok && launch_cluster_label(parent.data(), N, label.data(), &roots, nullptr) == hipSuccess;
    invariant();
    ok = ok && label[N] == GUARD;
    uint64_t bad_label = 0;
    for (uint32_t i = 0; i < N; i++) bad_label += label[i] != want_label[i];

    // ---- greedy: the old rows are what the seed says, the walk goes on over the new rows in index order
    std::vector<std::vector<uint32_t>> smaller(N);
    for (const Edge &e : edges)
        if (e.first != e.second) smaller[std::max(e.first, e.second)].push_back(std::min(e.first, e.second));
    std::vector<bool> is_rep(N, false);
    std::vector<uint32_t> want_rep(m);
    uint64_t want_reps = 0;
    for (uint32_t i = 0; i < n; i++) { is_rep[i] = all_reps || seed[i] == i; want_reps += is_rep[i]; }
    for (uint32_t i = n; i < N; i++) {
        uint32_t r = i;
        for (uint32_t j : smaller[i])
            if (is_rep[j] && (r == i || j < r)) r = j;
        want_rep[i - n] = r;
        is_rep[i] = r == i;
        want_reps += is_rep[i];
    }

    uint64_t cap = first_cap ? first_cap : std::max<uint64_t>(edges.size(), 1), used = 0, regrows = 0;
    std::vector<uint2> list(cap + 1, make_uint2(GUARD, GUARD));
    unsigned long long cursor = 0;
    uint32_t overflow = 0;
    for (size_t j = 0; j < jobs.size(); j++) {
        const Job &J = jobs[j];
        std::vector<Edge> mine = per_job[j];
        for (int attempt = 0;; attempt++) {
            ok = ok && launch_greedy_append(args_of(J), J.rect ? rect_sp : tri_sp, list.data(), cap, &cursor, &overflow, nullptr) == hipSuccess;
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
        std::vector<Edge> got;                                                    // what this launch appended is its edges, in some order
        for (uint64_t i = used; i < cursor && i < cap; i++) got.push_back({list[i].x, list[i].y});
        for (Edge &e : mine) e = {std::max(e.first, e.second), std::min(e.first, e.second)};
        std::sort(got.begin(), got.end());
        std::sort(mine.begin(), mine.end());
        ok = ok && got == mine;
        used = cursor;
    }
    std::vector<uint32_t> state(N + 1, GUARD), rep(m + 1, GUARD), left(257, GUARD);
    ok = ok && launch_greedy_seed(state.data(), all_reps ? nullptr : seed_dev.data(), n, N, nullptr) == hipSuccess;
    for (uint32_t i = 0; i < N; i++) ok = ok && state[i] == (i >= n ? 0u : (all_reps || seed[i] == i) ? 3u : 2u);
    ok = ok && state[N] == GUARD && seed_dev[n] == GUARD;
    uint64_t rounds = 0;
    bool done = N == 0;
    for (uint32_t batch = 8; !done; batch = std::min(batch * 2, 256u)) {
        ok = ok && launch_greedy_rounds(list.data(), used, state.data(), N, left.data(), batch, nullptr) == hipSuccess;
        ok = ok && left[batch] == GUARD;
        uint32_t r = 0;
        while (r < batch && left[r]) r++;
        rounds += std::min(r + 1, batch);
        done = r < batch;
        if (rounds > N) { ok = false; break; }                                      // at most n + m rounds, ever
    }
    for (uint32_t i = 0; i < n; i++) ok = ok && state[i] == ((all_reps || seed[i] == i) ? 3u : 2u);      // the old rows never change
    for (uint32_t i = n; i < N; i++) ok = ok && (state[i] == 2 || state[i] == 3);
    unsigned long long reps = ~0ull;
    ok = ok && launch_greedy_assign(list.data(), used, state.data(), N, rep.data(), &reps, nullptr, n) == hipSuccess;
    ok = ok && state[N] == GUARD && rep[m] == GUARD && list[cap].x == GUARD;        // nothing written behind the arrays
    uint64_t bad_rep = 0;
    for (uint32_t q = 0; q < m; q++) bad_rep += rep[q] != want_rep[q];
    const bool shaped = rounds >= shape.min_rounds && (!shape.want_regrow || regrows > 0);
    if (!ok || bad_label || roots != want_roots || bad_rep || reps != want_reps || !shaped) {
        failures++;
        printf("FAIL %s: n %u m %u edges %zu: %llu labels differ, clusters %llu want %llu; %llu reps differ, representatives %llu want %llu, rounds %llu "
               "(want >= %llu), regrows %llu%s\n", name.c_str(), n, m, edges.size(), (unsigned long long)bad_label, roots, (unsigned long long)want_roots,
               (unsigned long long)bad_rep, reps, (unsigned long long)want_reps, (unsigned long long)rounds, (unsigned long long)shape.min_rounds,
               (unsigned long long)regrows, ok ? "" : " (launch, invariant, guard word or list content)");
    } else {
        printf("ok   %s: n %u m %u edges %zu clusters %llu representatives %llu rounds %llu regrows %llu\n", name.c_str(), n, m, edges.size(), roots, reps,
               (unsigned long long)rounds, (unsigned long long)regrows);
    }
}

static std::vector<uint32_t> singles(uint32_t n)
{
    std::vector<uint32_t> s(n);
    for (uint32_t i = 0; i < n; i++) s[i] = i;
    return s;
}

static void case_small()                                                     // (also the ThreadSanitizer build's case)
{
    std::mt19937_64 rng(5);
    check("no rows at all", 0, 0, {}, {});
    check("no new rows", 200, 0, earlier(200, 150, rng), {});
    check("no old rows, one new", 0, 1, {}, {});
    check("one old row, one new, no edge", 1, 1, {0}, {flat_rect(0, 1, 1)});
    { Job J = flat_rect(0, 1, 1); J.set(0); check("one old row, one new, their edge", 1, 1, {0}, {J}); }
    check("one new row without an edge", 200, 1, earlier(200, 150, rng), {flat_rect(0, 1, 200)});
    {   // no old rows: the whole-table call on qry
        Job T = flat_tri(0, 150);
        for (uint64_t i = 0; i < T.pairs; i += 7) T.set(i);
        check("no old rows, a triangle of 150", 0, 150, {}, {T});
    }
    {   // 200 old rows in clusters, 90 new rows: a flat rectangle, then a list triangle
        Job R = flat_rect(0, 90, 200);
        for (uint64_t i = 0; i < R.pairs; i += 131) R.set(i);
        std::vector<Edge> e;
        for (uint32_t q = 1; q < 90; q += 2) e.push_back({q, q / 3});
        check("200 old rows, 90 new: rect flat, tri list", 200, 90, earlier(200, 120, rng), {R, list_job(false, e)});
        check("the same, a list that is regrown", 200, 90, earlier(200, 120, rng), {R, list_job(false, e)}, false, 10, {0, true});
    }
    check("new rows without edges", 100, 50, earlier(100, 60, rng), {flat_rect(0, 50, 100), flat_tri(0, 50)});
}

static void case_flat()
{
    std::mt19937_64 rng(7);
    for (uint32_t ncols : {1u, 63u, 65u})
        for (uint32_t m : {1u, 3u, 67u, 129u}) {                             // pairs m * ncols: none of them a multiple of 64
            Job R = flat_rect(0, m, ncols);
            for (uint64_t i = 0; i < R.pairs; i++)
                if (rng() % 5 == 0 || i + 1 == R.pairs) R.set(i);
            check("flat rect, ncols " + std::to_string(ncols) + ", " + std::to_string(m) + " new rows", ncols, m, earlier(ncols, ncols / 3, rng), {R});
            Job A = flat_rect(0, m, ncols);                                  // every pair: the last word is ragged
            for (uint64_t i = 0; i < A.pairs; i++) A.set(i);
            check("flat rect, every pair, ncols " + std::to_string(ncols) + ", " + std::to_string(m) + " new rows", ncols, m, singles(ncols), {A}, true);
        }
}

static void case_list()
{
    std::mt19937_64 rng(9);
    const uint32_t n = 900, m = 400;
    for (uint32_t K : {1u, 37u, 63u, 64u, 65u, 4097u}) {                     // lists whose length is not a multiple of 64
        std::vector<Edge> r, t;
        for (uint32_t i = 0; i < K; i++) {
            r.push_back({(uint32_t)(rng() % m), (uint32_t)(rng() % n)});
            const uint32_t a = 1 + (uint32_t)(rng() % (m - 1));
            t.push_back({a, (uint32_t)(rng() % a)});
        }
        Job R = list_job(true, r, false), T = list_job(false, t, false);
        for (uint32_t i = 0; i < K; i++) {
            if (rng() % 100 < 40 || i + 1 == K) R.set(i);
            if (rng() % 100 < 10) T.set(i);
        }
        check("lists of " + std::to_string(K) + " pairs", n, m, earlier(n, 600, rng), {R, T});
    }
}

// rect row blocks, then tri row blocks, over one parent / one list
static std::vector<Job> blocks(uint32_t n, uint32_t m, uint64_t seed, uint32_t fam)
{
    std::mt19937_64 rng(seed);
    std::vector<Job> v;
    const uint32_t cuts[] = {0, 1, m / 3, m / 3 + 1, m - 1, m};
    for (int b = 0; b < 5; b++) {
        if (cuts[b] >= cuts[b + 1]) continue;
        Job R = flat_rect(cuts[b], cuts[b + 1], n);
        for (uint32_t q = cuts[b]; q < cuts[b + 1]; q++)
            for (int k = 0; k < 3; k++) {
                const uint32_t c = (uint32_t)(rng() % n);
                if ((n + q) % fam == c % fam) flat_set(R, q, c);
            }
        v.push_back(R);
    }
    for (int b = 0; b < 5; b++) {
        if (cuts[b] >= cuts[b + 1]) continue;
        Job T = flat_tri(cuts[b], cuts[b + 1]);
        for (uint32_t q = std::max(cuts[b], 1u); q < cuts[b + 1]; q++)
            for (int k = 0; k < 3; k++) {
                const uint32_t c = (uint32_t)(rng() % q);
                if (q % fam == c % fam) flat_set(T, q, c);
            }
        if (T.pairs) v.push_back(T);
    }
    return v;
}

static void case_blocks()
{
    std::mt19937_64 rng(13);
    check("rect blocks then tri blocks, ncols 777", 777, 500, earlier(777, 500, rng), blocks(777, 500, 17, 7));
    check("rect blocks then tri blocks, ncols 65", 65, 300, earlier(65, 20, rng), blocks(65, 300, 19, 3));
}

static void case_bridge()
{
    // old clusters {0 .. 99} and {100 .. 199}; new row 0 has an edge into each: one cluster; greedy: it joins rep 0 (the smaller)
    std::vector<uint32_t> s(200);
    for (uint32_t i = 0; i < 200; i++) s[i] = i < 100 ? 0 : 100;
    Job R = flat_rect(0, 3, 200);
    flat_set(R, 0, 57);
    flat_set(R, 0, 100);
    flat_set(R, 0, 0);
    check("a new row bridging two old clusters", 200, 3, s, {R, flat_tri(0, 3)});
    // every new row q joins old singletons 2 q and 2 q + 1
    const uint32_t m = 150;
    std::vector<Edge> e;
    for (uint32_t q = 0; q < m; q++) { e.push_back({q, 2 * q}); e.push_back({q, 2 * q + 1}); }
    check("every new row joins two old singletons", 2 * m, m, singles(2 * m), {list_job(true, e)});
    // every new row q joins old rows q and q + 1: one path through all of them
    std::vector<Edge> p;
    for (uint32_t q = 0; q < m; q++) { p.push_back({q, q}); p.push_back({q, q + 1}); }
    check("new rows close a path over the old ones", m + 1, m, singles(m + 1), {list_job(true, p)});
}

static void case_chain()
{
    // two old clusters meet only through a chain of new rows: old 0 - new 0 - new 1 - ... - new 99 - old 50
    const uint32_t n = 100, m = 100;
    std::vector<uint32_t> s(n);
    for (uint32_t i = 0; i < n; i++) s[i] = i < 50 ? 0 : 50;
    Job R = flat_rect(0, m, n);
    flat_set(R, 0, 0);
    flat_set(R, m - 1, 50);
    Job T = flat_tri(0, m);
    for (uint32_t q = 1; q < m; q++) flat_set(T, q, q - 1);
    // greedy: new 0 joins old rep 0, new 1 has no rep beside it -> REP, new 2 joins it, ...: a chain in index order, a round decides two rows
    check("old clusters that meet through new rows only", n, m, s, {R, T}, false, 0, {m / 2 - 1, false});
    // a new-new chain with no old row beside it
    check("a chain of new rows in index order", n, m, s, {flat_rect(0, m, n), T}, false, 0, {m / 2 - 1, false});
    // new rows reach an old cluster only through another new row: a star of new rows around new row 7, which touches old row 60
    Job R2 = flat_rect(0, m, n);
    flat_set(R2, 7, 60);
    std::vector<Edge> star;
    for (uint32_t q = 0; q < m; q++)
        if (q != 7) star.push_back({std::max(q, 7u), std::min(q, 7u)});
    check("new rows beside an old cluster through one new row", n, m, s, {R2, list_job(false, star)});
}

static void case_density()
{
    std::mt19937_64 rng(11);
    const uint32_t n = 4000, m = 2000;
    std::vector<Edge> e;
    for (uint32_t w = 0; w < 65 * 3; w++)
        for (int b = 0; b < 64; b++) e.push_back({(uint32_t)(rng() % m), (uint32_t)(rng() % n)});
    Job L = list_job(true, e, false);
    for (uint32_t w = 0; w < 65 * 3; w++) {                                      // word w carries w % 65 bits, 0 .. 64
        std::vector<int> bits(64);
        for (int b = 0; b < 64; b++) bits[b] = b;
        std::shuffle(bits.begin(), bits.end(), rng);
        for (uint32_t k = 0; k < w % 65; k++) L.set((uint64_t)w * 64 + bits[k]);
    }
    check("mask words of every density, rect list", n, m, earlier(n, 3000, rng), {L});
    Job F = flat_rect(0, 333, 65);                                               // 21 645 pairs
    Job T = flat_tri(0, 333);                                                    // 55 278 pairs
    for (Job *J : {&F, &T})
        for (uint64_t w = 0; w < J->masks.size(); w++) {
            const uint64_t left = J->pairs - w * 64;
            unsigned long long mk = 0;
            for (uint32_t k = 0; k < (w * 7) % 65; k++) mk |= 1ull << (rng() % 64);
            if ((w * 7) % 65 == 64) mk = ~0ull;
            if (w % 3) mk = w % 5 ? 0 : mk & rng() & rng() & rng();
            J->masks[w] = left >= 64 ? mk : mk & ((1ull << left) - 1);
        }
    check("mask words of every density, flat rect and tri", 65, 333, earlier(65, 30, rng), {F, T});
}

static void case_greedy()
{
    // old rows: 0 REP, 1 MEMBER of 0, 2 REP.  New row 0 (index 3) has one edge, to old MEMBER 1: it must become a representative
    {
        Job R = flat_rect(0, 1, 3);
        flat_set(R, 0, 1);
        check("a new row beside an old MEMBER only", 3, 1, {0, 0, 2}, {R});
    }
    // new row 0 beside old REP 2 and old MEMBER 1: a member of 2
    {
        Job R = flat_rect(0, 1, 3);
        flat_set(R, 0, 1);
        flat_set(R, 0, 2);
        check("a new row beside an old REP", 3, 1, {0, 0, 2}, {R});
    }
    // new 0 beside old REPs 0 and 2 -> joins 0; new 1 beside new 0 (a MEMBER) only -> REP; new 2 beside new 1 -> its member; new 3 beside
    // old MEMBER 1 and new 2 (MEMBER) -> REP
    {
        Job R = flat_rect(0, 4, 3);
        flat_set(R, 0, 2);
        flat_set(R, 0, 0);
        flat_set(R, 3, 1);
        Job T = flat_tri(0, 4);
        flat_set(T, 1, 0);
        flat_set(T, 2, 1);
        flat_set(T, 3, 2);
        check("old and new representatives in one walk", 3, 4, {0, 0, 2}, {R, T});
    }
    // every old row a representative (the caller left the members out): ref_rep == NULL
    {
        std::mt19937_64 rng(21);
        const uint32_t n = 300, m = 500;
        std::vector<Edge> r, t;
        for (uint32_t q = 0; q < m; q++) {
            if (q % 3) r.push_back({q, (uint32_t)(rng() % n)});
            if (q % 4 == 0) r.push_back({q, (uint32_t)(rng() % n)});
            if (q && q % 2) t.push_back({q, (uint32_t)(rng() % q)});
        }
        check("every old row a representative (NULL)", n, m, singles(n), {list_job(true, r), list_job(false, t)}, true);
        // the same edges over an earlier result with members: other decisions
        check("the same edges, old members among them", n, m, earlier(n, 200, rng), {list_job(true, r), list_job(false, t)});
    }
    // a band among the new rows: row q beside q - 1 .. q - 4, and row q beside old row q % n when q % 5 == 0
    {
        const uint32_t n = 64, m = 1200;
        Job R = flat_rect(0, m, n), T = flat_tri(0, m);
        for (uint32_t q = 0; q < m; q++) {
            if (q % 5 == 0) flat_set(R, q, q % n);
            for (uint32_t k = 1; k <= 4 && k <= q; k++) flat_set(T, q, q - k);
        }
        std::mt19937_64 rng(23);
        check("a band among the new rows", n, m, earlier(n, 40, rng), {R, T});
    }
}

static void case_overflow()
{
    std::mt19937_64 rng(29);
    check("blocks, a list of 1 edge at first", 777, 500, earlier(777, 500, rng), blocks(777, 500, 31, 7), false, 1, {0, true});
    check("blocks, a list of 100 edges at first", 777, 500, earlier(777, 500, rng), blocks(777, 500, 37, 7), false, 100, {0, true});
    const uint32_t n = 500, m = 400;
    std::vector<Edge> r, t;
    for (uint32_t q = 0; q < m; q++) { r.push_back({q, q}); r.push_back({q, (q * 7) % n}); }
    for (uint32_t q = 1; q < m; q++) t.push_back({q, q / 2});
    const std::vector<uint32_t> s = earlier(n, 300, rng);
    // the rect job fits, the tri job overflows once and the list is regrown with the rect job's edges copied over
    check("the second job overflows once", n, m, s, {list_job(true, r), list_job(false, t)}, false, r.size() + 5, {0, true});
    check("a capacity inside a word", n, m, s, {list_job(true, r), list_job(false, t)}, false, 70, {0, true});
    check("a capacity of exactly the edges", n, m, s, {list_job(true, r), list_job(false, t)}, false, r.size() + t.size(), {0, false});
    check("a capacity one short", n, m, s, {list_job(true, r), list_job(false, t)}, false, r.size() + t.size() - 1, {0, true});
}

static void fuzz(uint64_t seed, int jobs)
{
    std::mt19937_64 rng(seed);
    for (int j = 0; j < jobs; j++) {
        const uint32_t n = (uint32_t)(rng() % (j % 7 == 0 ? 3 : j % 5 == 0 ? 8000 : 900));
        const uint32_t m = (uint32_t)(rng() % (j % 11 == 0 ? 3 : j % 5 == 0 ? 3000 : 700));
        const double dens = std::pow(10.0, -(double)(rng() % 5));           // 1 .. 1e-4
        const uint32_t fam = 1 + (uint32_t)(rng() % 40);                     // edges only inside residue classes of the concatenation
        const bool flat = rng() % 2 && (uint64_t)n * m <= 1500000 && m <= 1500;
        auto hit = [&] { return (double)(rng() % 1000000) < dens * 1e6; };
        std::vector<Job> v;
        if (flat) {
            for (uint32_t q = 0; q < m && n;) {                              // rect row blocks
                const uint32_t q2 = std::min<uint32_t>(m, q + 1 + (uint32_t)(rng() % m));
                Job R = flat_rect(q, q2, n);
                for (uint64_t i = 0; i < R.pairs; i++)
                    if ((n + q + i / n) % fam == (i % n) % fam && hit()) R.set(i);
                v.push_back(R);
                q = q2;
            }
            for (uint32_t q = 0; q < m;) {                                   // tri row blocks
                const uint32_t q2 = std::min<uint32_t>(m, q + 1 + (uint32_t)(rng() % m));
                Job T = flat_tri(q, q2);
                uint64_t row = std::max<uint64_t>(q, 1), col = 0;
                for (uint64_t i = 0; i < T.pairs; i++) {
                    if (row % fam == col % fam && hit()) T.set(i);
                    if (++col == row) { row++; col = 0; }
                }
                if (T.pairs) v.push_back(T);
                q = q2;
            }
        } else {
            const uint64_t K = rng() % 40000;
            std::vector<Edge> r, t;
            for (uint64_t i = 0; n && m && i < K; i++) r.push_back({(uint32_t)(rng() % m), (uint32_t)(rng() % n)});
            for (uint64_t i = 0; m > 1 && i < K / 2; i++) {
                const uint32_t a = 1 + (uint32_t)(rng() % (m - 1)), b = (uint32_t)(rng() % a);
                if (rng() % 2) t.push_back({a, b}); else t.push_back({b, a});     // a list names a pair either way round
            }
            Job R = list_job(true, r, false), T = list_job(false, t, false);
            for (uint64_t i = 0; i < R.pairs; i++)
                if ((n + r[i].first) % fam == r[i].second % fam && hit()) R.set(i);
            for (uint64_t i = 0; i < T.pairs; i++)
                if (t[i].first % fam == t[i].second % fam && hit()) T.set(i);
            if (R.pairs) v.push_back(R);
            if (T.pairs) v.push_back(T);
        }
        const bool all_reps = rng() % 4 == 0;
        const std::vector<uint32_t> s = all_reps ? singles(n) : earlier(n, (uint32_t)(rng() % (n + 1)), rng);
        const uint64_t cap = rng() % 3 ? 0 : 1 + rng() % 5000;               // every third job starts with a short list
        check("fuzz " + std::to_string(j), n, m, s, v, all_reps, cap);
    }
}

int main(int argc, char **argv)
{
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "small") case_small();
    else if (c == "flat") case_flat();
    else if (c == "list") case_list();
    else if (c == "blocks") case_blocks();
    else if (c == "bridge") case_bridge();
    else if (c == "chain") case_chain();
    else if (c == "density") case_density();
    else if (c == "greedy") case_greedy();
    else if (c == "overflow") case_overflow();
    else if (c == "fuzz" && argc > 3) fuzz(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
    else { fprintf(stderr, "usage: cluster_extend_emu small|flat|list|blocks|bridge|chain|density|greedy|overflow | fuzz <seed> <n>\n"); return 2; }
    if (failures) { printf("%d case(s) FAILED\n", failures); return 1; }
    printf("all cases agree\n");
    return 0;
}
