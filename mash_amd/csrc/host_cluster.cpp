// host_cluster.cpp -- the cluster entry points: the marked pairs of a thresholded triangle (cut_counts) united on the device
// (cluster.hip, cluster_medoid.hip), or gathered as an edge list for the greedy rounds (cluster_greedy.hip), the minimum spanning
// forest (cluster_forest.hip), the complete-linkage rounds (cluster_complete.hip) and the density passes (cluster_density.hip); an
// earlier clustering extended by new rows in the first two forms
#include "cut_internal.h"
#include <deque>

/* ------------------------------------------------- the jobs of a call and their marked pairs */

// One range of pairs of a clustering call, where its pairs stand in the index space of the call's rows, and what the job keeps on
// the device until the call's last wait: nothing is waited for between two jobs of a union, so each has buffers of its own
struct ClusterJob {
    OutRange R;
    mg::PairSpace sp;
    CutBufs bufs;
    PassABufs pa;
    DevBuf<unsigned long long> d_count;                       // counted: pass A's count of block b (the list: block 0), left on the device
    uint64_t nblocks = 0;
    const bool counted;
    ClusterJob(mg_ctx *ctx, const OutRange &R_, const mg::PairSpace &sp_, bool counted_)
        : R(R_), sp(sp_), bufs(ctx, ctx), pa(ctx), d_count(ctx), counted(counted_) {}
};

// What a call works on: `total` rows -- ref's (an earlier clustering; nullptr: none), then qry's -- and the jobs whose marked pairs
// are exactly the edges that touch a row of qry: the rectangle qry x ref (row = query q -> n + q, col = reference r) and the triangle
// of qry (both sides n + .), which without ref is the whole table.  A job without pairs is left out.
struct ClusterJobs {
    uint32_t total = 0, s = 0;
    std::deque<ClusterJob> list;
};

// The start of every driver: the jobs, and the refusals that do not depend on the entry point.  J->total == 0: nothing to do.
// denom_limit: the sketch size at which the weight key of forest_key.h stops being exact (0: the key is not used), `what` names
// its user.
static int cluster_jobs(mg_ctx *ctx, const mg_table *ref, const mg_table *qry, const Cut &cut, bool counted, ClusterJobs *J, uint32_t denom_limit = 0,
                        const char *what = "")
{
    const uint64_t n = ref ? ref->n : 0, m = qry->n;
    OutRange R;
    int rc = ref ? out_range(ctx, qry, ref, 0, m, false, &R) : MG_OK;
    if (rc != MG_OK) return rc;
    const bool rect = ref && !R.empty() && R.pairs;
    OutRange T;
    if ((rc = out_range(ctx, qry, qry, 0, m, true, &T)) != MG_OK || n + m == 0) return rc;
    if (cut.k < 1) return fail(ctx, MG_ERR_INVALID, "compare: bad k-mer size");
    if (n + m > 0x7FFFFFFFull) return fail(ctx, MG_ERR_UNSUPPORTED, "cluster: more than 2^31 - 1 rows");
    if (denom_limit && T.s >= denom_limit)
        return fail(ctx, MG_ERR_UNSUPPORTED, std::string(what) + ": sketch size 2^21 or more (the weight key orders denominators below 2^21 exactly)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));                  // (a call without a job still launches)
    J->total = (uint32_t)(n + m);
    J->s = T.s;
    if (rect) J->list.emplace_back(ctx, R, mg::PairSpace{(uint32_t)m, (uint32_t)n, (uint32_t)n, 0u}, counted);
    if (T.pairs) J->list.emplace_back(ctx, T, mg::PairSpace{(uint32_t)m, (uint32_t)m, (uint32_t)n, (uint32_t)n}, counted);
    return MG_OK;
}

// Pass A's way to the marked pairs of job J, the only call of cut_counts for clustering: the candidate list, or block after block of
// the matrix.  use(f) gets every piece with pass A's buffers bound; the consumer runs pass A itself (launch_finish_mark: where its
// count goes is the consumer's business) and reads the ballots.  begin(most_pairs) is called once, ahead of the first piece and
// behind it the denominator flags are cleared: before the first compare on the matrix route (most_pairs: all of R's), once the lists
// stand on the list route (their entries) -- lists that fall through to the matrix have begun nothing.
template <class Begin, class Use>
static int marked_pairs(mg_ctx *ctx, const Cut &cut, ClusterJob &J, Begin begin, Use use)
{
    auto start = [&](uint64_t most_pairs) -> int {
        const int rc = begin(most_pairs);
        if (rc != MG_OK) return rc;
        HIP_TRY(ctx, hipMemsetAsync(J.pa.seen, 0, ((size_t)J.R.s + 1) * 4, ctx->stream));
        return MG_OK;
    };
    return cut_counts(ctx, J.R, cut, true, {1ull << 30, "MASHGPU_CLUSTER_BLOCK_PAIRS", "cluster"}, J.bufs,
                      [&](uint64_t pairs, uint64_t, uint64_t blocks, bool lists) -> int {
        if (!J.pa.alloc(pairs, J.R.s) || (J.counted && J.d_count.alloc(blocks) != hipSuccess)) return kAllocFailed;
        return lists ? MG_OK : start(J.R.pairs);
    },
                      [&] { J.pa.release(); },
                      [&](mg::FinishArgs f, const RowBlock &, const CandLists *L) -> int {
        const int rc = L ? start(L->K) : MG_OK;
        if (rc != MG_OK) return rc;
        J.pa.bind(f);
        return use(f);
    });
}

// The arguments of every entry point, checked under the context's lock before `run` is called.  args_ok: the entry's own pointers.
// ref: the table of an earlier clustering, where the entry extends one (seed_name set), and `seed` that clustering over ref's rows
template <class Run>
static int cluster_call(mg_ctx *ctx, const char *name, const mg_table *ref, const mg_table *t, const Cut &cut, bool args_ok, const uint32_t *seed,
                        const char *seed_name, Run run)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const std::string who(name);
    if (!t || (seed_name && !ref) || !args_ok) return fail(ctx, MG_ERR_INVALID, who + ": NULL argument");
    if (!t->lengths || !t->has_lengths || (ref && (!ref->lengths || !ref->has_lengths)))
        return fail(ctx, MG_ERR_INVALID, who + (ref ? ": the tables carry no lengths" : ": the table carries no lengths"));
    if (!cut.filtered()) return fail(ctx, MG_ERR_INVALID, who + ": both filters are off (every pair would be an edge)");
    if (ref && ref->s != t->s)
        return fail(ctx, MG_ERR_INVALID, who + ": sketch sizes differ (" + std::to_string(ref->s) + " and " + std::to_string(t->s) + ")");
    for (uint64_t i = 0; seed && i < ref->n; i++) {
        const std::string at = who + ": " + seed_name + "[" + std::to_string(i) + "] = " + std::to_string(seed[i]);
        if (seed[i] > i) return fail(ctx, MG_ERR_INVALID, at + " is larger than its row");
        if (seed[seed[i]] != seed[i])
            return fail(ctx, MG_ERR_INVALID, at + " is not the first row of its cluster (" + seed_name + "[" + std::to_string(seed[i]) + "] = " +
                                                 std::to_string(seed[seed[i]]) + ")");
    }
    return run();
}

static uint64_t rows_of(const mg_table *t) { return t ? t->n : 0; }


/* ------------------------------------------------- single-linkage clusters (cluster.hip), their medoids (cluster_medoid.hip) */

// where a call with medoids wants them; score_out may be NULL
struct MedoidOut { uint32_t *medoid; uint64_t *score; };

// Every job's marked pairs united into `parent`, which lives across the jobs and their blocks -- each row its own cluster, or ref's
// rows seeded with the earlier labels ref_label (host) --, then one label launch.  No pass B, no distance table, no record, and one
// wait, at the end: pass A's counts stay on the device until then.
// M: a score beside the union, cleared once before the first block; every block's set bits unite and add their weights in one launch
// (launch_medoid_union), and the pick runs behind the labels on the same stream.  MASHGPU_MEDOID_PLAIN: two atomics per edge (the A/B
// of tools/cluster_medoid_bench.py; the bits are the same).
static int cluster_union(mg_ctx *ctx, const mg_table *ref, const mg_table *qry, const uint32_t *ref_label, const Cut &cut, uint32_t *label_out,
                         const MedoidOut *M, bool on_device, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    *n_clusters_out = *n_edges_out = 0;
    ClusterJobs J;
    const int rcj = cluster_jobs(ctx, ref, qry, cut, true, &J);
    if (rcj != MG_OK || !J.total) return rcj;
    const uint32_t total = J.total, n_old = (uint32_t)rows_of(ref);
    const bool plain = M && ctx_opt(ctx, "MASHGPU_MEDOID_PLAIN") != nullptr;
    const bool own_score = M && !(on_device && M->score);
    DevBuf<uint32_t> parent(ctx), label(ctx), medoid(ctx), pick(ctx);
    DevBuf<unsigned long long> score(ctx), best(ctx), d_roots(ctx);
    if (parent.alloc(total) != hipSuccess || d_roots.alloc(1) != hipSuccess || (!on_device && label.alloc(total) != hipSuccess) ||
        (M && (pick.alloc(total) != hipSuccess || best.alloc(total) != hipSuccess)) || (M && !on_device && medoid.alloc(total) != hipSuccess) ||
        (own_score && score.alloc(total) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(ctx, MG_ERR_NOMEM, "cluster: device allocation failed");
    }
    uint32_t *d_label = on_device ? label_out : label.p, *d_medoid = M && on_device ? M->medoid : medoid.p;
    unsigned long long *d_score = M && !own_score ? (unsigned long long *)M->score : score.p;
    if (ref) {
        // the earlier labels travel through `label`, which nobody writes before the label launch
        if (n_old) HIP_TRY(ctx, hipMemcpyAsync(d_label, ref_label, (size_t)n_old * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, mg::launch_cluster_seed(parent, d_label, n_old, total, ctx->stream));
    } else {
        HIP_TRY(ctx, mg::launch_cluster_init(parent, total, ctx->stream));
    }
    if (M) HIP_TRY(ctx, hipMemsetAsync(d_score, 0, (size_t)total * 8, ctx->stream));
    size_t counts = 1;                                        // [0]: the clusters, then every job's blocks
    for (ClusterJob &job : J.list) {
        const int rc = marked_pairs(ctx, cut, job, [](uint64_t) { return MG_OK; }, [&](const mg::FinishArgs &f) -> int {
            HIP_TRY(ctx, mg::launch_finish_mark(f, job.d_count + job.nblocks++, ctx->stream));      // (stores its count: no word is cleared)
            if (M) HIP_TRY(ctx, mg::launch_medoid_union(f, parent, d_score, job.sp, ctx->stream, plain));
            else HIP_TRY(ctx, mg::launch_cluster_union(f, parent, job.sp, ctx->stream));
            return MG_OK;
        });
        if (rc != MG_OK) return rc;
        counts += job.nblocks;
    }
    // the labels, the roots' number and pass A's counts, behind every union queued so far
    std::vector<unsigned long long> h(counts);
    HIP_TRY(ctx, mg::launch_cluster_label(parent, total, d_label, d_roots, ctx->stream));
    if (M) HIP_TRY(ctx, mg::launch_medoid_pick(d_label, d_score, total, best, pick, d_medoid, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), d_roots, 8, hipMemcpyDeviceToHost, ctx->stream));
    size_t at = 1;
    for (const ClusterJob &job : J.list) {
        if (job.nblocks) HIP_TRY(ctx, hipMemcpyAsync(h.data() + at, job.d_count, job.nblocks * 8, hipMemcpyDeviceToHost, ctx->stream));
        at += job.nblocks;
    }
    if (!on_device) {
        HIP_TRY(ctx, hipMemcpyAsync(label_out, d_label, (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (M) HIP_TRY(ctx, hipMemcpyAsync(M->medoid, d_medoid, (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (M && M->score) HIP_TRY(ctx, hipMemcpyAsync(M->score, d_score, (size_t)total * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // (every job's buffers are released behind this wait)
    *n_clusters_out = h[0];
    for (size_t b = 1; b < h.size(); b++) *n_edges_out += h[b];
    return MG_OK;
}

int mg_cluster_tri_host(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                        uint32_t *label_out_host, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    return cluster_call(ctx, "mg_cluster_tri_host", nullptr, t, cut, n_clusters_out && n_edges_out && (label_out_host || !rows_of(t)), nullptr, nullptr,
                        [&] { return cluster_union(ctx, nullptr, t, nullptr, cut, label_out_host, nullptr, false, n_clusters_out, n_edges_out); });
}

int mg_cluster_tri_dev(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                       uint32_t *label_out_dev, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    return cluster_call(ctx, "mg_cluster_tri_dev", nullptr, t, cut, n_clusters_out && n_edges_out && (label_out_dev || !rows_of(t)), nullptr, nullptr,
                        [&] { return cluster_union(ctx, nullptr, t, nullptr, cut, label_out_dev, nullptr, true, n_clusters_out, n_edges_out); });
}

int mg_cluster_tri_medoid_host(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                               uint32_t *label_out_host, uint32_t *medoid_out_host, uint64_t *score_out_host, uint64_t *n_clusters_out,
                               uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    const MedoidOut M{medoid_out_host, score_out_host};
    return cluster_call(ctx, "mg_cluster_tri_medoid_host", nullptr, t, cut,
                        n_clusters_out && n_edges_out && ((label_out_host && medoid_out_host) || !rows_of(t)), nullptr, nullptr,
                        [&] { return cluster_union(ctx, nullptr, t, nullptr, cut, label_out_host, &M, false, n_clusters_out, n_edges_out); });
}

int mg_cluster_tri_medoid_dev(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                              uint32_t *label_out_dev, uint32_t *medoid_out_dev, uint64_t *score_out_dev, uint64_t *n_clusters_out,
                              uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    const MedoidOut M{medoid_out_dev, score_out_dev};
    return cluster_call(ctx, "mg_cluster_tri_medoid_dev", nullptr, t, cut,
                        n_clusters_out && n_edges_out && ((label_out_dev && medoid_out_dev) || !rows_of(t)), nullptr, nullptr,
                        [&] { return cluster_union(ctx, nullptr, t, nullptr, cut, label_out_dev, &M, true, n_clusters_out, n_edges_out); });
}

int mg_cluster_extend_host(mg_ctx *ctx, const mg_table *ref, const mg_table *qry, const uint32_t *ref_label, int kmer_size, double kmer_space,
                           double max_distance, double max_p_value, uint32_t *label_out_host, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    return cluster_call(ctx, "mg_cluster_extend_host", ref, qry, cut,
                        n_clusters_out && n_edges_out && (ref_label || !rows_of(ref)) && (label_out_host || !(rows_of(ref) + rows_of(qry))), ref_label,
                        "ref_label",
                        [&] { return cluster_union(ctx, ref, qry, ref_label, cut, label_out_host, nullptr, false, n_clusters_out, n_edges_out); });
}


/* ------------------------------------------------- edge lists: the greedy rounds (cluster_greedy.hip), the forest (cluster_forest.hip) */

// The edge list of one call: grown on demand, the pairs of every block appended behind those of the blocks before it.  E: an edge as
// Append writes it ({hi, lo} for the greedy rounds, with the pair's counts beside them for the forest)
template <class E, hipError_t (*Append)(const mg::FinishArgs &, const mg::PairSpace &, E *, uint64_t, unsigned long long *, uint32_t *, hipStream_t)>
struct EdgeList {
    mg_ctx *ctx;
    DevBuf<E> buf;
    DevBuf<unsigned long long> ctl;                           // [0] cursor, [1] pass A's count of the block, [2] overflow flag (its low word)
    uint64_t cap = 0, used = 0, n_edges = 0, regrows = 0;
    explicit EdgeList(mg_ctx *c) : ctx(c), buf(c), ctl(c) {}
    int init(uint64_t want)
    {
        cap = std::max<uint64_t>(want, 1);
        if (buf.alloc(cap) != hipSuccess || ctl.alloc(3) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, MG_ERR_NOMEM, "cluster: no device memory for the edge list (" + std::to_string(cap * sizeof(E)) + " bytes)");
        }
        HIP_TRY(ctx, hipMemsetAsync(ctl, 0, 24, ctx->stream));
        return MG_OK;
    }
    // Pass A over f's counts (pass A's buffers are bound), its marked pairs appended; waits for the block's figures and, if the
    // list was too short for them, regrows it (the pairs of earlier blocks copied over) and appends the block again -- pass A's
    // ballots are still there.  sp: where f's pairs stand in the index space of the list
    int append(const mg::FinishArgs &f, const mg::PairSpace &sp)
    {
        unsigned long long h[3] = {0, 0, 0};
        HIP_TRY(ctx, mg::launch_finish_mark(f, ctl + 1, ctx->stream));
        for (int attempt = 0;; attempt++) {
            HIP_TRY(ctx, Append(f, sp, buf, cap, ctl, reinterpret_cast<uint32_t *>(ctl + 2), ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(h, ctl, 24, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (h[0] <= cap && !h[2]) break;
            if (attempt) return fail(ctx, MG_ERR_HIP, "cluster: the edge list overflowed after it was regrown");
            const uint64_t want = std::max<uint64_t>(h[0], 2 * cap);
            DevBuf<E> bigger(ctx);
            if (bigger.alloc(want) != hipSuccess) {
                (void)hipGetLastError();
                return fail(ctx, MG_ERR_NOMEM, "cluster: no device memory for the edge list (" + std::to_string(want * sizeof(E)) + " bytes for " +
                                                   std::to_string(h[0]) + " edges so far)");
            }
            if (used) HIP_TRY(ctx, hipMemcpyAsync(bigger, buf, used * sizeof(E), hipMemcpyDeviceToDevice, ctx->stream));
            const unsigned long long back[3] = {used, h[1], 0};
            HIP_TRY(ctx, hipMemcpyAsync(ctl, back, 24, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the old list goes back to the pool behind the copy)
            std::swap(buf.p, bigger.p);
            cap = want;
            regrows++;
        }
        used = h[0];
        n_edges += h[1];
        return MG_OK;
    }
};
using GreedyEdges = EdgeList<uint2, mg::launch_greedy_append>;

// the list with counts (cluster_forest.hip's append): the forest's, and the greedy rounds' when members join their NEAREST representative
static hipError_t forest_append(const mg::FinishArgs &f, const mg::PairSpace &sp, uint4 *edges, uint64_t cap, unsigned long long *cursor,
                                uint32_t *overflow, hipStream_t stream)
{
    return mg::launch_forest_append(f, sp.rows, edges, cap, cursor, overflow, stream);      // (whole triangles only: no bases)
}
using ForestEdges = EdgeList<uint4, forest_append>;

// Every job's marked pairs appended to E (one wait per block).  The list begins with the first job that brings pairs, no longer than
// the pairs its route can bring -- the candidates, or the whole range -- and no longer than 2^23 edges (64 MB, 128 with counts) or what
// the test knob cap_knob says: it doubles, or grows to what a block needs, when it is short
template <class Edges>
static int gather_edges(mg_ctx *ctx, ClusterJobs &J, const Cut &cut, const char *cap_knob, Edges &E)
{
    uint64_t edge_cap = 1ull << 23;
    if (const char *o = ctx_opt(ctx, cap_knob)) edge_cap = std::max<uint64_t>(1, strtoull(o, nullptr, 10));
    for (ClusterJob &job : J.list) {
        const int rc = marked_pairs(ctx, cut, job, [&](uint64_t most_edges) { return E.buf.p ? MG_OK : E.init(std::min(edge_cap, most_edges)); },
                                    [&](const mg::FinishArgs &f) { return E.append(f, job.sp); });
        if (rc != MG_OK) return rc;
    }
    return MG_OK;
}

// What follows the last append of a greedy call: the fixpoint over E's edges in batches (one wait per batch: the rows each of its
// rounds left open), the assignment, the copy.  state[] holds n rows; the first n_old of them are seeded from d_seed
// (launch_greedy_seed; seeded == false: every row open) and rep_out takes the rows from n_old on.
// Edges == ForestEdges: the list carries the pairs' counts and the assignment is the nearest representative's (launch_nearest_assign:
// two more launches in the last batch, no further wait); whole tables only (n_old == 0).
template <class Edges>
static int greedy_fixpoint(mg_ctx *ctx, Edges &E, uint32_t n, uint32_t n_old, bool seeded, const uint32_t *d_seed, uint32_t *rep_out,
                           bool rep_on_device, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    constexpr bool kNearest = std::is_same<Edges, ForestEdges>::value;
    DevBuf<uint32_t> state(ctx), rep(ctx), left(ctx);
    DevBuf<unsigned long long> d_n(ctx), best_key(ctx);
    constexpr uint32_t kBatchMax = 256;
    if (state.alloc(n) != hipSuccess || left.alloc(kBatchMax) != hipSuccess || d_n.alloc(1) != hipSuccess ||
        (!rep_on_device && rep.alloc(n - n_old) != hipSuccess) || (kNearest && best_key.alloc(n) != hipSuccess))
        return fail(ctx, MG_ERR_NOMEM, "cluster: device allocation failed");
    uint32_t *d_rep = rep_on_device ? rep_out : rep.p;
    if (seeded) HIP_TRY(ctx, mg::launch_greedy_seed(state, d_seed, n_old, n, ctx->stream));
    else HIP_TRY(ctx, hipMemsetAsync(state, 0, (size_t)n * 4, ctx->stream));
    std::vector<uint32_t> h(kBatchMax);
    uint64_t rounds = 0, batches = 0;
    for (uint32_t batch = 8;; batch = std::min(batch * 2, kBatchMax)) {
        HIP_TRY(ctx, mg::launch_greedy_rounds(E.buf, E.used, state, n, left, batch, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h.data(), left, (size_t)batch * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        batches++;
        uint32_t r = 0;
        while (r < batch && h[r]) r++;
        rounds += std::min(r + 1, batch);
        if (r < batch) break;
        if (rounds > n) return fail(ctx, MG_ERR_HIP, "cluster: the rounds did not reach their fixpoint");      // (at most n are ever needed)
    }
    unsigned long long reps = 0;
    if constexpr (kNearest) HIP_TRY(ctx, mg::launch_nearest_assign(E.buf, E.used, state, n, best_key, d_rep, d_n, ctx->stream));
    else HIP_TRY(ctx, mg::launch_greedy_assign(E.buf, E.used, state, n, d_rep, d_n, ctx->stream, n_old));
    HIP_TRY(ctx, hipMemcpyAsync(&reps, d_n, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (!rep_on_device && n > n_old) HIP_TRY(ctx, hipMemcpyAsync(rep_out, d_rep, (size_t)(n - n_old) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_clusters_out = reps;
    *n_edges_out = E.n_edges;
    ctx->greedy_rounds = rounds;
    ctx->greedy_batches = batches;
    ctx->greedy_regrows = E.regrows;
    ctx->greedy_edge_cap = E.cap;
    return MG_OK;
}

// The edges of every job (gather_edges), then the rounds in batches, then the assignment.  ref: an earlier result ref_rep (host; NULL:
// every row of ref a representative) over its rows seeds the states, and rep_out takes qry's rows alone.
// Edges: GreedyEdges (the first representative), or ForestEdges (the nearest one: 16 bytes an edge instead of 8, nothing else differs
// before the assignment)
template <class Edges>
static int cluster_greedy(mg_ctx *ctx, const mg_table *ref, const mg_table *qry, const uint32_t *ref_rep, const Cut &cut, uint32_t *rep_out,
                          bool rep_on_device, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    constexpr bool kNearest = std::is_same<Edges, ForestEdges>::value;
    *n_clusters_out = *n_edges_out = 0;
    ctx->greedy_rounds = ctx->greedy_batches = ctx->greedy_regrows = ctx->greedy_edge_cap = 0;
    ClusterJobs J;
    int rc = cluster_jobs(ctx, ref, qry, cut, false, &J, kNearest ? mg::FOREST_DENOM_LIMIT : 0, "cluster nearest");
    if (rc != MG_OK || !J.total) return rc;
    const uint32_t n_old = (uint32_t)rows_of(ref);
    DevBuf<uint32_t> seed(ctx);
    if (ref_rep && n_old) {
        if (seed.alloc(n_old) != hipSuccess) return fail(ctx, MG_ERR_NOMEM, "cluster: device allocation failed");
        HIP_TRY(ctx, hipMemcpyAsync(seed, ref_rep, (size_t)n_old * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    Edges E(ctx);
    if ((rc = gather_edges(ctx, J, cut, "MASHGPU_GREEDY_EDGE_CAP", E)) != MG_OK) return rc;
    return greedy_fixpoint(ctx, E, J.total, n_old, ref != nullptr, seed.p, rep_out, rep_on_device, n_clusters_out, n_edges_out);
}

int mg_cluster_tri_greedy_host(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                               uint32_t *rep_out_host, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    return cluster_call(ctx, "mg_cluster_tri_greedy_host", nullptr, t, cut, n_clusters_out && n_edges_out && (rep_out_host || !rows_of(t)), nullptr, nullptr,
                        [&] { return cluster_greedy<GreedyEdges>(ctx, nullptr, t, nullptr, cut, rep_out_host, false, n_clusters_out, n_edges_out); });
}

int mg_cluster_tri_greedy_dev(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                              uint32_t *rep_out_dev, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    return cluster_call(ctx, "mg_cluster_tri_greedy_dev", nullptr, t, cut, n_clusters_out && n_edges_out && (rep_out_dev || !rows_of(t)), nullptr, nullptr,
                        [&] { return cluster_greedy<GreedyEdges>(ctx, nullptr, t, nullptr, cut, rep_out_dev, true, n_clusters_out, n_edges_out); });
}

int mg_cluster_tri_nearest_host(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                                uint32_t *rep_out_host, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    return cluster_call(ctx, "mg_cluster_tri_nearest_host", nullptr, t, cut, n_clusters_out && n_edges_out && (rep_out_host || !rows_of(t)), nullptr, nullptr,
                        [&] { return cluster_greedy<ForestEdges>(ctx, nullptr, t, nullptr, cut, rep_out_host, false, n_clusters_out, n_edges_out); });
}

int mg_cluster_tri_nearest_dev(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                               uint32_t *rep_out_dev, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    return cluster_call(ctx, "mg_cluster_tri_nearest_dev", nullptr, t, cut, n_clusters_out && n_edges_out && (rep_out_dev || !rows_of(t)), nullptr, nullptr,
                        [&] { return cluster_greedy<ForestEdges>(ctx, nullptr, t, nullptr, cut, rep_out_dev, true, n_clusters_out, n_edges_out); });
}

int mg_cluster_extend_greedy_host(mg_ctx *ctx, const mg_table *ref, const mg_table *qry, const uint32_t *ref_rep, int kmer_size, double kmer_space,
                                  double max_distance, double max_p_value, uint32_t *rep_out_host, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    return cluster_call(ctx, "mg_cluster_extend_greedy_host", ref, qry, cut, n_clusters_out && n_edges_out && (rep_out_host || !rows_of(qry)), ref_rep,
                        "ref_rep",
                        [&] { return cluster_greedy<GreedyEdges>(ctx, ref, qry, ref_rep, cut, rep_out_host, false, n_clusters_out, n_edges_out); });
}

int mg_cluster_greedy_stats(mg_ctx *ctx, uint64_t *rounds_out, uint64_t *batches_out, uint64_t *regrows_out, uint64_t *edge_capacity_out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (rounds_out) *rounds_out = ctx->greedy_rounds;
    if (batches_out) *batches_out = ctx->greedy_batches;
    if (regrows_out) *regrows_out = ctx->greedy_regrows;
    if (edge_capacity_out) *edge_capacity_out = ctx->greedy_edge_cap;
    return MG_OK;
}

// The whole triangle of t: the edge list with the pairs' counts (gather_edges), then ONE batch -- the rounds, the labels, the sort,
// the denominators -- and one wait for it, then the distance rows of exactly those denominators and the records
static int cluster_forest_tri(mg_ctx *ctx, const mg_table *t, const Cut &cut, mg_result *out_host, uint64_t capacity, uint64_t *count_out,
                              uint32_t *label_out, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    *count_out = *n_clusters_out = *n_edges_out = 0;
    ctx->forest_rounds = ctx->forest_regrows = ctx->forest_edge_cap = 0;
    ctx->forest_live.clear();
    ctx->forest_chosen.clear();
    ClusterJobs J;
    int rc = cluster_jobs(ctx, nullptr, t, cut, false, &J, mg::FOREST_DENOM_LIMIT, "cluster forest");
    if (rc != MG_OK || !J.total) return rc;
    const uint32_t n = J.total, s = J.s;
    ForestEdges E(ctx);
    if ((rc = gather_edges(ctx, J, cut, "MASHGPU_FOREST_EDGE_CAP", E)) != MG_OK) return rc;
    const uint32_t rounds_queued = mg::forest_rounds(n);
    DevBuf<uint32_t> parent(ctx), comp(ctx), merged(ctx), label(ctx), seen(ctx);
    DevBuf<unsigned long long> best_key(ctx), best_rc(ctx), live(ctx), d_n(ctx);      // d_n: [0] the chosen edges, [1] the clusters
    DevBuf<uint4> forest(ctx);
    if (parent.alloc(n) != hipSuccess || comp.alloc(n) != hipSuccess || merged.alloc(rounds_queued) != hipSuccess || label.alloc(n) != hipSuccess ||
        seen.alloc((uint64_t)s + 1) != hipSuccess || best_key.alloc(n) != hipSuccess || best_rc.alloc(n) != hipSuccess || live.alloc(rounds_queued) != hipSuccess ||
        d_n.alloc(2) != hipSuccess ||
        forest.alloc(mg::forest_room(n)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, MG_ERR_NOMEM, "cluster: device allocation failed");
    }
    const mg::ForestBufs fb{parent, comp, best_key, best_rc, forest, d_n, merged, live};
    std::vector<uint32_t> h_merged(rounds_queued), h_seen((size_t)s + 1);
    std::vector<unsigned long long> h_live(rounds_queued);
    unsigned long long h_n[2] = {0, 0};
    HIP_TRY(ctx, mg::launch_forest_rounds(E.buf, E.used, fb, n, label, d_n + 1, seen, s, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h_merged.data(), merged, (size_t)rounds_queued * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h_live.data(), live, (size_t)rounds_queued * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h_seen.data(), seen, h_seen.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h_n, d_n, 16, hipMemcpyDeviceToHost, ctx->stream));
    if (label_out) HIP_TRY(ctx, hipMemcpyAsync(label_out, label, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t r = 0;
    while (r < rounds_queued && h_merged[r]) r++;
    if (E.used && r == rounds_queued) return fail(ctx, MG_ERR_HIP, "cluster forest: the rounds did not reach their fixpoint");   // (floor(log2 n) + 1 suffice)
    const uint64_t count = h_n[0];
    if (count + h_n[1] != n) return fail(ctx, MG_ERR_HIP, "cluster forest: the chosen edges do not span the clusters");
    *count_out = count;
    *n_clusters_out = h_n[1];
    *n_edges_out = E.n_edges;
    ctx->forest_rounds = E.used ? r + 1 : 0;
    ctx->forest_live.assign(h_live.begin(), h_live.begin() + ctx->forest_rounds);
    ctx->forest_chosen.assign(h_merged.begin(), h_merged.begin() + ctx->forest_rounds);
    ctx->forest_regrows = E.regrows;
    ctx->forest_edge_cap = E.cap;
    if (count > capacity) return fail(ctx, MG_ERR_NOMEM, "cluster forest: more forest edges than `capacity` (see *count_out)");
    if (!count) return MG_OK;
    const mg_table *v = J.list.front().R.rows;                // (edges were chosen: the triangle's job is there)
    FinishTables ft(ctx);
    if ((rc = build_finish_tables(ctx, s, cut, h_seen, ft)) != MG_OK) return rc;
    DevBuf<mg::FinishEdge> recs(ctx);
    HIP_TRY(ctx, recs.alloc(count));
    HIP_TRY(ctx, mg::launch_forest_finish(finish_args(v, v, s, true, nullptr, count, 0, ft, cut), forest, count, recs, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out_host, recs, count * sizeof(mg_result), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!ft.complete) patch_nan_distances(out_host, count, cut.k);
    return MG_OK;
}

int mg_cluster_tri_forest_host(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                               mg_result *out_host, uint64_t capacity, uint64_t *count_out, uint32_t *label_out_host, uint64_t *n_clusters_out,
                               uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    return cluster_call(ctx, "mg_cluster_tri_forest_host", nullptr, t, cut, count_out && n_clusters_out && n_edges_out && (out_host || !capacity), nullptr,
                        nullptr,
                        [&] { return cluster_forest_tri(ctx, t, cut, out_host, capacity, count_out, label_out_host, n_clusters_out, n_edges_out); });
}

int mg_cluster_forest_stats(mg_ctx *ctx, uint64_t *rounds_out, uint64_t *regrows_out, uint64_t *edge_capacity_out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (rounds_out) *rounds_out = ctx->forest_rounds;
    if (regrows_out) *regrows_out = ctx->forest_regrows;
    if (edge_capacity_out) *edge_capacity_out = ctx->forest_edge_cap;
    return MG_OK;
}

int mg_cluster_forest_rounds(mg_ctx *ctx, uint64_t *live_out, uint64_t *chosen_out, uint64_t capacity, uint64_t *rounds_out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!rounds_out || ((!live_out || !chosen_out) && capacity)) return fail(ctx, MG_ERR_INVALID, "mg_cluster_forest_rounds: NULL argument");
    *rounds_out = ctx->forest_live.size();
    for (uint64_t r = 0; r < capacity && r < ctx->forest_live.size(); r++) {
        live_out[r] = ctx->forest_live[r];
        chosen_out[r] = ctx->forest_chosen[r];
    }
    return MG_OK;
}


/* ------------------------------------------------- complete linkage (cluster_complete.hip) */

// The whole triangle of t: the edge list with the pairs' counts (gather_edges: it is the forest's list, MASHGPU_FOREST_EDGE_CAP its
// first capacity), the keys and the lookup built once behind the last append, then the rounds in batches as greedy_fixpoint queues
// them -- 8 (MASHGPU_COMPLETE_BATCH: the first batch's size, a test knob), then doubling, one wait per batch for merged[] -- and the
// labels.  At most n rounds are ever needed: each but the last merges a link at least.
static int cluster_complete_tri(mg_ctx *ctx, const mg_table *t, const Cut &cut, uint32_t *label_out, bool on_device, uint64_t *n_clusters_out,
                                uint64_t *n_edges_out)
{
    *n_clusters_out = *n_edges_out = 0;
    ctx->complete_rounds = ctx->complete_batches = ctx->complete_regrows = ctx->complete_edge_cap = 0;
    ctx->complete_live.clear();
    ctx->complete_merged.clear();
    ClusterJobs J;
    int rc = cluster_jobs(ctx, nullptr, t, cut, false, &J, mg::FOREST_DENOM_LIMIT, "cluster complete");
    if (rc != MG_OK || !J.total) return rc;
    const uint32_t n = J.total;
    ForestEdges E(ctx);
    if ((rc = gather_edges(ctx, J, cut, "MASHGPU_FOREST_EDGE_CAP", E)) != MG_OK) return rc;
    const uint64_t m = E.used, slots = mg::complete_slots(m);
    constexpr uint32_t kBatchMax = 256;
    uint32_t batch = 8;
    if (const char *o = ctx_opt(ctx, "MASHGPU_COMPLETE_BATCH")) batch = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, strtoull(o, nullptr, 10)), kBatchMax);
    DevBuf<uint32_t> parent(ctx), mate(ctx), merged(ctx), label(ctx);
    DevBuf<unsigned long long> best_key(ctx), best_rc(ctx), key(ctx), next(ctx), slot_rc(ctx), slot_e(ctx), live(ctx), d_roots(ctx);
    if (parent.alloc(n) != hipSuccess || mate.alloc(n) != hipSuccess || merged.alloc(kBatchMax) != hipSuccess || best_key.alloc(n) != hipSuccess ||
        best_rc.alloc(n) != hipSuccess || live.alloc(kBatchMax) != hipSuccess || d_roots.alloc(1) != hipSuccess ||
        (!on_device && label.alloc(n) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(ctx, MG_ERR_NOMEM, "cluster: device allocation failed");
    }
    if (m && (key.alloc(m) != hipSuccess || next.alloc(m) != hipSuccess || slot_rc.alloc(slots) != hipSuccess || slot_e.alloc(slots) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(ctx, MG_ERR_NOMEM, "cluster complete: no device memory for the links' keys and their index (" + std::to_string(16 * m + 16 * slots) +
                                           " bytes for " + std::to_string(m) + " edges)");
    }
    const mg::CompleteBufs cb{parent, mate, best_key, best_rc, key, next, slot_rc, slot_e, slots, ~0ull, 0ull, merged, live};
    uint32_t *d_label = on_device ? label_out : label.p;
    HIP_TRY(ctx, mg::launch_complete_begin(E.buf, m, cb, n, ctx->stream));
    std::vector<uint32_t> h_merged(kBatchMax);
    std::vector<unsigned long long> h_live(kBatchMax);
    uint64_t rounds = 0, batches = 0;
    for (; m; batch = std::min(batch * 2, kBatchMax)) {
        HIP_TRY(ctx, mg::launch_complete_rounds(E.buf, m, cb, n, batch, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_merged.data(), merged, (size_t)batch * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(h_live.data(), live, (size_t)batch * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        batches++;
        uint32_t r = 0;
        while (r < batch && h_merged[r]) r++;
        const uint32_t ran = std::min(r + 1, batch);
        ctx->complete_live.insert(ctx->complete_live.end(), h_live.begin(), h_live.begin() + ran);
        ctx->complete_merged.insert(ctx->complete_merged.end(), h_merged.begin(), h_merged.begin() + ran);
        rounds += ran;
        if (r < batch) break;
        if (rounds > n) return fail(ctx, MG_ERR_HIP, "cluster complete: the rounds did not reach their fixpoint");      // (at most n are ever needed)
    }
    unsigned long long roots = 0;
    HIP_TRY(ctx, mg::launch_cluster_label(parent, n, d_label, d_roots, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&roots, d_roots, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (!on_device) HIP_TRY(ctx, hipMemcpyAsync(label_out, d_label, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_clusters_out = roots;
    *n_edges_out = E.n_edges;
    ctx->complete_rounds = rounds;
    ctx->complete_batches = batches;
    ctx->complete_regrows = E.regrows;
    ctx->complete_edge_cap = E.cap;
    return MG_OK;
}

int mg_cluster_tri_complete_host(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                                 uint32_t *label_out_host, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    return cluster_call(ctx, "mg_cluster_tri_complete_host", nullptr, t, cut, n_clusters_out && n_edges_out && (label_out_host || !rows_of(t)), nullptr,
                        nullptr, [&] { return cluster_complete_tri(ctx, t, cut, label_out_host, false, n_clusters_out, n_edges_out); });
}

int mg_cluster_tri_complete_dev(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                                uint32_t *label_out_dev, uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    return cluster_call(ctx, "mg_cluster_tri_complete_dev", nullptr, t, cut, n_clusters_out && n_edges_out && (label_out_dev || !rows_of(t)), nullptr,
                        nullptr, [&] { return cluster_complete_tri(ctx, t, cut, label_out_dev, true, n_clusters_out, n_edges_out); });
}

int mg_cluster_complete_stats(mg_ctx *ctx, uint64_t *rounds_out, uint64_t *batches_out, uint64_t *regrows_out, uint64_t *edge_capacity_out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (rounds_out) *rounds_out = ctx->complete_rounds;
    if (batches_out) *batches_out = ctx->complete_batches;
    if (regrows_out) *regrows_out = ctx->complete_regrows;
    if (edge_capacity_out) *edge_capacity_out = ctx->complete_edge_cap;
    return MG_OK;
}

int mg_cluster_complete_rounds(mg_ctx *ctx, uint64_t *live_out, uint64_t *merged_out, uint64_t capacity, uint64_t *rounds_out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!rounds_out || ((!live_out || !merged_out) && capacity)) return fail(ctx, MG_ERR_INVALID, "mg_cluster_complete_rounds: NULL argument");
    *rounds_out = ctx->complete_live.size();
    for (uint64_t r = 0; r < capacity && r < ctx->complete_live.size(); r++) {
        live_out[r] = ctx->complete_live[r];
        merged_out[r] = ctx->complete_merged[r];
    }
    return MG_OK;
}


/* ------------------------------------------------- density clusters (cluster_density.hip) */

// where a density call wants its results; via and degree may be NULL
struct DensityOut { uint32_t *label, *via, *degree; };

// The whole triangle of t: the edge list with the pairs' counts (gather_edges: the list of `-B`, MASHGPU_GREEDY_EDGE_CAP its first
// capacity), then ONE batch behind the last append -- degrees, the cores united, the borders' best keys and picks, the relabelling --
// and one wait for it.  MASHGPU_DENSITY_PLAIN: two atomic adds per edge in the degree pass (the A/B of tools/cluster_density_bench.py;
// the bits are the same).
static int cluster_density(mg_ctx *ctx, const mg_table *t, const Cut &cut, uint32_t min_neighbours, const DensityOut &out, bool on_device,
                           uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    *n_clusters_out = *n_edges_out = 0;
    ctx->density_cores = ctx->density_borders = ctx->density_noise = ctx->density_regrows = ctx->density_edge_cap = 0;
    if (!min_neighbours) return fail(ctx, MG_ERR_INVALID, "cluster density: min_neighbours is 0 (every row would be a core)");
    ClusterJobs J;
    int rc = cluster_jobs(ctx, nullptr, t, cut, false, &J, mg::FOREST_DENOM_LIMIT, "cluster density");
    if (rc != MG_OK || !J.total) return rc;
    const uint32_t n = J.total;
    const bool plain = ctx_opt(ctx, "MASHGPU_DENSITY_PLAIN") != nullptr;
    ForestEdges E(ctx);
    if ((rc = gather_edges(ctx, J, cut, "MASHGPU_GREEDY_EDGE_CAP", E)) != MG_OK) return rc;
    const bool own_via = !(on_device && out.via), own_deg = !(on_device && out.degree);
    DevBuf<uint32_t> parent(ctx), first(ctx), label(ctx), via(ctx), deg(ctx);
    DevBuf<unsigned long long> best_key(ctx), d_counts(ctx);
    if (parent.alloc(n) != hipSuccess || first.alloc(n) != hipSuccess || best_key.alloc(n) != hipSuccess || d_counts.alloc(5) != hipSuccess ||
        (!on_device && label.alloc(n) != hipSuccess) || (own_via && via.alloc(n) != hipSuccess) || (own_deg && deg.alloc(n) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(ctx, MG_ERR_NOMEM, "cluster: device allocation failed");
    }
    const mg::DensityBufs db{own_deg ? deg.p : out.degree, parent, on_device ? out.label : label.p, own_via ? via.p : out.via, first, best_key, d_counts};
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, mg::launch_density(E.buf, E.used, db, n, min_neighbours, plain, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h, d_counts, 32, hipMemcpyDeviceToHost, ctx->stream));
    if (!on_device) {
        HIP_TRY(ctx, hipMemcpyAsync(out.label, db.label, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (out.via) HIP_TRY(ctx, hipMemcpyAsync(out.via, db.via, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (out.degree) HIP_TRY(ctx, hipMemcpyAsync(out.degree, db.deg, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (h[0] + h[1] + h[2] != n) return fail(ctx, MG_ERR_HIP, "cluster density: cores, borders and noise do not add up to the rows");
    *n_clusters_out = h[3];
    *n_edges_out = E.n_edges;
    ctx->density_cores = h[0];
    ctx->density_borders = h[1];
    ctx->density_noise = h[2];
    ctx->density_regrows = E.regrows;
    ctx->density_edge_cap = E.cap;
    return MG_OK;
}

int mg_cluster_tri_density_host(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                                uint32_t min_neighbours, uint32_t *label_out_host, uint32_t *via_out_host, uint32_t *degree_out_host,
                                uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    const DensityOut out{label_out_host, via_out_host, degree_out_host};
    return cluster_call(ctx, "mg_cluster_tri_density_host", nullptr, t, cut, n_clusters_out && n_edges_out && (label_out_host || !rows_of(t)), nullptr,
                        nullptr, [&] { return cluster_density(ctx, t, cut, min_neighbours, out, false, n_clusters_out, n_edges_out); });
}

int mg_cluster_tri_density_dev(mg_ctx *ctx, const mg_table *t, int kmer_size, double kmer_space, double max_distance, double max_p_value,
                               uint32_t min_neighbours, uint32_t *label_out_dev, uint32_t *via_out_dev, uint32_t *degree_out_dev,
                               uint64_t *n_clusters_out, uint64_t *n_edges_out)
{
    const Cut cut{kmer_size, kmer_space, max_distance, max_p_value};
    const DensityOut out{label_out_dev, via_out_dev, degree_out_dev};
    return cluster_call(ctx, "mg_cluster_tri_density_dev", nullptr, t, cut, n_clusters_out && n_edges_out && (label_out_dev || !rows_of(t)), nullptr,
                        nullptr, [&] { return cluster_density(ctx, t, cut, min_neighbours, out, true, n_clusters_out, n_edges_out); });
}

int mg_cluster_density_stats(mg_ctx *ctx, uint64_t *cores_out, uint64_t *borders_out, uint64_t *noise_out, uint64_t *regrows_out,
                             uint64_t *edge_capacity_out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (cores_out) *cores_out = ctx->density_cores;
    if (borders_out) *borders_out = ctx->density_borders;
    if (noise_out) *noise_out = ctx->density_noise;
    if (regrows_out) *regrows_out = ctx->density_regrows;
    if (edge_capacity_out) *edge_capacity_out = ctx->density_edge_cap;
    return MG_OK;
}
