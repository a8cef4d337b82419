// host_taxscreen.cpp -- the taxonomy of a screen (mash taxscreen): taxonomy object, per-hash LCA and database histogram
// once per database, per-taxon counts and clade sums per mixture
#include "host_internal.h"

struct mg_taxonomy {
    mg_ctx *ctx = nullptr;
    uint64_t n = 0;
    std::vector<uint32_t> parent;       // host copy: the clade sums walk it
    uint32_t *d_parent = nullptr, *d_depth = nullptr;
};

int mg_taxonomy_create(mg_ctx *ctx, const uint32_t *parent, uint64_t n_nodes, mg_taxonomy **out)
{
    if (!ctx) return MG_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!out || (!parent && n_nodes)) return fail(ctx, MG_ERR_INVALID, "mg_taxonomy_create: NULL argument");
    if (n_nodes == 0 || n_nodes >= 0xFFFFFFF0ull) return fail(ctx, MG_ERR_INVALID, "mg_taxonomy_create: node count must be in [1, 2^32 - 16)");
    for (uint64_t i = 0; i < n_nodes; i++)
        if (parent[i] >= n_nodes) return fail(ctx, MG_ERR_INVALID, "mg_taxonomy_create: parent of node " + std::to_string(i) + " is out of range");
    // depths: walk up from every node without one to a node that has one (or a root), then number the path on the way back;
    // a walk that meets its own path is a cycle
    const uint32_t UNSET = 0xFFFFFFFFu, ON_PATH = 0xFFFFFFFEu;
    std::vector<uint32_t> depth(n_nodes, UNSET), path;
    for (uint64_t i = 0; i < n_nodes; i++) {
        if (depth[i] != UNSET) continue;
        path.clear();
        uint32_t v = (uint32_t)i, base;
        for (;;) {
            if (depth[v] == ON_PATH) return fail(ctx, MG_ERR_INVALID, "mg_taxonomy_create: cycle through node " + std::to_string(v));
            if (depth[v] != UNSET) { base = depth[v] + 1; break; }
            depth[v] = ON_PATH;
            path.push_back(v);
            if (parent[v] == v) { base = 0; break; }
            v = parent[v];
        }
        for (size_t q = path.size(); q-- > 0;) depth[path[q]] = base++;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    mg_taxonomy *t = new mg_taxonomy;
    t->ctx = ctx;
    t->n = n_nodes;
    t->parent.assign(parent, parent + n_nodes);
    hipError_t e = hipMalloc(&t->d_parent, n_nodes * 4);
    if (e == hipSuccess) e = hipMalloc(&t->d_depth, n_nodes * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_parent, parent, n_nodes * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_depth, depth.data(), n_nodes * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);          // (`depth` goes out of scope)
    if (e != hipSuccess) {
        mg_taxonomy_free(t);
        return fail(ctx, MG_ERR_HIP, std::string("mg_taxonomy_create: ") + hipGetErrorString(e));
    }
    *out = t;
    return MG_OK;
}

void mg_taxonomy_free(mg_taxonomy *t)
{
    if (!t) return;
    hipSetDevice(t->ctx->device);
    if (t->d_parent) hipFree(t->d_parent);
    if (t->d_depth) hipFree(t->d_depth);
    delete t;
}

void screen_tax_release(mg_screen *sc)
{
    mg_screen::Tax &x = sc->tx;
    for (void *q : {(void *)x.slot_node, (void *)x.hash_count, (void *)x.count, (void *)x.list, (void *)x.vals})
        if (q) hipFree(q);
    uint64_t builds = x.builds;
    x = mg_screen::Tax();
    x.builds = builds;
}

hipError_t screen_tax_clear(mg_screen *sc, uint64_t nt)
{
    if (!sc->tx.tax) return hipSuccess;
    return mg::launch_tax_clear(sc->tx.slot_node, sc->touched, nt, (uint32_t)sc->tx.tax->n, sc->tx.count, sc->ctx->stream);
}

int mg_screen_set_taxa(mg_screen *sc, const mg_taxonomy *tax, const uint32_t *row_node, uint64_t n_rows)
{
    if (!sc) return MG_ERR_INVALID;
    mg_ctx *ctx = sc->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!tax || (!row_node && n_rows)) return fail(ctx, MG_ERR_INVALID, "mg_screen_set_taxa: NULL argument");
    if (tax->ctx != ctx) return fail(ctx, MG_ERR_INVALID, "mg_screen_set_taxa: the taxonomy belongs to another context");
    if (n_rows != sc->db->n) return fail(ctx, MG_ERR_INVALID, "mg_screen_set_taxa: " + std::to_string(n_rows) + " row nodes for a table of " + std::to_string(sc->db->n) + " rows");
    if (!sc->touched) return fail(ctx, MG_ERR_UNSUPPORTED, "mg_screen_set_taxa: databases of more than 2^31 hashes keep no touched list and no rows-by-hash index");
    for (uint64_t i = 0; i < n_rows; i++)
        if (row_node[i] != MG_TAX_NONE && row_node[i] >= tax->n)
            return fail(ctx, MG_ERR_INVALID, "mg_screen_set_taxa: node of row " + std::to_string(i) + " is out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = screen_ensure_index(sc);
    if (rc != MG_OK) return rc;
    screen_tax_release(sc);                               // (a second binding replaces the first; hipFree waits for the device)
    mg_screen::Tax &x = sc->tx;
    const uint64_t nn = tax->n, postings = sc->db->n * sc->db->s, long_cap = postings / mg::TAX_LONG_RUN + 1;
    DevBuf<uint32_t> d_rows(ctx), d_long(ctx);
    DevBuf<unsigned long long> d_nlong(ctx);
    std::vector<uint32_t> hc(nn + 2);
    unsigned long long n_long = 0;
    hipError_t e = hipMalloc(&x.slot_node, sc->slots * 4);
    if (e == hipSuccess) e = hipMalloc(&x.hash_count, (nn + 2) * 4);
    if (e == hipSuccess) e = hipMalloc(&x.count, (nn + 2) * 4);
    if (e == hipSuccess) e = d_rows.alloc(n_rows);
    if (e == hipSuccess) e = d_long.alloc(long_cap);
    if (e == hipSuccess) e = d_nlong.alloc(1);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rows, row_node, n_rows * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(x.hash_count, 0, (nn + 2) * 4, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(x.count, 0, (nn + 2) * 4, ctx->stream);
    if (e == hipSuccess) e = mg::launch_tax_lca(sc->slots, sc->slot_end, sc->ent, d_rows, tax->d_parent, tax->d_depth, x.slot_node, d_long, d_nlong, long_cap, ctx->stream);
    if (e == hipSuccess) e = mg::launch_tax_hist(x.slot_node, sc->slots, nullptr, nullptr, (uint32_t)nn, x.hash_count, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hc.data(), x.hash_count, (nn + 2) * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&n_long, d_nlong, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        screen_tax_release(sc);
        return fail(ctx, MG_ERR_HIP, std::string("mg_screen_set_taxa: ") + hipGetErrorString(e));
    }
    // which nodes will ever be reported: those with database hashes at or below them (clade_hash_count > 0).  Their number is
    // that of the taxa the database touches plus their ancestors, so one walk up per node with hashes is cheap; it is done once.
    std::vector<uint32_t> clade(nn, 0);
    for (uint64_t v = 0; v < nn; v++) {
        if (!hc[v]) continue;
        for (uint32_t a = (uint32_t)v;; a = tax->parent[a]) {
            clade[a] += hc[v];
            if (tax->parent[a] == a) break;
        }
    }
    std::vector<uint32_t> pos(nn, 0xFFFFFFFFu), buckets;
    for (uint64_t v = 0; v < nn; v++) {
        if (!clade[v]) continue;
        pos[v] = (uint32_t)x.nodes.size();
        x.nodes.push_back((uint32_t)v);
        buckets.push_back((uint32_t)v);
        x.hash_counts.push_back(hc[v]);
        x.clade_hash_counts.push_back(clade[v]);
    }
    for (uint32_t v : x.nodes) x.up.push_back(tax->parent[v] == v ? -1 : (int32_t)pos[tax->parent[v]]);
    for (int q = 0; q < 2; q++) {                         // MG_TAX_DISJOINT (bucket nn), then MG_TAX_NONE (nn + 1)
        if (!hc[nn + q]) continue;
        x.nodes.push_back(q == 0 ? MG_TAX_DISJOINT : MG_TAX_NONE);
        buckets.push_back((uint32_t)(nn + q));
        x.hash_counts.push_back(hc[nn + q]);
        x.clade_hash_counts.push_back(hc[nn + q]);
        x.up.push_back(-1);
    }
    const uint64_t m = x.nodes.size();
    e = hipMalloc(&x.list, std::max<uint64_t>(m, 1) * 4);
    if (e == hipSuccess) e = hipMalloc(&x.vals, std::max<uint64_t>(m, 1) * 4);
    if (e == hipSuccess && m) e = hipMemcpyAsync(x.list, buckets.data(), m * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        screen_tax_release(sc);
        return fail(ctx, MG_ERR_HIP, std::string("mg_screen_set_taxa: ") + hipGetErrorString(e));
    }
    x.tax = tax;
    x.long_runs = n_long;
    x.builds++;
    char note[200];
    snprintf(note, sizeof note, "per-hash LCA built %llu time(s): %llu hashes, %llu long runs (> %u rows) folded by a workgroup each, %llu taxa carry hashes",
             (unsigned long long)x.builds, (unsigned long long)sc->distinct, (unsigned long long)n_long, mg::TAX_LONG_RUN, (unsigned long long)m);
    x.note = note;
    return MG_OK;
}

const char *mg_screen_tax_note(const mg_screen *sc) { return sc ? sc->tx.note.c_str() : ""; }

int mg_screen_tax_finish_host(mg_screen *sc, mg_taxon_count *out, uint64_t capacity, uint64_t *n_out, uint64_t *total_count,
                              uint64_t *total_hash_count, uint64_t *mix_hashes_out, uint32_t *mix_nhash_out, uint64_t *distinct_out)
{
    if (!sc) return MG_ERR_INVALID;
    mg_ctx *ctx = sc->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!n_out || (!out && capacity)) return fail(ctx, MG_ERR_INVALID, "mg_screen_tax_finish_host: NULL argument");
    if (!sc->touched) return fail(ctx, MG_ERR_UNSUPPORTED, "mg_screen_tax_finish_host: databases of more than 2^31 hashes keep no touched list");
    mg_screen::Tax &x = sc->tx;
    if (!x.tax) return fail(ctx, MG_ERR_INVALID, "mg_screen_tax_finish_host: no taxonomy bound (mg_screen_set_taxa)");
    const uint64_t m = x.nodes.size(), take = std::min(capacity, m);
    *n_out = m;                                            // (the taxa that carry database hashes: known since set_taxa)
    if (take || total_count) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        uint64_t nt = 0;
        const int rc = screen_touched(sc, &nt);
        if (rc != MG_OK) return rc;
        std::vector<uint32_t> pageable;
        uint32_t *tc = static_cast<uint32_t *>(ctx_pinned(ctx, std::max<uint64_t>(m, 1) * 4));
        if (!tc) { pageable.resize(std::max<uint64_t>(m, 1)); tc = pageable.data(); }
        // (the counters are rebuilt from the touched list on every call: a sizing call and the one that follows it agree)
        hipError_t e = screen_tax_clear(sc, nt);
        if (e == hipSuccess) e = mg::launch_tax_hist(x.slot_node, nt, sc->touched, sc->obs, (uint32_t)x.tax->n, x.count, ctx->stream);
        if (e == hipSuccess) e = mg::launch_tax_gather(x.count, x.list, m, x.vals, ctx->stream);
        if (e == hipSuccess && m) e = hipMemcpyAsync(tc, x.vals, m * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx, MG_ERR_HIP, std::string("mg_screen_tax_finish: ") + hipGetErrorString(e));
        for (uint64_t i = 0; i < take; i++) out[i] = mg_taxon_count{x.nodes[i], tc[i], x.hash_counts[i], tc[i], x.clade_hash_counts[i]};
        // clade sums on the host: the nodes with counts are at most the touched hashes, each walks its ancestors inside the list
        uint64_t total = 0;
        for (uint64_t i = 0; i < m; i++) {
            if (!tc[i]) continue;
            total += tc[i];
            for (int32_t a = x.up[i]; a >= 0; a = x.up[a])
                if ((uint64_t)a < take) out[a].clade_count += tc[i];
        }
        if (total_count) *total_count = total;
    }
    if (total_hash_count) *total_hash_count = sc->distinct;   // every distinct hash is in exactly one bucket
    const uint64_t s = sc->p.sketch_size;
    if (mix_hashes_out) for (uint64_t i = 0; i < s; i++) mix_hashes_out[i] = i < sc->mix.size() ? sc->mix[i] : MG_HASH_PAD;
    if (mix_nhash_out) *mix_nhash_out = (uint32_t)sc->mix.size();
    if (distinct_out) *distinct_out = sc->distinct;
    return MG_OK;
}

// inspection: the key table and slot_node come to the host whole (database-sized; for tests and debugging)
int mg_screen_hash_taxa_host(mg_screen *sc, uint64_t *hashes_out, uint32_t *nodes_out, uint64_t capacity, uint64_t *n_out)
{
    if (!sc) return MG_ERR_INVALID;
    mg_ctx *ctx = sc->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (!n_out || ((!hashes_out || !nodes_out) && capacity)) return fail(ctx, MG_ERR_INVALID, "mg_screen_hash_taxa_host: NULL argument");
    if (!sc->tx.tax) return fail(ctx, MG_ERR_INVALID, "mg_screen_hash_taxa_host: no taxonomy bound (mg_screen_set_taxa)");
    *n_out = sc->distinct;
    if (capacity == 0) return MG_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<unsigned long long> keys(sc->slots);
    std::vector<uint32_t> nodes(sc->slots);
    hipError_t e = hipMemcpyAsync(keys.data(), sc->keys, sc->slots * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(nodes.data(), sc->tx.slot_node, sc->slots * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, MG_ERR_HIP, std::string("mg_screen_hash_taxa: ") + hipGetErrorString(e));
    std::vector<std::pair<uint64_t, uint32_t>> v;
    v.reserve(sc->distinct);
    for (uint64_t i = 0; i < sc->slots; i++)
        if (keys[i] != mg::SCR_EMPTY) v.emplace_back(keys[i], nodes[i]);
    std::sort(v.begin(), v.end());
    for (uint64_t i = 0; i < std::min<uint64_t>(capacity, v.size()); i++) { hashes_out[i] = v[i].first; nodes_out[i] = v[i].second; }
    return MG_OK;
}
