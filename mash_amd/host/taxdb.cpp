// taxdb.cpp -- see taxdb.h
#include "taxdb.h"

#include <algorithm>
#include <fstream>
#include <sstream>

namespace taxdb {

// fields of a dump line: separated by "\t|", every field but the first starts with the tab that follows the bar
static std::vector<std::string> dump_fields(const std::string &line)
{
    std::vector<std::string> f;
    size_t at = 0;
    for (;;) {
        const size_t e = line.find("\t|", at);
        f.push_back(line.substr(at, e == std::string::npos ? std::string::npos : e - at));
        if (e == std::string::npos) break;
        at = e + 2;
        if (at < line.size() && line[at] == '\t') at++;
    }
    return f;
}

bool Taxonomy::load(const std::string &nodes_file, const std::string &names_file, std::string *err)
{
    std::ifstream nf(nodes_file);
    if (!nf.is_open()) { *err = "unable to open nodes file"; return false; }
    std::map<uint64_t, std::pair<uint64_t, std::string>> seen;            // taxID -> (parent taxID, rank); the first line of a taxID wins
    std::string line;
    while (std::getline(nf, line)) {
        const std::vector<std::string> f = dump_fields(line);
        if (f.size() < 3 || f[0].empty()) continue;
        char *end;
        const uint64_t t = strtoull(f[0].c_str(), &end, 10);
        if (end == f[0].c_str()) break;                                      // (the reference stops at the first line it cannot read)
        seen.emplace(t, std::make_pair(strtoull(f[1].c_str(), nullptr, 10), f[2]));
    }
    nodes.clear();
    index.clear();
    for (const auto &kv : seen) {
        index[kv.first] = (uint32_t)nodes.size();
        Node n;
        n.taxid = kv.first;
        n.rank = kv.second.second;
        nodes.push_back(n);
    }
    for (Node &n : nodes) {
        const uint64_t p = seen[n.taxid].first;
        auto it = index.find(p);
        n.parent = (p == n.taxid || it == index.end()) ? -1 : (int64_t)it->second;
    }
    std::ifstream mf(names_file);
    if (!mf.is_open()) { *err = "unable to open names file"; return false; }
    while (std::getline(mf, line)) {
        const std::vector<std::string> f = dump_fields(line);
        if (f.size() < 4 || f[3] != "scientific name") continue;
        auto it = index.find(strtoull(f[0].c_str(), nullptr, 10));
        if (it != index.end()) nodes[it->second].name = f[1];
    }
    return true;
}

bool reference_taxids(const std::vector<std::string> &names, const std::vector<std::string> &comments, const std::string &mapping_file,
                      std::vector<uint64_t> *out)
{
    std::unordered_map<std::string, uint64_t> by_name;
    if (!mapping_file.empty()) {
        std::ifstream mf(mapping_file);
        if (!mf.is_open()) return false;
        uint64_t t;
        std::string name;
        while (mf >> t) {
            mf.ignore(1);
            std::getline(mf, name, '\n');
            by_name.emplace(name, t);
        }
    }
    out->assign(names.size(), 0);
    for (size_t i = 0; i < names.size(); i++) {
        uint64_t t = 0;
        auto it = by_name.find(names[i]);
        if (it != by_name.end()) t = it->second;
        if (t == 0) {
            std::istringstream words(comments[i]);
            std::string w;
            while (words >> w)
                if (w == "taxid") words >> t;                                 // (a word that is no number leaves 0 and ends the scan)
        }
        (*out)[i] = t;
    }
    return true;
}

Binding::Binding(const Taxonomy &tax, const std::vector<uint64_t> &row_taxid)
{
    base = (uint32_t)tax.nodes.size();
    parent.resize(base);
    for (uint32_t i = 0; i < base; i++) parent[i] = tax.nodes[i].parent < 0 ? i : (uint32_t)tax.nodes[i].parent;
    row_node.resize(row_taxid.size());
    for (size_t r = 0; r < row_taxid.size(); r++) {
        const uint64_t t = row_taxid[r];
        if (t == 0) { row_node[r] = MG_TAX_NONE; continue; }
        auto it = tax.index.find(t);
        if (it != tax.index.end() && tax.nodes[it->second].parent >= 0) { row_node[r] = it->second; continue; }
        row_node[r] = (uint32_t)parent.size();
        parent.push_back((uint32_t)parent.size());
        private_taxid.push_back(t);
    }
    if (parent.empty()) { parent.push_back(0); }                             // (an empty taxonomy and no reference with a taxID: one unused root)
}

std::map<uint64_t, Counts> counts_by_taxid(const Taxonomy &tax, const Binding &b, const mg_taxon_count *taxa, uint64_t n)
{
    std::map<uint64_t, Counts> counts;
    // hashes the reference files under a taxID other than their node's: own counts only, the clade sums follow below
    auto own = [&](uint64_t taxid, const mg_taxon_count &e) {
        Counts &c = counts[taxid];
        c.tax += e.tax_count;
        c.tax_hash += e.tax_hash_count;
        for (const Node *v = tax.find(taxid); v; v = v->parent < 0 ? nullptr : &tax.nodes[v->parent]) {
            Counts &a = counts[v->taxid];
            a.clade += e.tax_count;
            a.clade_hash += e.tax_hash_count;
        }
    };
    for (uint64_t i = 0; i < n; i++) {
        const mg_taxon_count &e = taxa[i];
        if (e.node == MG_TAX_NONE) own(0, e);
        else if (e.node == MG_TAX_DISJOINT) own(1, e);
        else if (e.node >= b.base) own(b.private_taxid[e.node - b.base], e);
        else if (tax.nodes[e.node].parent < 0 && tax.nodes[e.node].taxid != 1) own(1, e);   // references met at another root: the reference answers taxID 1
        else {
            Counts &c = counts[tax.nodes[e.node].taxid];
            c.tax += e.tax_count;
            c.tax_hash += e.tax_hash_count;
            c.clade += e.clade_count;
            c.clade_hash += e.clade_hash_count;
        }
    }
    return counts;
}

static void report_node(FILE *fp, const Taxonomy &tax, const std::map<uint64_t, Counts> &counts,
                        const std::unordered_map<uint64_t, std::vector<uint64_t>> &children, uint64_t total, uint64_t taxid, int depth)
{
    auto it = counts.find(taxid);
    const Node *node = tax.find(taxid);
    if (it == counts.end() || it->second.clade == 0 || !node) return;
    const Counts &c = it->second;
    fprintf(fp, "%.4f\t%i\t%i\t%i\t%i\t%s\t%llu\t%s%s\n", 100 * (unsigned)c.clade / double(total), (unsigned)c.clade, (unsigned)c.tax, (unsigned)c.clade_hash,
            (unsigned)c.tax_hash, node->rank.c_str(), (unsigned long long)taxid, std::string(2 * depth, ' ').c_str(), node->name.c_str());
    auto ch = children.find(taxid);
    if (ch == children.end()) return;
    std::vector<uint64_t> order = ch->second;                                // ascending taxID (counts is an ordered map)
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return counts.at(a).clade > counts.at(b).clade; });
    for (uint64_t t : order) report_node(fp, tax, counts, children, total, t, depth + 1);
}

void write_report(FILE *fp, const Taxonomy &tax, const std::map<uint64_t, Counts> &counts, uint64_t total_count)
{
    fprintf(fp, "%%\thashes\ttaxHashes\thashesDB\ttaxHashesDB\ttaxID\trank\tname\n");
    // (the reference's `unclassified` line needs a clade count under taxID 0, which its clade loop never gives: getEntry(0)
    //  fails; hashes without a taxon are in total_count and have no line)
    std::unordered_map<uint64_t, std::vector<uint64_t>> children;
    for (const auto &kv : counts) {
        const Node *v = tax.find(kv.first);
        if (v && v->parent >= 0 && kv.second.clade > 0) children[tax.nodes[v->parent].taxid].push_back(kv.first);
    }
    report_node(fp, tax, counts, children, total_count, 1, 0);
}

}  // namespace taxdb
