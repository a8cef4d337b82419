// taxdb.h -- the host side of `mash taxscreen`: NCBI taxonomy dumps, the taxID of every reference, the mapping between taxIDs
// and the dense node indices libmashgpu works on, and the Kraken-style report (replaces taxdb.hpp and
// CommandTaxScreen.cpp:116-165 of the reference; the per-hash LCA and the counts are the library's).
#pragma once
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mashgpu.h"

namespace taxdb {

struct Node {
    uint64_t taxid = 0;
    int64_t parent = -1;                    // position in Taxonomy::nodes; -1: a root (its own parent, or a parent the file lacks)
    std::string rank, name;                 // name: the scientific name
};

struct Taxonomy {
    std::vector<Node> nodes;                // ascending taxID
    std::unordered_map<uint64_t, uint32_t> index;
    // nodes.dmp / names.dmp with the field rules of taxdb.hpp:107-160; false: a file could not be opened (*err says which)
    bool load(const std::string &nodes_file, const std::string &names_file, std::string *err);
    const Node *find(uint64_t taxid) const
    {
        auto it = index.find(taxid);
        return it == index.end() ? nullptr : &nodes[it->second];
    }
};

// taxID per reference: the mapping file first (<taxid><one separator char><reference name to end of line>), else the last
// `taxid <n>` word pair of the comment, else 0 (CommandTaxScreen.cpp:116-165); false: the mapping file could not be opened
bool reference_taxids(const std::vector<std::string> &names, const std::vector<std::string> &comments, const std::string &mapping_file,
                      std::vector<uint64_t> *out);

// The forest handed to mg_taxonomy_create and the node of every database row.  A reference whose taxID is a root or is not
// in the taxonomy gets a node of its own (a root without children): getLowestCommonAncestor answers taxID 1 whenever two
// references meet at a root or one of them is unknown, and keeps the taxID of a single such reference (taxdb.hpp:162-196);
// with private roots the device's "no common ancestor" says exactly that.
struct Binding {
    std::vector<uint32_t> parent, row_node;
    std::vector<uint64_t> private_taxid;    // taxID of node base + i
    uint32_t base = 0;                      // = taxonomy nodes
    Binding(const Taxonomy &tax, const std::vector<uint64_t> &row_taxid);
};

struct Counts {
    uint64_t clade = 0, tax = 0, tax_hash = 0, clade_hash = 0;
};

// the library's per-node counts as the reference's counts[taxID] (CommandTaxScreen.cpp:427-464)
std::map<uint64_t, Counts> counts_by_taxid(const Taxonomy &tax, const Binding &b, const mg_taxon_count *taxa, uint64_t n);

// TaxDB::writeReport, taxdb.hpp:216-257.  Children by descending clade count, ties by ascending taxID (what the reference's
// std::sort gives for up to 16 children; beyond that its order is unspecified).
void write_report(FILE *fp, const Taxonomy &tax, const std::map<uint64_t, Counts> &counts, uint64_t total_count);

}  // namespace taxdb
