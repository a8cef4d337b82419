// taxscreen_internal.h — launch interface between host_taxscreen.cpp and taxscreen.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mg {

// values of slot_node beside node indices 0 .. n_nodes-1 (the first two = MG_TAX_NONE / MG_TAX_DISJOINT of mashgpu.h)
constexpr uint32_t TAX_NONE = 0xFFFFFFFFu;        // every row of the hash is without a node (the reference's taxID 0)
constexpr uint32_t TAX_DISJOINT = 0xFFFFFFFEu;    // rows under different roots: no common ancestor
constexpr uint32_t TAX_EMPTY = 0xFFFFFFFDu;       // the slot holds no key
// a run of more than TAX_LONG_RUN rows goes to a workgroup (tax_lca_long_kernel) instead of one work-item
constexpr uint32_t TAX_LONG_RUN = 64;

// counters are indexed by bucket: node, or n_nodes for TAX_DISJOINT, n_nodes + 1 for TAX_NONE
// per-hash LCA over the rows-by-slot index: slot_node[slot] for every slot; slots with long runs are listed in long_list
// (*n_long, device) and folded by the second launch, which reads *n_long itself (no host wait in between)
hipError_t launch_tax_lca(uint64_t slots, const uint32_t *slot_end, const uint32_t *ent, const uint32_t *row_node, const uint32_t *parent,
                          const uint32_t *depth, uint32_t *slot_node, uint32_t *long_list, unsigned long long *n_long, uint64_t long_cap,
                          hipStream_t stream);
// counts[bucket(slot_node[slot])] += 1 over every occupied slot (touched == nullptr, n = slots) or over the touched
// slots with obs >= 1 (n = their number)
hipError_t launch_tax_hist(const uint32_t *slot_node, uint64_t n, const uint32_t *touched, const uint32_t *obs, uint32_t n_nodes,
                           uint32_t *counts, hipStream_t stream);
// counts[bucket(slot_node[touched[i]])] = 0
hipError_t launch_tax_clear(const uint32_t *slot_node, const uint32_t *touched, uint64_t nt, uint32_t n_nodes, uint32_t *counts, hipStream_t stream);
// out[i] = counts[list[i]]
hipError_t launch_tax_gather(const uint32_t *counts, const uint32_t *list, uint64_t m, uint32_t *out, hipStream_t stream);

}  // namespace mg
