// Best-first expansion of `kreeq subgraph` (reference DBG::bestFirst / dijkstra, src/subgraph.cpp:417-579); see subgraph.cpp.
#pragma once
#include <cstdint>
#include <functional>
#include <string>

#include "kreeq_amd.h"

namespace kqhost {

// One search per k-mer of `sub` (the seeds) through the graph of `db`; what the searches discover is added to `sub` with
// its database entry after the last one.  Returns the number of k-mers added.  Throws std::runtime_error on an ABI error.
uint64_t subgraph_best_first(kq_handle* db, kq_handle* sub, int k, int map_count, int kmer_depth, uint32_t cov_cutoff,
                             const std::function<void(const std::string&)>& log = nullptr);

}  // namespace kqhost
