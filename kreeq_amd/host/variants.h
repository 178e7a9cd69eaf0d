// Candidate-error search behind `kreeq validate -o vcf` (reference src/variants.cpp); see variants.cpp.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "fastx.h"
#include "kreeq_amd.h"

namespace kqhost {

enum VariantType { VAR_SNV, VAR_INS, VAR_DEL, VAR_COM };        // gfalibs DBGpath::type as src/variants.cpp:283-297 assigns it

struct DbgPath {                                                // gfalibs DBGpath: one alternative path found at a position
    VariantType type = VAR_SNV;
    uint64_t pos = 0;                                           // first base behind the source k-mer, inside its segment (src/variants.cpp:139-140)
    std::string sequence;
    uint32_t ref_len = 0;                                       // COM only: original bases replaced
};
struct VariantSite { size_t seq_index = 0; uint64_t seg_start = 0; std::vector<DbgPath> paths; };

// Where the search gets the graph from.  One resident table (graph_of_handle), or a database that is loaded map range by
// map range (the reference's search loops over map ranges the same way, src/variants.cpp:78-84, with a cache of what it has
// seen, :199-210): branch_scan fills flags[c] for every k-mer start of `joined` (kq_branch_scan's contract), lookup the
// logical entry of every key of `want` (kq_lookup_keys' contract).
struct GraphSource {
    std::function<void(const std::string& joined, uint32_t cov_cutoff, std::vector<uint8_t>& flags)> branch_scan;
    std::function<void(const std::vector<uint64_t>& want, std::vector<kq_entry>& got)> lookup;
    kq_handle* resident = nullptr;                              // the one table that holds the whole graph (graph_of_handle); null under map-range passes
};
GraphSource graph_of_handle(kq_handle* h);

// The device limits of kq_search_variants as the CLI uses them.  max_span 0 stays with the host search: the reference pops an
// empty queue there, and the host search (no target) and the device search (the pop skipped: one target, k-mer c + k) differ.
constexpr int kVcfDeviceMaxDepth = 253, kVcfDeviceMinSpan = 1, kVcfDeviceMaxSpan = 255;

// DBG::correctSequences over all sequences: device pre-filter + host searches with batched device lookups.  With KQ_VCF_DEVICE=1
// (off by default), a resident table, depth and span inside the device limits and no sequence above kDeviceCallBytes (cli_plan.h), the
// searches run on the device instead (kq_search_variants), whole sequences grouped into calls; the sites are the same.
std::vector<VariantSite> find_candidate_errors(const GraphSource& g, int k, const std::vector<SeqRecord>& seqs, int kmer_depth, int max_span,
                                               uint32_t cov_cutoff, const std::function<void(const std::string&)>& log = nullptr);
inline std::vector<VariantSite> find_candidate_errors(kq_handle* h, int k, const std::vector<SeqRecord>& seqs, int kmer_depth, int max_span,
                                                      uint32_t cov_cutoff, const std::function<void(const std::string&)>& log = nullptr) {
    return find_candidate_errors(graph_of_handle(h), k, seqs, kmer_depth, max_span, cov_cutoff, log);
}
// the VCF text of the sites (header + one record per path)
std::vector<std::string> vcf_lines(const std::vector<SeqRecord>& seqs, const std::vector<VariantSite>& sites);

}  // namespace kqhost
