// gfa_out.h -- the host side of `kreeq subgraph`'s graph output: GFA 1 text and the numbers of the "+++Assembly summary+++"
// block from the three arrays of kq_subgraph_gfa.  Pure functions, no device call (tests/native/gfa_out_main.cpp runs them on
// the host under sanitizers).
//
// The text (reference DBG::DBGgraphToGFA, src/kreeq.cpp:523-600, through gfalibs' writer): a header, all segments, all links.
//   H	VN:Z:1.0
//   S	<id>	<bases>	DP:f:<cov>
//   L	<a>	<sign>	<b>	<sign>	<k-1>M	KC:i:<count>
// No CB colour tag: the table keeps no colour.  The block has the reference's layout line for line (gfalibs Report::reportStats)
// without `# separated components` and `# bubbles`, whose definitions live in gfalibs; a subgraph has no scaffolds, contigs,
// gaps or paths, so those lines are the constants every run of the reference prints.
#pragma once
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "kreeq_amd.h"

namespace kqhost {

struct GfaGraph {
    int k = 0;
    std::vector<kq_gfa_segment> segs;
    std::string seq;
    std::vector<kq_gfa_edge> edges;
};

inline uint64_t gfa_segment_len(const GfaGraph& g, const kq_gfa_segment& s) { return (uint64_t)s.n_kmers + (uint64_t)g.k - 1; }

// false when a record points outside its array (nothing is appended then)
inline bool gfa_valid(const GfaGraph& g) {
    for (auto& s : g.segs)
        if (s.n_kmers == 0 || s.seq_off > g.seq.size() || gfa_segment_len(g, s) > g.seq.size() - s.seq_off) return false;
    for (auto& e : g.edges)
        if (e.from >= g.segs.size() || e.to >= g.segs.size()) return false;
    return true;
}

inline void gfa_text(const GfaGraph& g, std::string& out) {
    out += "H\tVN:Z:1.0\n";
    for (size_t i = 0; i < g.segs.size(); ++i) {
        const kq_gfa_segment& s = g.segs[i];
        out += "S\t" + std::to_string(i) + "\t";
        out.append(g.seq, (size_t)s.seq_off, (size_t)gfa_segment_len(g, s));
        out += "\tDP:f:" + std::to_string(s.cov) + "\n";
    }
    const std::string overlap = std::to_string(g.k - 1) + "M\tKC:i:";
    for (auto& e : g.edges) {
        out += "L\t" + std::to_string(e.from) + (e.from_rc ? "\t-\t" : "\t+\t") + std::to_string(e.to) + (e.to_rc ? "\t-\t" : "\t+\t") + overlap + std::to_string(e.count) + "\n";
    }
}

struct GfaStats {
    uint64_t segments = 0, total_len = 0, edges = 0, components = 0, largest = 0, dead_ends = 0, disconnected = 0, disconnected_len = 0, circular = 0;
};

// components: segments joined by links (union-find); dead ends: segment ends no link touches; disconnected: segments no link
// touches; circular: a link from a segment's own + end to its own + start, or - to -
inline GfaStats gfa_stats(const GfaGraph& g) {
    GfaStats st;
    const size_t n = g.segs.size();
    st.segments = n; st.edges = g.edges.size();
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t a) {
        while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; }
        return a;
    };
    std::vector<uint8_t> touched(n, 0), circular(n, 0);                  // bit 0: the + start, bit 1: the + end
    for (auto& e : g.edges) {
        if (e.from >= n || e.to >= n) continue;                          // (gfa_valid refuses such a graph)
        const uint32_t ra = find(e.from), rb = find(e.to);
        if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
        touched[e.from] |= e.from_rc ? 1 : 2;
        touched[e.to] |= e.to_rc ? 2 : 1;
        if (e.from == e.to && (e.from_rc != 0) == (e.to_rc != 0)) circular[e.from] = 1;
    }
    std::vector<uint64_t> comp_len(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const uint64_t len = gfa_segment_len(g, g.segs[i]);
        st.total_len += len;
        comp_len[find((uint32_t)i)] += len;
        st.dead_ends += 2 - (touched[i] & 1) - ((touched[i] >> 1) & 1);
        if (!touched[i]) { ++st.disconnected; st.disconnected_len += len; }
        st.circular += circular[i];
    }
    for (size_t i = 0; i < n; ++i)
        if (parent[i] == i) { ++st.components; st.largest = std::max(st.largest, comp_len[i]); }
    return st;
}

inline std::string gfa_ratio(uint64_t a, uint64_t b) {
    if (!b) return "nan";
    char buf[64];
    snprintf(buf, sizeof buf, "%.2f", (double)a / (double)b);
    return buf;
}

inline void gfa_block(const GfaStats& s, std::string& out) {
    out += "+++Assembly summary+++: \n# scaffolds: 0\nTotal scaffold length: 0\nAverage scaffold length: nan\nScaffold N50: 0\nScaffold auN: 0.00\n"
           "Scaffold L50: 0\nLargest scaffold: 0\nSmallest scaffold: 0\n# contigs: 0\nTotal contig length: 0\nAverage contig length: nan\nContig N50: 0\n"
           "Contig auN: 0.00\nContig L50: 0\nLargest contig: 0\nSmallest contig: 0\n# gaps in scaffolds: 0\nTotal gap length in scaffolds: 0\n"
           "Average gap length in scaffolds: 0.00\nGap N50 in scaffolds: 0\nGap auN in scaffolds: 0.00\nGap L50 in scaffolds: 0\nLargest gap in scaffolds: 0\n"
           "Smallest gap in scaffolds: 0\nBase composition (A:C:G:T): 0:0:0:0\nGC content %: nan\n# soft-masked bases: 0\n";
    out += "# segments: " + std::to_string(s.segments) + "\nTotal segment length: " + std::to_string(s.total_len) + "\nAverage segment length: " + gfa_ratio(s.total_len, s.segments) +
           "\n# gaps: 0\n# paths: 0\n# edges: " + std::to_string(s.edges) + "\nAverage degree: " + gfa_ratio(s.edges, s.segments) + "\n# connected components: " +
           std::to_string(s.components) + "\nLargest connected component length: " + std::to_string(s.largest) + "\n# dead ends: " + std::to_string(s.dead_ends) +
           "\n# disconnected components: " + std::to_string(s.disconnected) + "\nTotal length disconnected components: " + std::to_string(s.disconnected_len) +
           "\n# circular segments: " + std::to_string(s.circular) + "\n# circular paths: 0\n";
}

}  // namespace kqhost
