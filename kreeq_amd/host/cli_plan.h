// cli_plan.h -- the decisions of the CLI that need no GPU: what -o asks for, how whole sequences are grouped into device calls,
// and how a call's segments are cut into formatted chunks.  Pure functions (tests/native/cli_plan_main.cpp runs them on the host).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "fastx.h"
#include "kreeq_amd.h"

namespace kqhost {

// extension after the last '.', keeping a trailing ".gz" attached ("x.gfa.gz" -> "gfa.gz")
inline std::string file_ext(const std::string& path) {
    std::string p = path;
    std::string gz;
    if (p.size() > 3 && p.substr(p.size() - 3) == ".gz") { gz = ".gz"; p.resize(p.size() - 3); }
    size_t dot = p.rfind('.');
    if (dot == std::string::npos) return "";
    return p.substr(dot + 1) + gz;
}

// What -o asks for (DBG::report, src/kreeq-output.cpp:34-136).  A name without a dot IS its extension ("-o vcf": the records
// go to stdout) and prints no QV table (src/kreeq.cpp:78); the reference's first switch has no case for .kreeq / .hist, so
// they validate like every other extension (:62-72).
struct OutPlan {
    std::string ext = "stdout";
    bool want_stats = true, want_qv = true;                     // the summary block; the QV table of a validation
    bool per_base = false, vcf = false, kreeq = false, hist = false;
    bool refused = false;                                       // validate -o x.gfa*: the variant graph is not built
    bool table_gz = false;                                      // x.kwig.gz / x.bed.gz / x.csvtable.gz: the text table as BGZF; per_base stays
    std::string table_ext;                                      // false and ext keeps its ".gz"; table_ext is the format inside
    bool tables() const { return per_base || table_gz; }        // a per-base file is written, plain or compressed
    const std::string& table_format() const { return table_gz ? table_ext : ext; }
};
inline OutPlan plan_output(int mode, const std::string& out_file) {
    OutPlan p;
    if (out_file != "") p.ext = file_ext("." + out_file);
    p.kreeq = p.ext == "kreeq"; p.vcf = p.ext == "vcf"; p.hist = p.ext == "hist";
    p.per_base = p.ext == "kwig" || p.ext == "bkwig" || p.ext == "bed" || p.ext == "csvtable";
    p.table_gz = p.ext == "kwig.gz" || p.ext == "bed.gz" || p.ext == "csvtable.gz";      // (.bkwig is binary and compact already: no .bkwig.gz)
    if (p.table_gz) p.table_ext = p.ext.substr(0, p.ext.size() - 3);
    p.want_qv = out_file.find(".") != std::string::npos || out_file == "";
    p.want_stats = p.want_qv || p.kreeq;
    p.refused = mode == 0 && (p.ext == "gfa" || p.ext == "gfa2" || p.ext == "gfa.gz" || p.ext == "gfa2.gz");
    return p;
}

// ---- whole sequences per device call ------------------------------------------------------------------------------------
constexpr uint64_t kDeviceCallBytes = 1ull << 30;               // joined text per kq_lookup_sequence_dev / kq_search_variants call

struct JoinedSeqs {
    std::string text;                 // the sequences, each followed by '\n' (a non-ACGT byte ends every segment)
    std::vector<uint64_t> offset;     // start of each sequence inside `text`
};
inline JoinedSeqs join_sequences(const std::vector<SeqRecord>& seqs, size_t lo, size_t hi) {
    JoinedSeqs j;
    size_t total = 0;
    for (size_t s = lo; s < hi; ++s) total += seqs[s].seq.size() + 1;
    j.text.reserve(total);
    for (size_t s = lo; s < hi; ++s) { j.offset.push_back(j.text.size()); j.text += seqs[s].seq; j.text.push_back('\n'); }
    return j;
}
// the call that starts at sequence lo ends before the returned one: whole sequences while the joined bytes stay within
// `limit`, and always at least one
inline size_t next_call(const std::vector<SeqRecord>& seqs, size_t lo, uint64_t limit) {
    size_t hi = lo;
    uint64_t len = 0;
    while (hi < seqs.size() && (hi == lo || len + seqs[hi].seq.size() + 1 <= limit)) { len += seqs[hi].seq.size() + 1; ++hi; }
    return hi;
}
inline bool all_fit(const std::vector<SeqRecord>& seqs, uint64_t limit) {
    for (auto& s : seqs) if (s.seq.size() + 1 > limit) return false;
    return true;
}

// ---- per-base tables ----------------------------------------------------------------------------------------------------
inline bool is_base(char c) {
    switch (c) { case 'A': case 'C': case 'G': case 'T': case 'a': case 'c': case 'g': case 't': return true; default: return false; }
}
// segments of one sequence = maximal runs of bases (gfalibs appendSequence splits at N runs)
inline std::vector<std::pair<uint64_t, uint64_t>> segments_of(const std::string& s) {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    for (uint64_t i = 0; i < s.size();) {
        if (!is_base(s[i])) { ++i; continue; }
        uint64_t j = i;
        while (j < s.size() && is_base(s[j])) ++j;
        out.emplace_back(i, j - i);
        i = j;
    }
    return out;
}
typedef std::vector<std::vector<std::pair<uint64_t, uint64_t>>> SegmentLists;      // per sequence: (start, length) of its segments
inline SegmentLists all_segments(const std::vector<SeqRecord>& seqs) {
    SegmentLists segs;
    for (auto& s : seqs) segs.push_back(segments_of(s.seq));
    return segs;
}

struct Triple { uint32_t cov, fw, bw; };                        // one position of a per-base table, as the .bkwig payload holds it
inline Triple oriented(const kq_dbgbase& b) { return {b.cov, b.isFw ? b.fw : b.bw, b.isFw ? b.bw : b.fw}; }

// The per-base table of a run in map ranges, accumulated on the device: the triples of the whole genome lie in one array,
// segment after segment, and every range looks the sequences up group by group (next_call) into one text buffer and one
// per-base array sized for the largest group.  A group's segment lists are rebased to its text (kq_per_base_merge_dev takes
// them as they are), and its triples begin at first_triple of the accumulator.
struct TableGroup {
    size_t lo = 0, hi = 0;                                      // its sequences
    uint64_t text_off = 0, text_len = 0;                        // its range of the joined text (join_sequences over all sequences)
    std::vector<uint64_t> seg_start, seg_len;                   // seg_start: inside the group's text
    uint64_t first_triple = 0, n_triples = 0;
};
struct TablePassPlan {
    std::vector<TableGroup> groups;
    bool fits = true;                                           // false: a sequence (with its separator) exceeds the limit
    uint64_t acc_bytes = 0, max_text = 0, max_per_base = 0;     // 12 x positions; the largest group's text and per-base array
    uint64_t device_bytes() const { return acc_bytes + max_text + max_per_base; }
};
inline TablePassPlan plan_table_passes(const std::vector<SeqRecord>& seqs, const SegmentLists& segs, uint64_t limit) {
    TablePassPlan p;
    p.fits = all_fit(seqs, limit);
    uint64_t text_off = 0, first = 0;
    for (size_t lo = 0, hi; lo < seqs.size(); lo = hi) {
        hi = next_call(seqs, lo, limit);
        TableGroup g;
        g.lo = lo; g.hi = hi; g.text_off = text_off; g.first_triple = first;
        for (size_t s = lo; s < hi; ++s) {
            for (auto& seg : segs[s]) { g.seg_start.push_back(g.text_len + seg.first); g.seg_len.push_back(seg.second); g.n_triples += seg.second; }
            g.text_len += seqs[s].seq.size() + 1;
        }
        text_off += g.text_len; first += g.n_triples;
        p.max_text = std::max(p.max_text, g.text_len);
        p.max_per_base = std::max(p.max_per_base, g.text_len * (uint64_t)sizeof(kq_dbgbase));
        p.groups.push_back(std::move(g));
    }
    p.acc_bytes = first * sizeof(Triple);
    return p;
}

// The segments of sequences [lo, hi) -- one device call, whose triples lie segment after segment -- cut into chunks of at most
// `chunk` lines for kq_format_table_dev: whole segments or parts of one.  The first piece of a segment carries the header
// flag; a later piece of an expanded table (.bed / .csvtable) has up to k - 1 positions before it as its window's history.
// name_off has one entry per sequence and one behind: where its header lies in the concatenated names.
inline std::vector<std::vector<kq_table_seg>> cut_table_chunks(const SegmentLists& segs, size_t lo, size_t hi, const std::vector<uint32_t>& name_off,
                                                               uint64_t chunk, int k, bool expanded) {
    std::vector<std::vector<kq_table_seg>> chunks(1);
    uint64_t lines = 0, first = 0;                              // first: triple index of the segment inside the call
    for (size_t s = lo; s < hi; ++s)
        for (auto& seg : segs[s]) {
            for (uint64_t done = 0; done < seg.second;) {
                const uint64_t take = std::min(seg.second - done, chunk - lines);
                kq_table_seg p{};
                p.first = first + done; p.n = take; p.abs_pos = seg.first + done;
                p.name_off = name_off[s]; p.name_len = name_off[s + 1] - name_off[s];
                p.n_ctx = expanded ? (uint32_t)std::min<uint64_t>(done, (uint64_t)k - 1) : 0;
                p.flags = done == 0 ? KQ_TABLE_SEG_HEADER : 0;
                chunks.back().push_back(p);
                lines += take; done += take;
                if (lines >= chunk) { chunks.emplace_back(); lines = 0; }
            }
            first += seg.second;
        }
    if (chunks.back().empty()) chunks.pop_back();
    return chunks;
}

}  // namespace kqhost
