// The GPU-free decisions of the CLI (kreeq_amd/host/cli_plan.h) as a stand-alone host program: the output plan against a table
// written out by hand, the grouping of sequences into device calls at a small limit, and the cutter of formatted chunks.
#include <cstdio>
#include <string>
#include <vector>

#include "cli_plan.h"

using namespace kqhost;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

// ---- output plan: (mode, -o) -> ext, stats, qv, per_base, vcf, kreeq, hist, refused ----------------------------------------
struct PlanRow { int mode; const char* out; const char* ext; int stats, qv, per_base, vcf, kreeq, hist, refused; };
static const PlanRow kPlans[] = {
    {0, "", "stdout", 1, 1, 0, 0, 0, 0, 0},
    {0, "vcf", "vcf", 0, 0, 0, 1, 0, 0, 0},                  // a name without a dot is its extension: no summary, no QV table
    {0, "x.vcf", "vcf", 1, 1, 0, 1, 0, 0, 0},
    {0, "x.kreeq", "kreeq", 1, 1, 0, 0, 1, 0, 0},
    {0, "kreeq", "kreeq", 1, 0, 0, 0, 1, 0, 0},              // the summary is printed for a database even without a dot
    {0, "run.1/db.kreeq", "kreeq", 1, 1, 0, 0, 1, 0, 0},
    {0, "dir.kreeq/x", "kreeq/x", 1, 1, 0, 0, 0, 0, 0},      // a dot earlier in the path: no format, but summary and QV
    {0, "out.d/name", "d/name", 1, 1, 0, 0, 0, 0, 0},
    {0, "x.kwig", "kwig", 1, 1, 1, 0, 0, 0, 0},
    {0, "x.bkwig", "bkwig", 1, 1, 1, 0, 0, 0, 0},
    {0, "x.bed", "bed", 1, 1, 1, 0, 0, 0, 0},
    {0, "x.csvtable", "csvtable", 1, 1, 1, 0, 0, 0, 0},
    {0, "bkwig", "bkwig", 0, 0, 1, 0, 0, 0, 0},
    {0, "x.kwig.gz", "kwig.gz", 1, 1, 0, 0, 0, 0, 0},
    {0, "x.hist", "hist", 1, 1, 0, 0, 0, 1, 0},
    {0, "hist", "hist", 0, 0, 0, 0, 0, 1, 0},
    {0, "x.unknownext", "unknownext", 1, 1, 0, 0, 0, 0, 0},
    {0, "x.gfa", "gfa", 1, 1, 0, 0, 0, 0, 1},
    {0, "x.gfa2", "gfa2", 1, 1, 0, 0, 0, 0, 1},
    {0, "x.gfa.gz", "gfa.gz", 1, 1, 0, 0, 0, 0, 1},
    {0, "x.gfa2.gz", "gfa2.gz", 1, 1, 0, 0, 0, 0, 1},
    {0, "gfa", "gfa", 0, 0, 0, 0, 0, 0, 1},
    {0, "name", "name", 0, 0, 0, 0, 0, 0, 0},
    {1, "", "stdout", 1, 1, 0, 0, 0, 0, 0},
    {1, "u.kreeq", "kreeq", 1, 1, 0, 0, 1, 0, 0},
    {1, "u.hist", "hist", 1, 1, 0, 0, 0, 1, 0},
    {1, "u.gfa", "gfa", 1, 1, 0, 0, 0, 0, 0},                // union has never refused it: it prints the summary and writes nothing
};

static void test_plans() {
    for (const PlanRow& w : kPlans) {
        const OutPlan p = plan_output(w.mode, w.out);
        CHECK(p.ext == w.ext, "-o '%s': ext '%s'", w.out, p.ext.c_str());
        CHECK(p.want_stats == !!w.stats && p.want_qv == !!w.qv && p.per_base == !!w.per_base && p.vcf == !!w.vcf && p.kreeq == !!w.kreeq &&
              p.hist == !!w.hist && p.refused == !!w.refused,
              "mode %d -o '%s': stats %d qv %d per_base %d vcf %d kreeq %d hist %d refused %d", w.mode, w.out, p.want_stats, p.want_qv, p.per_base, p.vcf,
              p.kreeq, p.hist, p.refused);
    }
}

// ---- call grouping ------------------------------------------------------------------------------------------------------
static std::vector<SeqRecord> seqs_of_lengths(const std::vector<size_t>& lens) {
    std::vector<SeqRecord> seqs;
    for (size_t i = 0; i < lens.size(); ++i) { SeqRecord r; r.header = "s" + std::to_string(i); r.seq = std::string(lens[i], "ACGT"[i % 4]); seqs.push_back(r); }
    return seqs;
}

static void test_calls() {
    const uint64_t limit = 8;
    struct Case { std::vector<size_t> lens; std::vector<size_t> ends; bool fit; };      // ends: the sequence behind each call
    const std::vector<Case> cases = {
        {{}, {}, true},
        {{7}, {1}, true},                                    // limit - 1 bases and the separator: fits
        {{8}, {1}, false},                                   // limit bases do not fit, and still form a call
        {{0}, {1}, true},
        {{7, 7}, {1, 2}, true},
        {{3, 3}, {2}, true},                                 // the last sequence ends exactly at the limit
        {{3, 3, 0}, {2, 3}, true},
        {{0, 0, 0, 0, 0, 0, 0, 0, 0}, {8, 9}, true},         // empty sequences cost their separator
        {{2, 8, 2}, {1, 2, 3}, false},
        {{2, 9, 0, 0, 6}, {1, 2, 4, 5}, false},
        {{1, 2, 1, 4, 2}, {3, 5}, true},
    };
    for (size_t c = 0; c < cases.size(); ++c) {
        const std::vector<SeqRecord> seqs = seqs_of_lengths(cases[c].lens);
        std::vector<size_t> ends;
        bool within = true;
        for (size_t lo = 0; lo < seqs.size();) {
            const size_t hi = next_call(seqs, lo, limit);
            CHECK(hi > lo && hi <= seqs.size(), "case %zu: call [%zu, %zu)", c, lo, hi);
            if (hi <= lo) break;
            const JoinedSeqs j = join_sequences(seqs, lo, hi);
            CHECK(j.offset.size() == hi - lo, "case %zu: %zu offsets", c, j.offset.size());
            CHECK(j.text.size() <= limit || hi == lo + 1, "case %zu: call [%zu, %zu) holds %zu bytes", c, lo, hi, j.text.size());
            within = within && j.text.size() <= limit;
            for (size_t s = lo; s < hi; ++s)                 // every sequence where its offset says, its separator behind it
                CHECK(j.text.compare((size_t)j.offset[s - lo], seqs[s].seq.size() + 1, seqs[s].seq + "\n") == 0, "case %zu: sequence %zu", c, s);
            if (hi < seqs.size()) CHECK(j.text.size() + seqs[hi].seq.size() + 1 > limit, "case %zu: sequence %zu would have fitted", c, hi);
            ends.push_back(hi);
            lo = hi;                                         // (in order, and each sequence in exactly one call)
        }
        CHECK(ends == cases[c].ends, "case %zu: %zu calls", c, ends.size());
        CHECK(all_fit(seqs, limit) == cases[c].fit && within == cases[c].fit, "case %zu: all_fit %d, every call within the limit %d", c, all_fit(seqs, limit), within);
    }
}

// ---- piece cutter -------------------------------------------------------------------------------------------------------
static void check_cut(const std::vector<SeqRecord>& seqs, const SegmentLists& segs, const std::vector<uint32_t>& name_off, size_t lo, size_t hi,
                      uint64_t chunk, int k, bool expanded) {
    const auto chunks = cut_table_chunks(segs, lo, hi, name_off, chunk, k, expanded);
    size_t ci = 0, pi = 0;                                   // the piece expected next
    uint64_t lines = 0, first = 0, total = 0;
    for (size_t s = lo; s < hi; ++s)
        for (auto& seg : segs[s]) {
            for (uint64_t done = 0; done < seg.second;) {
                if (ci < chunks.size() && pi == chunks[ci].size()) { ++ci; pi = 0; lines = 0; }
                CHECK(ci < chunks.size(), "k %d chunk %llu: the pieces end at sequence %zu", k, (unsigned long long)chunk, s);
                if (ci >= chunks.size()) return;
                const kq_table_seg& p = chunks[ci][pi++];
                CHECK(p.n >= 1 && p.n <= seg.second - done, "piece of %llu positions", (unsigned long long)p.n);
                if (p.n < 1 || p.n > seg.second - done) return;
                CHECK(p.first == first + done && p.abs_pos == seg.first + done, "k %d chunk %llu: first %llu abs_pos %llu", k, (unsigned long long)chunk,
                      (unsigned long long)p.first, (unsigned long long)p.abs_pos);
                CHECK(p.flags == (done == 0 ? (uint32_t)KQ_TABLE_SEG_HEADER : 0u), "flags %u at done %llu", p.flags, (unsigned long long)done);
                CHECK(p.n_ctx == (expanded ? (uint32_t)std::min<uint64_t>(done, (uint64_t)k - 1) : 0u), "n_ctx %u at done %llu", p.n_ctx, (unsigned long long)done);
                CHECK(p.first >= p.n_ctx, "the history starts before the call's triples");
                CHECK(p.name_off == name_off[s] && p.name_len == seqs[s].header.size(), "name %u + %u of sequence %zu", p.name_off, p.name_len, s);
                lines += p.n; done += p.n; total += p.n;
                CHECK(lines <= chunk, "k %d: a chunk of %llu lines, limit %llu", k, (unsigned long long)lines, (unsigned long long)chunk);
            }
            first += seg.second;
        }
    CHECK(total == first, "positions");
    CHECK(total == 0 ? chunks.empty() : (ci + 1 == chunks.size() && pi == chunks[ci].size()), "k %d chunk %llu: pieces left over", k, (unsigned long long)chunk);
    for (size_t c = 0; c + 1 < chunks.size(); ++c) {         // every chunk but the last is full
        uint64_t n = 0;
        for (auto& p : chunks[c]) n += p.n;
        CHECK(n == chunk, "chunk %zu holds %llu lines of %llu", c, (unsigned long long)n, (unsigned long long)chunk);
    }
}

static void test_cutter() {
    std::vector<SeqRecord> seqs(5);
    seqs[0].header = "s0";       seqs[0].seq = "ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTA";      // one segment of 41
    seqs[1].header = "gap";      seqs[1].seq = "NNNN";                                           // no segment
    seqs[2].header = "seq_two";  seqs[2].seq = "ACNGTACGTANNAnnacgtacgtacgtACGTACGTACGTACGTACGTACGTAC";      // (0,2) (3,7) (12,1) (15,38)
    seqs[3].header = "";         seqs[3].seq = "";
    seqs[4].header = "last";     seqs[4].seq = "NACGTN";                                         // (1,4): shorter than k = 5, 32
    const SegmentLists segs = all_segments(seqs);
    CHECK(segs[0].size() == 1 && segs[0][0] == std::make_pair((uint64_t)0, (uint64_t)41), "segments of s0");
    CHECK(segs[1].empty() && segs[3].empty(), "segments of gap");
    CHECK(segs[2].size() == 4 && segs[2][1] == std::make_pair((uint64_t)3, (uint64_t)7) && segs[2][3] == std::make_pair((uint64_t)15, (uint64_t)38), "segments of seq_two");
    std::vector<uint32_t> name_off;
    uint32_t off = 0;
    for (auto& s : seqs) { name_off.push_back(off); off += (uint32_t)s.header.size(); }
    name_off.push_back(off);
    const uint64_t seg_len = 41;
    for (int k : {2, 5, 32})
        for (uint64_t chunk : {(uint64_t)1, (uint64_t)k - 1, (uint64_t)k, seg_len - 1, seg_len, seg_len + 1, (uint64_t)1 << 20})
            for (int expanded = 0; expanded < 2; ++expanded) {
                check_cut(seqs, segs, name_off, 0, 5, chunk, k, expanded != 0);              // several sequences per call
                check_cut(seqs, segs, name_off, 0, 1, chunk, k, expanded != 0);
                check_cut(seqs, segs, name_off, 1, 2, chunk, k, expanded != 0);              // a call without a segment
                check_cut(seqs, segs, name_off, 2, 5, chunk, k, expanded != 0);
                check_cut(seqs, segs, name_off, 4, 5, chunk, k, expanded != 0);
            }
    const kq_dbgbase fw = {1, 2, 3, 1, {0, 0, 0}}, bw = {1, 2, 3, 0, {0, 0, 0}};             // fw, bw, cov, isFw
    const Triple a = oriented(fw), b = oriented(bw);
    CHECK(a.cov == 3 && a.fw == 1 && a.bw == 2 && b.cov == 3 && b.fw == 2 && b.bw == 1 && sizeof(Triple) == 12, "oriented");
}

int main() {
    test_plans();
    test_calls();
    test_cutter();
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
