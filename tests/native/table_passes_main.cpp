// The plan of the per-base table under map-range passes (plan_table_passes, kreeq_amd/host/cli_plan.h) as a stand-alone host
// program: the groups, their text ranges, their rebased segment lists, the running first_triple and the three sizes, checked
// against what the sequences themselves say, at call limits of 8, 100, 200 and 2^30 bytes.
#include <cstdio>
#include <string>
#include <vector>

#include "cli_plan.h"

using namespace kqhost;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static SeqRecord seq_of(const std::string& name, const std::string& text) { SeqRecord r; r.header = name; r.seq = text; return r; }
static std::string bases(size_t n) { std::string s(n, 'A'); for (size_t i = 0; i < n; ++i) s[i] = "ACGTacgt"[i % 8]; return s; }
// n bytes with N runs: one at the start, one in the middle, a lone N near the end (where there is room)
static std::string gapped(size_t n) {
    std::string s = bases(n);
    if (n > 0) s[0] = 'N';
    for (size_t i = n / 2; i < n / 2 + 3 && i < n; ++i) s[i] = 'N';
    if (n > 4) s[n - 2] = 'n';
    return s;
}

static TablePassPlan check_plan(const std::vector<SeqRecord>& seqs, uint64_t limit, const char* what) {
    const SegmentLists segs = all_segments(seqs);
    const TablePassPlan p = plan_table_passes(seqs, segs, limit);
    bool fits = true;
    for (auto& s : seqs) fits = fits && s.seq.size() + 1 <= limit;
    CHECK(p.fits == fits, "%s limit %llu: fits %d", what, (unsigned long long)limit, p.fits);
    size_t next_seq = 0;
    uint64_t text_off = 0, first = 0, max_text = 0;
    for (size_t gi = 0; gi < p.groups.size(); ++gi) {
        const TableGroup& g = p.groups[gi];
        CHECK(g.lo == next_seq && g.hi > g.lo && g.hi <= seqs.size(), "%s limit %llu: group %zu is [%zu, %zu)", what, (unsigned long long)limit, gi, g.lo, g.hi);
        if (g.lo != next_seq || g.hi <= g.lo || g.hi > seqs.size()) return p;
        CHECK(g.hi == next_call(seqs, g.lo, limit), "%s: group %zu is not next_call's", what, gi);
        CHECK(g.text_off == text_off && g.first_triple == first, "%s limit %llu: group %zu text_off %llu first_triple %llu", what, (unsigned long long)limit, gi,
              (unsigned long long)g.text_off, (unsigned long long)g.first_triple);
        CHECK(g.seg_start.size() == g.seg_len.size(), "%s: list lengths", what);
        uint64_t len = 0, n = 0, prev_end = 0;
        size_t j = 0;                                        // the segment of the group expected next
        for (size_t s = g.lo; s < g.hi; ++s) {
            for (auto& seg : segs[s]) {                      // every segment in exactly one group, in order
                CHECK(j < g.seg_start.size(), "%s: group %zu misses a segment of sequence %zu", what, gi, s);
                if (j >= g.seg_start.size()) return p;
                CHECK(g.seg_start[j] == len + seg.first && g.seg_len[j] == seg.second, "%s limit %llu: group %zu segment %zu is %llu + %llu", what, (unsigned long long)limit, gi, j,
                      (unsigned long long)g.seg_start[j], (unsigned long long)g.seg_len[j]);
                CHECK(g.seg_start[j] >= prev_end && g.seg_len[j] > 0, "%s: group %zu segment %zu is not behind the one before it", what, gi, j);
                prev_end = g.seg_start[j] + g.seg_len[j];
                // rebased: inside the sequence's own part of the group text, bases from end to end, no base around it
                CHECK(seg.first + seg.second <= seqs[s].seq.size(), "%s: segment beyond its sequence", what);
                CHECK(is_base(seqs[s].seq[seg.first]) && is_base(seqs[s].seq[seg.first + seg.second - 1]), "%s: segment ends", what);
                CHECK(seg.first == 0 || !is_base(seqs[s].seq[seg.first - 1]), "%s: a base before the segment", what);
                CHECK(seg.first + seg.second == seqs[s].seq.size() || !is_base(seqs[s].seq[seg.first + seg.second]), "%s: a base behind the segment", what);
                n += seg.second; ++j;
            }
            len += seqs[s].seq.size() + 1;
        }
        CHECK(j == g.seg_start.size(), "%s: group %zu holds %zu segments, %zu expected", what, gi, g.seg_start.size(), j);
        CHECK(g.text_len == len && g.n_triples == n, "%s limit %llu: group %zu text_len %llu n_triples %llu", what, (unsigned long long)limit, gi, (unsigned long long)g.text_len,
              (unsigned long long)g.n_triples);
        CHECK(prev_end <= g.text_len, "%s: group %zu: a segment ends at %llu of %llu bytes", what, gi, (unsigned long long)prev_end, (unsigned long long)g.text_len);
        CHECK(g.text_len <= limit || g.hi == g.lo + 1, "%s limit %llu: group %zu holds %llu bytes", what, (unsigned long long)limit, gi, (unsigned long long)g.text_len);
        if (g.hi < seqs.size()) CHECK(g.text_len + seqs[g.hi].seq.size() + 1 > limit, "%s: sequence %zu would have fitted", what, g.hi);
        text_off += len; first += n; next_seq = g.hi;
        max_text = std::max(max_text, len);
    }
    CHECK(next_seq == seqs.size(), "%s limit %llu: the groups end at sequence %zu of %zu", what, (unsigned long long)limit, next_seq, seqs.size());
    uint64_t positions = 0;
    for (auto& l : segs) for (auto& seg : l) positions += seg.second;
    CHECK(first == positions && p.acc_bytes == 12 * positions, "%s limit %llu: acc_bytes %llu for %llu positions", what, (unsigned long long)limit, (unsigned long long)p.acc_bytes,
          (unsigned long long)positions);
    CHECK(p.max_text == max_text && p.max_per_base == 16 * max_text, "%s limit %llu: max_text %llu max_per_base %llu", what, (unsigned long long)limit, (unsigned long long)p.max_text,
          (unsigned long long)p.max_per_base);
    CHECK(p.device_bytes() == 12 * positions + 17 * max_text, "%s: device_bytes", what);
    if (fits) CHECK(p.max_text <= limit, "%s limit %llu: max_text %llu although every sequence fits", what, (unsigned long long)limit, (unsigned long long)p.max_text);
    return p;
}

static void test_small_limits() {
    for (uint64_t limit : {(uint64_t)8, (uint64_t)100, (uint64_t)200}) {
        const size_t l = (size_t)limit;
        check_plan({}, limit, "no sequence");
        check_plan({seq_of("e", "")}, limit, "one empty sequence");
        check_plan({seq_of("a", bases(1))}, limit, "one base");
        check_plan({seq_of("a", bases(l - 2))}, limit, "limit - 1 bytes with the separator");
        check_plan({seq_of("a", bases(l - 1))}, limit, "limit bytes with the separator");
        check_plan({seq_of("a", bases(l))}, limit, "limit bases: does not fit");
        check_plan({seq_of("n", std::string(5, 'N'))}, limit, "a sequence without bases");
        check_plan({seq_of("g", gapped(l - 1))}, limit, "N runs");
        // all of them at once, twice over, so that groups begin and end at every kind of sequence
        std::vector<SeqRecord> all;
        for (int rep = 0; rep < 2; ++rep) {
            all.push_back(seq_of("e", ""));
            all.push_back(seq_of("one", bases(1)));
            all.push_back(seq_of("lm2", bases(l - 2)));
            all.push_back(seq_of("n", std::string(3, 'n')));
            all.push_back(seq_of("lm1", gapped(l - 1)));
            all.push_back(seq_of("half", gapped(l / 2)));
            all.push_back(seq_of("half2", bases(l / 2 - 1)));
            all.push_back(seq_of("one2", bases(1)));
        }
        check_plan(all, limit, "mixed, all fit");
        all.insert(all.begin() + 3, seq_of("big", gapped(l)));
        all.push_back(seq_of("big2", bases(l + 7)));
        check_plan(all, limit, "mixed, two above the limit");
    }
    // known answers: four sequences of 99 bases (100 bytes each), the second and fourth with a gap of 3
    std::vector<SeqRecord> four = {seq_of("a", bases(99)), seq_of("b", bases(99)), seq_of("c", bases(99)), seq_of("d", bases(99))};
    four[1].seq.replace(40, 3, "NNN"); four[3].seq.replace(0, 3, "NNN");
    const SegmentLists segs = all_segments(four);
    const TablePassPlan p200 = plan_table_passes(four, segs, 200), p100 = plan_table_passes(four, segs, 100), p99 = plan_table_passes(four, segs, 99);
    CHECK(p200.fits && p200.groups.size() == 2 && p200.max_text == 200 && p200.max_per_base == 3200 && p200.acc_bytes == 12 * (99 + 96 + 99 + 96), "four at 200");
    CHECK(p200.groups.size() == 2 && p200.groups[1].text_off == 200 && p200.groups[1].first_triple == 195 && p200.groups[1].seg_start == std::vector<uint64_t>({0, 103}) &&
          p200.groups[0].seg_start == std::vector<uint64_t>({0, 100, 143}) && p200.groups[0].seg_len == std::vector<uint64_t>({99, 40, 56}), "four at 200: lists");
    CHECK(p100.fits && p100.groups.size() == 4 && p100.max_text == 100 && p100.groups[3].first_triple == 294 && p100.groups[3].seg_start == std::vector<uint64_t>({3}), "four at 100");
    CHECK(!p99.fits && p99.groups.size() == 4, "four at 99");
}

// limit 2^30: the sequences of 0, 1, limit - 1 and limit bytes, one large one at a time (its plan is one group either way)
static void test_large_limit() {
    const uint64_t limit = (uint64_t)1 << 30;
    check_plan({seq_of("e", ""), seq_of("a", bases(1)), seq_of("n", "NNNN"), seq_of("g", gapped(1000))}, limit, "small sequences at 2^30");
    {
        std::vector<SeqRecord> seqs(3);
        seqs[0] = seq_of("a", bases(5));
        seqs[1].header = "big"; seqs[1].seq.reserve((size_t)limit); seqs[1].seq.assign((size_t)limit - 2, 'C'); seqs[1].seq[12345] = 'N';      // limit - 1 bytes with its separator
        seqs[2] = seq_of("z", gapped(50));
        const TablePassPlan p = check_plan(seqs, limit, "limit - 1 bytes at 2^30");
        CHECK(p.fits && p.groups.size() == 3 && p.max_text == limit - 1 && p.groups[2].text_off == 6 + limit - 1 && p.groups[2].first_triple == 5 + limit - 3, "limit - 1 bytes at 2^30: groups");
        seqs[1].seq.push_back('G');                                                                        // limit bytes: fits exactly
        check_plan(seqs, limit, "limit bytes at 2^30");
        seqs[1].seq.push_back('T');                                                                        // limit bases: not with its separator
        CHECK(!check_plan(seqs, limit, "limit bases at 2^30").fits, "limit bases at 2^30 fit");
    }
}

int main() {
    test_small_limits();
    test_large_limit();
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
