// The three modes of the CLI (reference Input::read, src/input.cpp:76-181).  validate and union are ONE loop over ranges of
// the hash maps (run_ranges); subgraph has a sequence of calls of its own.  All compute goes through the C ABI
// (include/kreeq_amd.h) to the GPU; the files and the text come from db_source, per_base, variants and subgraph.
#include <sys/resource.h>
#include <unistd.h>

#include <cmath>
#include <fstream>
#include <iostream>
#include <map>

#include "db_source.h"
#include "per_base.h"
#include "subgraph.h"
#include "gfa_out.h"

namespace kqhost {

namespace {

uint64_t db_bytes(const std::string& dir, int map_count) {
    uint64_t b = file_size(dir + "/.map.hc.bin");
    for (int m = 0; m < map_count; ++m) b += file_size(dir + "/.map." + std::to_string(m) + ".bin");
    return b;
}
long peak_rss_mb() { struct rusage ru; getrusage(RUSAGE_SELF, &ru); return ru.ru_maxrss / 1024; }

// distinct k-mers a read set may hold, from its size on disk (a FASTQ record spends about half its bytes on bases,
// a gzipped one is ~4x smaller; at 30x coverage and 0.5 % errors about a fifth of the k-mer instances are distinct)
uint64_t distinct_estimate(uint64_t read_bytes) { return read_bytes / 2 + (1 << 20); }
// Map ranges to count in (the reference's computeMapRange, src/kreeq.cpp:59-63, bounds its maps by -m / 90 % of the
// RAM; here the bound is the HBM): the table (16 B per slot at load <= 0.7) plus the partition scratch and the
// pending-set arena should stay within 60 % of what is free, or of -m <GB> when that is smaller.
int passes_for(const UserInput& ui, uint64_t distinct) {
    uint64_t free_b = 0, total_b = 0;
    if (kq_device_memory(ui.device, &free_b, &total_b) != KQ_OK) return 1;
    double budget = 0.6 * (double)free_b;
    if (ui.maxMem > 0) budget = std::min(budget, ui.maxMem * 1e9);
    const double table = (double)distinct / 0.7 * 16.0;
    return (int)std::max(1.0, std::min(128.0, std::ceil(table / budget)));
}

void print_stats(const char* title, const kq_stats& st) {            // DBG::summary + DBG::DBstats, src/graph-builder.cpp:288-293
    std::cout << title << "\n"
              << "Total kmers: " << st.total << "\n"
              << "Unique kmers: " << st.unique << "\n"
              << "Distinct kmers: " << st.distinct << "\n"
              << "Missing kmers: " << st.missing << "\n"
              << "Total edges: " << st.edges << "\n";
}
void print_dbg_stats(const kq_stats& st) { print_stats("DBG Summary statistics:", st); }

DbSource open_db(Run& r, const std::string& dir) {                   // Input::loadGraph, src/input.cpp:56-74
    DbSource db(dir);
    verbose("Overriding default kmer length (" + std::to_string(r.ui.kmerLen) + ") with DB kmer length (" + std::to_string(db.idx.k) + ").");
    r.k = db.idx.k; r.map_count = db.idx.map_count;
    return db;
}
void load_sequences(Run& r) {
    if (r.ui.inSequence.empty()) return;
    verbose("Loading input sequences");
    read_fastx(r.ui.inSequence, [&](SeqRecord&& s) { r.seqs.push_back(std::move(s)); });
    r.genome = join_sequences(r.seqs, 0, r.seqs.size());
    verbose("Sequences loaded");
}

// -o vcf / -o x.vcf: DBG::correctSequences (src/variants.cpp:40-50) + gfalibs' VCF writer; "-o vcf" names no file:
// the records go to stdout (validateFiles/test.50.tst)
void write_vcf(const Run& r, const GraphSource& g) {
    const int depth = r.ui.kmerDepth == -1 ? r.k : r.ui.kmerDepth;   // include/kreeq.h:171-173 (unidirectional search)
    auto sites = find_candidate_errors(g, r.k, r.seqs, depth, r.ui.maxSpan, r.ui.covCutOff, [](const std::string& m) { verbose(m); });
    auto lines = vcf_lines(r.seqs, sites);
    if (r.ui.outFile == "vcf") { for (auto& l : lines) std::cout << l << "\n"; return; }
    std::ofstream ofs(r.ui.outFile);
    for (auto& l : lines) ofs << l << "\n";
}

// Maps [lo, hi) into the (empty) table of r.h: from the reads when there is no database -- every range of several rescans
// them, with KQ_OPT_COUNT_MAP_RANGE keeping the range's k-mers -- else from the first database's map files, with every further
// database's maps of the range loaded into a table of their own and merged region by region on the device (kq_merge =
// mergeSubMaps, src/graph-builder.cpp:341-347).
void fill_range(Run& r, const std::vector<DbSource>& dbs, uint64_t read_bytes, bool whole, int lo, int hi) {
    if (dbs.empty()) {
        if (!whole) kq_or_die(kq_set_option(r.h, KQ_OPT_COUNT_MAP_RANGE, (int64_t)lo | ((int64_t)hi << 16)));
        verbose("Loading input reads.");
        for (auto& f : r.ui.inReads) count_reads_file(r.h, f, parser_threads(r.ui, read_bytes), read_bytes, r.ui.device);
        verbose("Reads loaded.");
        return;
    }
    const uint64_t n_in = dbs[0].import_into(r.h, lo, hi);
    verbose("Database loaded (" + std::to_string(n_in) + " k-mers; peak host memory " + std::to_string(peak_rss_mb()) + " MB)");
    for (size_t n = 1; n < dbs.size(); ++n) {
        kq_handle* src = nullptr;
        kq_or_die(kq_create(&src, r.ui.device, r.k, r.map_count, dbs[n].entries_bound(lo, hi) + 1024));
        dbs[n].import_into(src, lo, hi);
        kq_or_die(kq_set_option(r.h, KQ_OPT_MERGE_PATH, 2));
        kq_or_die(kq_merge(r.h, src));
        kq_destroy(src);
    }
}

// The map-range loop of validate and union: the GPU counterpart of the reference's computeMapRange / loadMapRange
// (src/kreeq.cpp:59-74) and of its spill-to-disk behaviour under -m.  Only 1/n of the table is resident at a time.  Per range:
// clear (after the first), fill, summary, lookup of the sequences over the range's maps, histogram, export of the range's map
// files -- each only where the output plan asks for it.  Summary numbers, histogram and QV counters add up over the disjoint
// ranges, the per-base vector is filled range by range (a position is evaluated in exactly one), a .kreeq output is written
// range by range.  Every output is then emitted once.  With n = 1 the table stays resident afterwards, and only then the
// outputs that need the whole graph at once read it: the variant search of -o vcf (graph_of_handle) and the device writer of
// the per-base tables.  With n > 1 the per-base tables may accumulate on the device range by range instead of in the host vector
// (TablePasses, opt-in), and the variant search runs over the database on disk (the input one, or a temporary one
// written during the loop -- the reference dumps its maps to disk and reloads ranges likewise).
void run_ranges(Run& r, const std::vector<DbSource>& dbs, uint64_t read_bytes, int n) {
    const UserInput& ui = r.ui;
    const OutPlan& plan = r.plan;
    const bool validate = ui.mode == 0, search = validate && plan.vcf && !ui.inSequence.empty();
    const bool device_tables = validate && plan.tables() && n == 1 && table_device_wanted(r);
    TablePasses acc;                                                 // (taken before the first fill: the count path sizes its arena around it)
    const bool acc_tables = validate && plan.tables() && n > 1 && table_passes_wanted(r) && table_passes_begin(r, acc);
    const bool lookup = validate && !ui.inSequence.empty() && !plan.vcf && !device_tables && !acc_tables;      // every other extension validates (src/kreeq-output.cpp:62-72)
    if (lookup && plan.tables()) r.per_base.assign(r.genome.text.size(), kq_dbgbase{});
    // where the ranges go when a later step needs them again: the .kreeq output, or a temporary database for the variant search
    std::string range_db;
    if (plan.kreeq) range_db = ui.outFile;
    else if (search && dbs.empty() && n > 1) range_db = ui.prefix + "/.kreeq_ranges_" + std::to_string((long)getpid()) + ".kreeq";
    kq_stats sum{};
    std::map<uint64_t, uint64_t> hist;                               // gfalibs printHist (format not pinned by any fixture)
    std::vector<kq_entry> hc_all;
    for (int p = 0; p < n; ++p) {
        const auto [lo, hi] = pass_range(p, n, r.map_count);
        verbose("Pass " + std::to_string(p + 1) + "/" + std::to_string(n) + ": maps [" + std::to_string(lo) + "," + std::to_string(hi) + ")");
        if (p) kq_or_die(kq_clear(r.h));
        fill_range(r, dbs, read_bytes, n == 1, lo, hi);
        if (plan.want_stats) {
            kq_stats st;
            kq_or_die(kq_summary(r.h, &st));
            sum.total += st.total; sum.unique += st.unique; sum.distinct += st.distinct; sum.edges += st.edges;
            verbose("Summary computed");
        }
        if (lookup) {
            verbose("Validating sequence");
            kq_or_die(kq_lookup_sequence(r.h, r.genome.text.data(), r.genome.text.size(), ui.covCutOff, (uint16_t)lo, (uint16_t)hi,
                                         plan.tables() ? r.per_base.data() : nullptr, r.counters));
        }
        if (acc_tables) {
            verbose("Validating sequence");
            table_passes_range(r, acc, lo, hi);
        }
        if (plan.hist) {
            uint64_t m = 0;
            kq_or_die(kq_histogram(r.h, nullptr, nullptr, 0, &m));
            std::vector<uint64_t> cov((size_t)m), cnt((size_t)m);
            if (m) kq_or_die(kq_histogram(r.h, cov.data(), cnt.data(), m, &m));
            for (uint64_t i = 0; i < m; ++i) hist[cov[i]] += cnt[i];
        }
        if (!range_db.empty()) export_db_maps(r.h, ui.device, range_db, r.map_count, lo, hi, hc_all);
    }
    if (plan.want_stats) {
        sum.missing = (r.k < 32 ? (1ull << (2 * r.k)) : 0ull) - sum.distinct;          // src/graph-builder.cpp:286, as kq_summary has it for one range
        print_dbg_stats(sum);
    }
    verbose("Writing ouput: " + ui.outFile);
    if (!range_db.empty()) { write_db_finish(range_db, r.k, r.map_count, hc_all); if (plan.kreeq) verbose("Database written"); }
    if (device_tables) write_per_base_device(r);
    if (acc_tables) { table_passes_write(r, acc); print_qv(r); }
    if (lookup) print_qv(r);
    if (validate && plan.tables() && !device_tables && !acc_tables) write_per_base_host(r);
    if (plan.hist) { std::ofstream ofs(ui.outFile); for (auto& kv : hist) ofs << kv.first << "\t" << kv.second << "\n"; }
    if (search) {
        if (n == 1) write_vcf(r, graph_of_handle(r.h));
        else if (!dbs.empty()) write_vcf(r, graph_of_db_ranges(r.h, dbs[0], n));
        else {
            { DbSource tmp(range_db); write_vcf(r, graph_of_db_ranges(r.h, tmp, n)); }
            for (int m = 0; m < r.map_count; ++m) ::unlink((range_db + "/.map." + std::to_string(m) + ".bin").c_str());
            ::unlink((range_db + "/.map.hc.bin").c_str()); ::unlink((range_db + "/.index").c_str()); ::rmdir(range_db.c_str());
        }
    }
    verbose("Peak host memory: " + std::to_string(peak_rss_mb()) + " MB");
}

// a table for the largest of the n ranges of the databases
void create_for_ranges(Run& r, const std::vector<DbSource>& dbs, int n) {
    uint64_t cap = 0;
    for (int p = 0; p < n; ++p) {
        const auto range = pass_range(p, n, r.map_count);
        uint64_t c = 0;
        for (auto& d : dbs) c += d.entries_bound(range.first, range.second);
        cap = std::max(cap, c);
    }
    kq_or_die(kq_create(&r.h, r.ui.device, r.k, r.map_count, cap + 1024));
}

void run_validate(Run& r) {                                          // src/input.cpp:86-118
    UserInput& ui = r.ui;
    std::vector<DbSource> dbs;
    uint64_t bytes = 0;
    if (!ui.inReads.empty()) {
        for (auto& f : ui.inReads) bytes += file_size(f) * (file_ext(f).find("gz") != std::string::npos ? 4 : 1);
        if (ui.passes == 0) {                                        // automatic: as many map ranges as the HBM asks for
            ui.passes = passes_for(ui, distinct_estimate(bytes));
            if (ui.passes > 1) verbose("Table of ~" + std::to_string(distinct_estimate(bytes)) + " k-mers does not fit the free HBM: counting in " + std::to_string(ui.passes) + " map ranges");
        }
        r.k = ui.kmerLen;
    } else {
        if (ui.kmerDB.size() > 1) die("More than one DBG database provided. Merge them first. Exiting.");
        if (ui.kmerDB.empty()) die("Cannot load DBG input. Exiting.");
        // the database is read map range by map range (DbSource): a few maps' entries on the host at a time; when its table
        // does not fit the HBM (or -m), it is also EVALUATED range by range (src/kreeq.cpp:59-74)
        dbs.push_back(open_db(r, ui.kmerDB[0]));
        if (ui.passes == 0) {
            const uint64_t bound = dbs[0].entries_bound(0, r.map_count);
            ui.passes = passes_for(ui, bound);
            if (ui.passes > 1) verbose("Table of <= " + std::to_string(bound) + " k-mers does not fit the free HBM: validating in " + std::to_string(ui.passes) + " map ranges");
        }
    }
    const int n = ui.passes = std::min(ui.passes, r.map_count);
    if (!dbs.empty()) create_for_ranges(r, dbs, n);              // (one range of reads gets the table single-pass counting has always had)
    else kq_or_die(kq_create(&r.h, ui.device, r.k, r.map_count, n == 1 ? distinct_estimate(bytes) : distinct_estimate(bytes) / (uint64_t)n + (1 << 20)));
    load_sequences(r);
    run_ranges(r, dbs, bytes, n);
}

void run_union(Run& r) {                                             // src/input.cpp:119-152
    const UserInput& ui = r.ui;
    verbose("Merging input databases.");
    int k = 0, map_count = 128;
    for (auto& db : ui.kmerDB) {
        DbIndex idx = read_index(db);
        if (k == 0) { k = idx.k; map_count = idx.map_count; }
        if (k != idx.k) { fprintf(stderr, "Cannot merge databases with different kmer length.\n"); exit(1); }
    }
    if (k == 0 || k > 32) { fprintf(stderr, "Invalid kmer length.\n"); exit(1); }
    r.k = k; r.map_count = map_count;
    // DBG::kunion (src/graph-builder.cpp:297-351): largest database first (:341-344); the databases are merged MAP RANGE BY
    // MAP RANGE (mergeMaps map by map, :341-347), and a range is summarised / written before the next one is loaded.
    // One range when everything fits the HBM (and -m); the host holds a few maps' entries at a time either way.
    std::vector<std::pair<uint64_t, size_t>> order;
    for (size_t i = 0; i < ui.kmerDB.size(); ++i) order.emplace_back(db_bytes(ui.kmerDB[i], map_count), i);
    std::sort(order.rbegin(), order.rend());
    std::vector<DbSource> dbs;
    for (auto& o : order) dbs.emplace_back(ui.kmerDB[o.second]);
    uint64_t total = 0;
    for (auto& d : dbs) total += d.entries_bound(0, map_count);       // 24-byte slots at load <= 7/8: an upper bound of the entries
    const int passes = ui.passes ? std::min(ui.passes, map_count) : std::min(passes_for(ui, total + total / 2), map_count);   // (+ the source table of a merge)
    if (passes > 1) verbose("Merging in " + std::to_string(passes) + " map ranges");
    create_for_ranges(r, dbs, passes);
    verbose("DBG object generated. Merging.");
    run_ranges(r, dbs, 0, passes);
}

void run_subgraph(Run& r) {                                          // src/input.cpp:153-181
    const UserInput& ui = r.ui;
    // loadGraph: the whole database in one resident table (the reference's traversal changes its frontier between map
    // ranges, which is not restated: DESIGN.md section 12)
    const std::vector<DbSource> dbs = {open_db(r, ui.kmerDB[0])};
    const uint64_t bound = dbs[0].entries_bound(0, r.map_count);
    if (passes_for(ui, bound) > 1)
        die("Error: the database (<= " + std::to_string(bound) + " k-mers) does not fit the device memory in one table; subgraph does not run in map ranges");
    create_for_ranges(r, dbs, 1);
    const uint64_t n_in = dbs[0].import_into(r.h, 0, r.map_count);
    verbose("Database loaded (" + std::to_string(n_in) + " k-mers)");
    load_sequences(r);
    const bool trace = env_flag("KQ_SUBGRAPH_TRACE");
    auto step = [trace, t0 = now_s()](const char* what) mutable {    // KQ_SUBGRAPH_TRACE=1: wall clock of the steps to stderr
        const double t1 = now_s();
        if (trace) fprintf(stderr, "[subgraph] %s: %.3f s\n", what, t1 - t0);
        t0 = t1;
    };
    kq_handle* sub = nullptr;
    kq_or_die(kq_create(&sub, ui.device, r.k, r.map_count, r.genome.text.size() + 1024));
    verbose("Subsetting graph");                                     // DBG::subgraph, src/subgraph.cpp:116-161
    kq_or_die(kq_subgraph_seed(r.h, sub, r.genome.text.data(), r.genome.text.size(), ui.noReference ? KQ_SUBGRAPH_NO_REFERENCE : 0));
    step("seed");
    verbose("Searching graph");                                      // DBG::searchGraph, :290-299; default depths: include/kreeq.h:171-175
    const bool best_first = ui.travAlgorithm == "best-first";
    const int depth = ui.kmerDepth != -1 ? ui.kmerDepth : best_first ? r.k : (r.k + 1) / 2;
    uint64_t n_added = 0;
    // KQ_SUBGRAPH_DEVICE=1 (off by default): the best-first searches run on the GPU, one per lane (kq_subgraph_best_first), instead of on the
    // host in lockstep rounds of lookups; a depth above 255 keeps the host search (the device state block is sized for a uint8_t depth)
    const bool bf_device = best_first && env_flag("KQ_SUBGRAPH_DEVICE") && depth >= 0 && depth <= 255;
    if (bf_device) {
        kq_or_die(kq_subgraph_best_first(r.h, sub, depth, ui.covCutOff, &n_added));
        verbose("Best-first: device search, " + std::to_string(n_added) + " k-mers added");
    } else if (best_first) n_added = subgraph_best_first(r.h, sub, r.k, r.map_count, depth, ui.covCutOff, [](const std::string& m) { verbose("Best-first: host search"); verbose(m); });      // (the log is called once, at the end)
    else kq_or_die(kq_subgraph_expand(r.h, sub, depth, &n_added));
    step("expand");
    if (best_first && trace) fprintf(stderr, "[subgraph] best-first ran as the %s search\n", bf_device ? "device" : "host");
    verbose(std::to_string(n_added) + " k-mers added by the search");
    verbose("Remove missing edges");                                 // DBG::removeMissingEdges, :599-628
    kq_or_die(kq_subgraph_trim(sub, ui.covCutOff));
    step("trim");
    kq_stats st;
    kq_or_die(kq_summary(sub, &st));
    print_stats("Subgraph summary statistics:", st);                 // DBG::summary(ParallelMap32color&), :163-188
    // KQ_SUBGRAPH_GFA=1 (off by default): the graph of DBG::DBGgraphToGFA (src/kreeq.cpp:523-600) is built on the GPU
    // (kq_subgraph_gfa); its "+++Assembly summary+++" block goes between the two summaries and -o <name>.gfa is written.
    // Without it nothing is printed here (gfalibs' report of its GFA model).
    if (env_flag("KQ_SUBGRAPH_GFA")) {
        const uint32_t flags = ui.noCollapse ? KQ_GFA_NO_COLLAPSE : 0;
        kq_gfa_counts cnt{};
        GfaGraph g;
        g.k = r.k;
        kq_or_die(kq_subgraph_gfa(sub, flags, nullptr, 0, nullptr, 0, nullptr, 0, &cnt));
        g.segs.resize(cnt.n_segments); g.seq.resize(cnt.n_seq); g.edges.resize(cnt.n_edges);
        // (the vectors' data() may be null when empty: one element of room keeps "the arrays are wanted" apart from "counts only")
        kq_gfa_segment seg0{}; kq_gfa_edge edge0{}; char seq0 = 0;
        kq_or_die(kq_subgraph_gfa(sub, flags, g.segs.empty() ? &seg0 : g.segs.data(), cnt.n_segments, g.seq.empty() ? &seq0 : &g.seq[0], cnt.n_seq,
                                  g.edges.empty() ? &edge0 : g.edges.data(), cnt.n_edges, &cnt));
        step("gfa");
        verbose("subgraph GFA built on the device: " + std::to_string(cnt.n_segments) + " segments, " + std::to_string(cnt.n_edges) + " links, " +
                std::to_string(cnt.n_dropped_edges) + " links dropped, " + std::to_string(cnt.n_cycles) + " cycles");
        if (!gfa_valid(g)) die("Error: the device returned a graph whose records leave their arrays");
        std::string text;
        gfa_block(gfa_stats(g), text);
        fwrite(text.data(), 1, text.size(), stdout);
        if (!ui.outFile.empty()) {
            text.clear();
            gfa_text(g, text);
            FILE* f = fopen(ui.outFile.c_str(), "wb");
            if (!f || fwrite(text.data(), 1, text.size(), f) != text.size() || fclose(f) != 0) die("Error: cannot write " + ui.outFile);
            verbose("Graph written to " + ui.outFile);
        }
    }
    kq_destroy(sub);
    kq_or_die(kq_summary(r.h, &st));                                 // DBG::report with no -o, src/kreeq-output.cpp:34-60
    print_dbg_stats(st);
}

}  // namespace

int run(UserInput& ui) {
    Run r;
    r.ui = ui;
    if (ui.outFile.find(".kreeq") != std::string::npos) r.ui.prefix = ui.outFile;        // src/input.cpp:78-79
    r.plan = plan_output(ui.mode, ui.outFile);
    if (r.plan.refused) die("Error: ." + r.plan.ext + " output (variant graph) is not supported by this build: use -o vcf");
    switch (ui.mode) {
        case 0: run_validate(r); break;
        case 1: run_union(r); break;
        case 2: run_subgraph(r); break;
        default:
            fprintf(stderr, "Invalid mode.\n");
            exit(1);
    }
    kq_destroy(r.h);
    return EXIT_SUCCESS;
}

}  // namespace kqhost
