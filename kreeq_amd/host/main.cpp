// kreeq (MI355X build) -- host CLI with the reference's `validate` / `union` / `subgraph` interface.
// Flag names, stdout blocks, exit codes and the .kreeq directory follow vgl-hub/kreeq @ 2024_08_07
// (src/main.cpp:78-97, :220-229; src/input.cpp:76-152; src/kreeq-output.cpp:34-136;
// src/graph-builder.cpp:288-293; src/kreeq.cpp:78-106).  All compute goes through the C ABI
// (include/kreeq_amd.h) to the GPU; this file is the command line: the three option tables, the help texts and the host-only
// `dbtool` helpers of the tests.  run.cpp holds the modes.
#include <getopt.h>

#include <cstring>
#include <mutex>
#include <stdexcept>

#include "cli_common.h"
#include "cli_plan.h"
#include "fastx.h"
#include "kreeq_db.h"

using namespace kqhost;

namespace {

const char* kVersion = "0.1.0-mi355x";
int cmd_flag = 0;

bool is_number(const char* s) { if (!*s) return false; for (; *s; ++s) if (*s < '0' || *s > '9') return false; return true; }
bool is_int(const char* s) { if (*s == '-' || *s == '+') ++s; return is_number(s); }
void if_file_exists(const char* p) {
    struct stat st;
    if (stat(p, &st) != 0) { printf("File does not exist (%s). Terminating.\n", p); exit(EXIT_FAILURE); }
}
// the file names behind -r / -d: every argument up to the next option or number (src/main.cpp:169-180)
void take_files(int argc, char** argv, std::vector<std::string>& out) {
    optind--;
    for (; optind < argc && *argv[optind] != '-' && !is_int(argv[optind]); optind++) {
        if_file_exists(argv[optind]);
        out.push_back(argv[optind]);
    }
}
int number_arg() {
    if (!is_number(optarg)) { fprintf(stderr, "input '%s' to option -%c must be a number\n", optarg, optopt); exit(EXIT_FAILURE); }
    return atoi(optarg);
}
// dbtool: count, bases and order-independent digest (sum of FNV-1a) of the '\n'-separated sequences of a batch
void digest_lines(const char* b, size_t len, unsigned long long& n, unsigned long long& bases, unsigned long long& digest) {
    for (size_t i = 0; i <= len;) {
        const char* nl = (const char*)memchr(b + i, '\n', len - i);
        const size_t j = nl ? (size_t)(nl - b) : len;
        unsigned long long hsh = 1469598103934665603ull;
        for (size_t c = i; c < j; ++c) { hsh ^= (unsigned char)b[c]; hsh *= 1099511628211ull; }
        ++n; bases += j - i; digest += hsh;
        i = j + 1;
    }
}
void print_help() { printf("kreeq [mode] -h\nfor additional help.\n\nModes:\nvalidate\nunion\nsubgraph\n"); exit(0); }
void print_mode_help(int mode) {
    if (mode == 0) {
        printf("kreeq [command]\n\nOptions:\n");
        printf("\t-c --coverage-cutoff coverage cutoff.\n");
        printf("\t-d --database kreeq database to load.\n");
        printf("\t-f --input-sequence sequence input file (fasta,fastq).\n");
        printf("\t-r --input-reads read input files (fastq).\n");
        printf("\t-k --kmer-length length of kmers.\n");
        printf("\t-o --out-format supported extensions:\n");
        printf("\t\t .kreeq dumps hashmaps to file for reuse; .kwig .bkwig per-base tables; .hist coverage histogram.\n");
        printf("\t\t .kwig.gz .bed.gz .csvtable.gz the text tables as BGZF (bgzip-compatible).\n");
        printf("\t-t --tmp-prefix prefix to temporary directory (unused: the table lives in HBM).\n");
        printf("\t-m --max-memory <GB> HBM the k-mer table may use (default: 60 %% of what is free); bounds the map ranges counted at a time.\n");
        printf("\t-j --threads <n> parser threads for the read files (default: all cores).\n");
        printf("\t--device <n> GPU to use (default 0).\n");
        printf("\t--passes <n> count the reads n times, one range of the hash maps per pass (HBM use = 1/n of the table); default: as many as -m asks for.\n");
        printf("\t-v --version software version.\n");
        printf("\t--cmd print $0 to stdout.\n");
    } else if (mode == 2) {
        printf("kreeq subgraph [options]\n\nOptions:\n");
        printf("\t-c --coverage-cutoff exclude nodes and edges below or equal to the cutoff (default: 0).\n");
        printf("\t-d --database DBG database.\n");
        printf("\t-f --input-sequence sequence input file (fasta).\n");
        printf("\t--traversal-algorithm <string> the approach used for graph search (best-first/traversal, default: best-first).\n");
        printf("\t--search-depth the max depth for graph traversal (default: k for best-first, ceil(k / 2) for traversal; traversal: at most 255).\n");
        printf("\t--no-collapse do not collapse linear nodes (takes effect with KQ_SUBGRAPH_GFA=1, which builds the graph; no effect otherwise).\n");
        printf("\t--no-reference do not include reference nodes (default: false).\n");
        printf("\t-o --out-format with KQ_SUBGRAPH_GFA=1: <name>.gfa, the subgraph as GFA 1 (no .gfa.gz / .gfa2); refused otherwise.\n");
        printf("\t-p --input-positions not supported by this build: refused.\n");
        printf("\t-j --threads <n> accepted for compatibility.\n");
        printf("\t-m --max-memory <GB> HBM the database table may use (default: 60 %% of what is free).\n");
        printf("\t--device <n> GPU to use (default 0).\n");
        printf("\t--cmd print $0 to stdout.\n");
    } else {
        printf("kreeq union [options]\n\nOptions:\n");
        printf("\t-d --databases DBG databases to merge.\n");
        printf("\t-j --threads <n> accepted for compatibility.\n");
        printf("\t-o --out-format generates various kinds of outputs (currently supported: .kreeq).\n");
        printf("\t-m --max-memory <GB> HBM the merge may use (default: 60 %% of what is free); bounds the map ranges merged at a time.\n");
        printf("\t--passes <n> merge the databases in n ranges of the hash maps.\n");
        printf("\t--cmd print $0 to stdout.\n");
    }
    exit(0);
}

}  // namespace

int main(int argc, char** argv) {
    UserInput ui;
    if (argc == 1 || argc == 2) print_help();
    std::string mode = argv[1];
    if (mode == "dbtool") {           // host-only helper (no GPU): `dbtool dump <db>` | `dbtool rewrite <in> <out>`
        try {
            std::vector<kq_entry> entries;
            DbIndex idx;
            if (argc == 4 && std::string(argv[2]) == "dump") {
                read_db(argv[3], entries, &idx);
                printf("#k=%d map_count=%d columns: map key fw0 fw1 fw2 fw3 bw0 bw1 bw2 bw3 cov hc\n", idx.k, idx.map_count);
                std::sort(entries.begin(), entries.end(), [](const kq_entry& a, const kq_entry& b) { return a.key < b.key; });
                for (auto& e : entries)
                    printf("%llu %llu %u %u %u %u %u %u %u %u %u %u\n", (unsigned long long)(e.key % (uint64_t)idx.map_count),
                           (unsigned long long)e.key, e.fw[0], e.fw[1], e.fw[2], e.fw[3], e.bw[0], e.bw[1], e.bw[2], e.bw[3], e.cov, e.hc);
                return EXIT_SUCCESS;
            }
            if (argc == 5 && std::string(argv[2]) == "rewrite") {
                read_db(argv[3], entries, &idx);
                write_db(argv[4], idx.k, idx.map_count, entries);
                return EXIT_SUCCESS;
            }
            if (argc >= 4 && std::string(argv[2]) == "seqsum") {       // order-independent digest of the sequences a reader yields
                const unsigned threads = argc > 4 ? (unsigned)atoi(argv[4]) : 0;
                const size_t batch = argc > 5 ? (size_t)atoll(argv[5]) : ((size_t)1 << 20);
                unsigned long long n = 0, bases = 0, digest = 0, batches = 0;
                const char* fail_after = getenv("KQ_TEST_FAIL_AFTER_BATCHES");     // failure-path test: the consumer throws mid-file
                auto eat = [&](const std::string& b) {
                    if (fail_after && ++batches > (unsigned long long)atoll(fail_after)) throw std::runtime_error("consumer failed (injected)");
                    digest_lines(b.data(), b.size(), n, bases, digest);
                };
                if (threads == 0) read_batches(argv[3], batch, eat); else read_batches_parallel(argv[3], batch, threads, eat);
                printf("%llu %llu %llu\n", n, bases, digest);
                return EXIT_SUCCESS;
            }
            if (argc >= 6 && std::string(argv[2]) == "seqsink") {      // the same digest through the zero-copy sink reader (plain heap buffers)
                const unsigned threads = (unsigned)atoi(argv[4]);
                const size_t cap = (size_t)atoll(argv[5]);
                unsigned long long n = 0, bases = 0, digest = 0;
                std::mutex m;
                std::vector<std::vector<char>> bufs(std::max(1u, threads));
                BatchSink sink;
                sink.acquire = [&](unsigned t, size_t* c) { bufs[t].resize(cap); *c = cap; return bufs[t].data(); };
                if (!getenv("KQ_TEST_NO_BIG")) {      // (a sink without one-off buffers refuses over-long sequences)
                    sink.acquire_big = [&](unsigned, size_t nb) { return (char*)malloc(nb); };
                    sink.submit_big = [&](unsigned t, char* b, size_t len) { sink.submit(t, b, len); free(b); };
                }
                sink.submit = [&](unsigned, char* b, size_t len) {
                    if (!len) return;
                    unsigned long long ln = 0, lb = 0, ld = 0;
                    digest_lines(b, len, ln, lb, ld);
                    std::lock_guard<std::mutex> l(m);
                    n += ln; bases += lb; digest += ld;
                };
                read_batches_sink(argv[3], threads, sink);
                printf("%llu %llu %llu\n", n, bases, digest);
                return EXIT_SUCCESS;
            }
        } catch (const std::exception& ex) { fprintf(stderr, "%s\n", ex.what()); return EXIT_FAILURE; }
        fprintf(stderr, "usage: kreeq dbtool dump <db.kreeq> | rewrite <in.kreeq> <out.kreeq> | seqsum <fastx> [threads] [batch_bytes]\n");
        return EXIT_FAILURE;
    }
    if (mode == "validate") ui.mode = 0;
    else if (mode == "union") ui.mode = 1;
    else if (mode == "subgraph") ui.mode = 2;
    else { fprintf(stderr, "mode %s does not exist. Terminating\n", argv[1]); return EXIT_FAILURE; }

    // one table per mode (src/main.cpp:78-97 validate, :298-315 subgraph, :220-229 union; --passes / -m of union: the HBM bound of
    // the merge); an option that a mode's table does not list never reaches the switch below
    static struct option validate_options[] = {
        {"coverage-cutoff", required_argument, 0, 'c'}, {"database", required_argument, 0, 'd'},
        {"input-positions", required_argument, 0, 'p'}, {"input-sequence", required_argument, 0, 'f'},
        {"kmer-length", required_argument, 0, 'k'}, {"search-depth", required_argument, 0, 0},
        {"max-span", required_argument, 0, 0}, {"out-format", required_argument, 0, 'o'},
        {"input-reads", required_argument, 0, 'r'}, {"tmp-prefix", required_argument, 0, 't'},
        {"max-memory", required_argument, 0, 'm'}, {"threads", required_argument, 0, 'j'},
        {"device", required_argument, 0, 0}, {"passes", required_argument, 0, 0},
        {"verbose", no_argument, &verbose_flag, 1}, {"cmd", no_argument, &cmd_flag, 1},
        {"version", no_argument, 0, 'v'}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
    static struct option subgraph_options[] = {
        {"coverage-cutoff", required_argument, 0, 'c'}, {"database", required_argument, 0, 'd'},
        {"input-sequence", required_argument, 0, 'f'}, {"traversal-algorithm", required_argument, 0, 0},
        {"search-depth", required_argument, 0, 0}, {"no-collapse", no_argument, &ui.noCollapse, 1},
        {"no-reference", no_argument, &ui.noReference, 1}, {"out-format", required_argument, 0, 'o'},
        {"input-positions", required_argument, 0, 'p'}, {"threads", required_argument, 0, 'j'},
        {"max-memory", required_argument, 0, 'm'}, {"device", required_argument, 0, 0},
        {"verbose", no_argument, &verbose_flag, 1}, {"cmd", no_argument, &cmd_flag, 1},
        {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
    static struct option union_options[] = {
        {"databases", required_argument, 0, 'd'}, {"out-format", required_argument, 0, 'o'},
        {"threads", required_argument, 0, 'j'}, {"device", required_argument, 0, 0},
        {"max-memory", required_argument, 0, 'm'}, {"passes", required_argument, 0, 0},
        {"verbose", no_argument, &verbose_flag, 1}, {"cmd", no_argument, &cmd_flag, 1},
        {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
    const struct option* long_options = ui.mode == 0 ? validate_options : ui.mode == 2 ? subgraph_options : union_options;
    const char* short_options = ui.mode == 0 ? "-:c:d:f:k:o:p:r:t:m:j:vh" : ui.mode == 2 ? "-:c:d:f:j:m:o:p:h" : "-:d:j:o:m:h";
    for (;;) {
        int option_index = 0;
        int c = getopt_long(argc, argv, short_options, long_options, &option_index);
        if (c == -1) break;
        switch (c) {
            case ':': fprintf(stderr, "option -%c is missing a required argument\n", optopt); return EXIT_FAILURE;
            case 0: {
                const char* name = long_options[option_index].name;
                if (strcmp(name, "search-depth") == 0) ui.kmerDepth = atoi(optarg);
                if (strcmp(name, "max-span") == 0) ui.maxSpan = atoi(optarg);
                if (strcmp(name, "traversal-algorithm") == 0) ui.travAlgorithm = optarg;
                if (strcmp(name, "device") == 0) ui.device = atoi(optarg);
                if (strcmp(name, "passes") == 0) ui.passes = std::max(0, atoi(optarg));
                break;
            }
            case 'c': ui.covCutOff = (uint32_t)number_arg(); break;
            case 'k': ui.kmerLen = number_arg(); break;
            case 'd':                                                // validate takes one database, union and subgraph every name that follows
                if (ui.mode == 0) { if_file_exists(optarg); ui.kmerDB.push_back(optarg); }
                else take_files(argc, argv, ui.kmerDB);
                break;
            case 'r': take_files(argc, argv, ui.inReads); break;
            case 'f': if_file_exists(optarg); ui.inSequence = optarg; break;
            case 'p': if_file_exists(optarg); ui.inBedInclude = optarg; break;
            case 'j': ui.maxThreads = atoi(optarg); break;
            case 'o': ui.outFile = optarg; break;
            case 't': ui.prefix = optarg; break;
            case 'm': ui.maxMem = atof(optarg); break;
            case 'v': printf("kreeq v%s (MI355X build)\n", kVersion); exit(0);
            case 'h': print_mode_help(ui.mode); break;
            default: break;                                          // positional arguments are ignored like the reference
        }
    }
    if (ui.mode == 0 && (ui.kmerLen < 2 || ui.kmerLen > 32)) { fprintf(stderr, "Invalid kmer length.\n"); return EXIT_FAILURE; }
    if (ui.mode == 1 && ui.kmerDB.size() < 2) { fprintf(stderr, "At least two databases required (-d).\n"); return EXIT_FAILURE; }   // src/main.cpp:290-293
    if (ui.mode == 2) {
        if (ui.kmerDB.size() != 1) { fprintf(stderr, "Need to provide one database (-d).\n"); return EXIT_FAILURE; }   // src/main.cpp:413-416
        if (!ui.inBedInclude.empty()) { fprintf(stderr, "Error: -p / --input-positions is not supported by this build (BED paths to segments are not built).\n"); return EXIT_FAILURE; }
        // KQ_SUBGRAPH_GFA=1 (off by default): the graph is built on the GPU (kq_subgraph_gfa), its block printed and -o <name>.gfa written
        if (!ui.outFile.empty() && !env_flag("KQ_SUBGRAPH_GFA")) { fprintf(stderr, "Error: -o %s: subgraph output files (GFA) are not supported by this build; the summary goes to stdout.\n", ui.outFile.c_str()); return EXIT_FAILURE; }
        if (!ui.outFile.empty() && !(ui.outFile.find('.') != std::string::npos && file_ext(ui.outFile) == "gfa")) {
            fprintf(stderr, "Error: -o %s: subgraph mode writes <name>.gfa only (GFA 1, uncompressed).\n", ui.outFile.c_str());
            return EXIT_FAILURE;
        }
        if (ui.travAlgorithm != "best-first" && ui.travAlgorithm != "traversal") {       // src/subgraph.cpp:296
            fprintf(stderr, "Cannot find input algorithm (%s). Terminating.\n", ui.travAlgorithm.c_str());
            return EXIT_FAILURE;
        }
    }
    if (cmd_flag) {
        for (int i = 0; i < argc; ++i) printf("%s ", argv[i]);
        printf("\n");
    }
    try {
        return run(ui);
    } catch (const std::exception& ex) {
        fprintf(stderr, "%s\n", ex.what());
        return EXIT_FAILURE;
    }
}
