// cli_common.h -- what every translation unit of the `kreeq` CLI shares: the parsed command line, the error exits, the verbose
// log, the clock and the two readers of environment switches.
#pragma once
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "kreeq_amd.h"

namespace kqhost {

struct UserInput {                       // reference UserInputKreeq (include/input.h:25-34) + gfalibs UserInput fields used
    int mode = 0;                        // 0 validate, 1 union, 2 subgraph
    std::string inSequence, outFile, prefix = ".", inBedInclude;
    std::vector<std::string> inReads, kmerDB;
    int kmerLen = 21;
    uint32_t covCutOff = 0;
    int kmerDepth = -1, maxSpan = 5, maxThreads = 0;
    double maxMem = 0;
    int device = 0;
    int passes = 0;                      // --passes: count the maps in this many ranges (memory-bounded mode); 0 = as many as the HBM asks for
    std::string travAlgorithm = "best-first";      // subgraph (include/input.h:32)
    int noCollapse = 0, noReference = 0;
};

inline int verbose_flag = 0;

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline const double t_start = now_s();
inline void verbose(const std::string& s) { if (verbose_flag) fprintf(stderr, "[%8.3f s] %s\n", now_s() - t_start, s.c_str()); }

[[noreturn]] inline void die(const std::string& msg) {
    fprintf(stderr, "%s\n", msg.c_str());
    exit(EXIT_FAILURE);
}
inline void kq_or_die(int rc) { if (rc != KQ_OK) die(std::string("Error: ") + kq_last_error()); }

// NAME=<non-zero integer> switches a device path or a trace on; a numeric knob is at least 1
inline bool env_flag(const char* name) { const char* e = getenv(name); return e && atoi(e) != 0; }
inline uint64_t env_u64(const char* name, uint64_t dflt) { const char* e = getenv(name); return e ? (uint64_t)std::max(1ll, atoll(e)) : dflt; }

inline uint64_t file_size(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 ? (uint64_t)st.st_size : 0; }

// ingest.cpp: the reads of one file counted into the table of h through a pool of page-locked buffers
void count_reads_file(kq_handle* h, const std::string& path, unsigned threads, uint64_t input_bytes, int device);
unsigned parser_threads(const UserInput& ui, uint64_t input_bytes);
// run.cpp: validate, union and subgraph
int run(UserInput& ui);

}  // namespace kqhost
