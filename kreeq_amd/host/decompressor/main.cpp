// kreeq-decompressor -- reads the .bkwig files `kreeq validate -o x.bkwig` writes (reference src/decompressor.cpp).
//
//   inflate -i x.bkwig [--expand]    the whole file as .kwig text (or, with --expand, as the .csvtable text): the payload goes
//                                    through the device formatter kq_format_table in bounded chunks
//   lookup  -i x.bkwig (-c coords.bed | header:start-end) [-s span]
//                                    the lines of a few ranges: a seek and a handful of lines, formatted on the host with the
//                                    line rules of csrc/kq_table_core.h; runs without a GPU
//
// Two deliberate differences from the reference's lookup, both where it crashes or calls itself wrong: a range whose start lies
// in no component of its header (also begin - span < 1) is refused, and so is lookup --expand.
#include <getopt.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/kreeq_amd.h"
#include "../../csrc/kq_table_core.h"
#include "../bkwig_index.h"

namespace {

const char* kVersion = "0.0.1";
int verbose_flag = 0, cmd_flag = 0, expand_flag = 0;

[[noreturn]] void die(const std::string& msg) { fprintf(stderr, "%s\n", msg.c_str()); exit(EXIT_FAILURE); }

struct Options {
    std::string input, coordinates;
    uint64_t span = 0;
    std::vector<std::string> positional;
};

void help(bool lookup) {
    printf(lookup ? "kreeq-decompressor lookup [header:start-end]\n" : "kreeq-decompressor inflate\n");
    printf("\nOptions:\n\t-i --input-file .bkwig input.\n");
    if (lookup) printf("\t-c --coordinate-file sequence coordinates to extract (bed).\n\t-s --span <int> print context before and after coordinate positions.\n");
    else printf("\t--expand print the expanded table (.csvtable) instead of .kwig.\n");
    printf("\t-m --max-memory accepted, unused.\n\t-j --threads <n> accepted, unused.\n\t-v --version software version.\n\t--cmd print $0 to stdout.\n");
    exit(EXIT_SUCCESS);
}

Options parse(int argc, char** argv, bool lookup) {
    // the reference's option tables (src/decompressor.cpp:271-285, :361-377)
    static struct option inflate_options[] = {
        {"input-file", required_argument, 0, 'i'}, {"out-format", required_argument, 0, 'o'}, {"max-memory", required_argument, 0, 'm'},
        {"threads", required_argument, 0, 'j'},    {"expand", no_argument, &expand_flag, 1},  {"verbose", no_argument, &verbose_flag, 1},
        {"cmd", no_argument, &cmd_flag, 1},        {"version", no_argument, 0, 'v'},          {"help", no_argument, 0, 'h'},
        {0, 0, 0, 0}};
    static struct option lookup_options[] = {
        {"input-file", required_argument, 0, 'i'}, {"coordinate-file", required_argument, 0, 'c'}, {"span", required_argument, 0, 's'},
        {"out-format", required_argument, 0, 'o'}, {"max-memory", required_argument, 0, 'm'},      {"threads", required_argument, 0, 'j'},
        {"expand", no_argument, &expand_flag, 1},  {"verbose", no_argument, &verbose_flag, 1},     {"cmd", no_argument, &cmd_flag, 1},
        {"version", no_argument, 0, 'v'},          {"help", no_argument, 0, 'h'},
        {0, 0, 0, 0}};
    Options o;
    for (;;) {
        int index = 0;
        const int c = getopt_long(argc, argv, lookup ? "-:i:c:s:o:m:j:vh" : "-:i:o:m:j:vh", lookup ? lookup_options : inflate_options, &index);
        if (c == -1) break;
        switch (c) {
            case ':': die(std::string("option -") + (char)optopt + " is missing a required argument");
            case '?': die("unknown option");
            case 1: o.positional.push_back(optarg); break;               // ("-" in the option string: positional arguments arrive here)
            case 0: break;
            case 'i': o.input = optarg; break;
            case 'c': o.coordinates = optarg; break;
            case 's': o.span = (uint64_t)std::max(0ll, atoll(optarg)); break;
            case 'o': case 'm': case 'j': break;
            case 'v': printf("kreeq-decompressor v%s\n", kVersion); exit(EXIT_SUCCESS);
            case 'h': help(lookup);
        }
    }
    return o;
}

struct StringSink {
    std::string& s;
    void put(uint64_t at, char c) { s[(size_t)at] = c; }
};

// ---- lookup ---------------------------------------------------------------------------------------------------------------
struct Range { uint64_t begin, end; };

int run_lookup(std::ifstream& in, const BkwigIndex& idx, const Options& o) {
    if (expand_flag) die("Error: lookup --expand is not supported (the reference's own source calls its clamped case wrong); use inflate --expand.");
    // headers in order of first appearance, a header's ranges in file order
    std::vector<std::pair<std::string, std::vector<Range>>> sets;
    auto push = [&](const std::string& header, uint64_t begin, uint64_t end) {
        for (auto& s : sets) if (s.first == header) { s.second.push_back({begin, end}); return; }
        sets.push_back({header, {{begin, end}}});
    };
    if (o.positional.size() > 2) die("Error: too many positional arguments (" + o.positional[2] + ").");
    if (o.positional.size() == 2) {                                      // header:start-end
        const std::string& a = o.positional[1];
        const size_t colon = a.rfind(':'), dash = a.rfind('-');
        if (colon == std::string::npos || dash == std::string::npos || dash < colon) die("Error: cannot read the coordinate " + a + " (header:start-end).");
        push(a.substr(0, colon), strtoull(a.c_str() + colon + 1, nullptr, 10), strtoull(a.c_str() + dash + 1, nullptr, 10));
    }
    if (!o.coordinates.empty()) {
        std::ifstream bed(o.coordinates);
        if (!bed) die("Error: cannot open " + o.coordinates);
        std::string line, header;
        while (std::getline(bed, line)) {
            std::istringstream iss(line);
            uint64_t begin = 0, end = 0;
            if (iss >> header >> begin >> end) push(header, begin, end);
        }
    }
    if (sets.empty()) die("Error: lookup needs coordinates (-c coords.bed or header:start-end).");
    std::cout << std::to_string(idx.k) << "\n";
    for (auto& set : sets) {
        const BkwigPath* path = idx.find(set.first);
        if (!path) { std::cout.flush(); die("Could not find header (" + set.first + ") Exiting."); }
        for (const Range& r : set.second) {
            if (r.begin < o.span + 1) { std::cout.flush(); die("Error: " + set.first + ":" + std::to_string(r.begin) + " minus the span starts before the sequence."); }
            // src/decompressor.cpp:136-151 as written: the offset moves only when the range ends strictly inside the component
            // of its start; a range that reaches or overhangs the component's end is clamped and keeps the payload-start offset
            uint64_t start = r.begin - o.span - 1, end = r.end + o.span - 1;
            uint64_t offset = idx.payload_offset();
            bool found = false;
            for (const BkwigComponent& comp : path->comps) {
                if (!(start >= comp.abs_pos && start < comp.abs_pos + comp.len)) continue;
                found = true;
                if (end > comp.abs_pos + comp.len) end = comp.abs_pos + comp.len;
                else if (comp.abs_pos + comp.len > end) { offset += comp.byte_pos + (start - comp.abs_pos) * 12; break; }
            }
            if (!found) { std::cout.flush(); die("Error: " + set.first + ":" + std::to_string(start + 1) + " lies in no component of the sequence."); }
            const uint64_t len = end > start ? end - start : 0;
            std::vector<uint32_t> values((size_t)len * 3);
            in.clear();
            in.seekg((std::streamoff)offset);
            in.read((char*)values.data(), (std::streamsize)(len * 12));
            if ((uint64_t)in.gcount() != len * 12) { std::cout.flush(); die("Error: file truncated"); }
            std::string text;
            uint64_t bytes = 0;
            for (uint64_t i = 0; i < len; ++i) bytes += kqtab::fixed_line_len(values[i * 3], values[i * 3 + 1], values[i * 3 + 2]);
            text.resize((size_t)bytes);
            StringSink sink{text};
            uint64_t at = 0;
            for (uint64_t i = 0; i < len; ++i) at = kqtab::put_fixed_line(sink, at, values[i * 3], values[i * 3 + 1], values[i * 3 + 2]);
            std::cout << set.first << ":" << start + 1 << "-" << end + 1 << "\n" << text << "\n";
        }
    }
    std::cout.flush();
    return EXIT_SUCCESS;
}

// ---- inflate --------------------------------------------------------------------------------------------------------------
void kq_or_die(int rc) { if (rc != KQ_OK) die(std::string("Error: ") + kq_last_error()); }

uint64_t chunk_lines() { const char* e = getenv("KQ_TABLE_CHUNK_LINES"); return e ? (uint64_t)std::max(1ll, atoll(e)) : (1ull << 20); }

int run_inflate(std::ifstream& in, const BkwigIndex& idx, uint64_t file_bytes) {
    if (file_bytes - idx.payload_offset() != idx.payload_bytes) { std::cout << "Error: file truncated" << std::endl; return EXIT_FAILURE; }
    const int k = idx.k;
    if (k < 2 || k > 32) die("Error: the file states k = " + std::to_string(k) + ", outside 2..32.");
    kq_handle* h = nullptr;
    kq_or_die(kq_create(&h, 0, k, 128, 0));
    if (!expand_flag) std::cout << std::to_string(k) << "\n";
    std::string names;
    std::vector<uint32_t> name_off;
    for (auto& p : idx.paths) { name_off.push_back((uint32_t)names.size()); names += p.header; }
    // chunks of at most `chunk` positions: whole components, or parts of one; an expanded part carries the k - 1 positions
    // before it as its window's history
    const uint64_t chunk = chunk_lines();
    std::vector<kq_table_seg> segs;
    std::vector<uint32_t> triples;
    std::vector<char> out(1 << 20);
    uint64_t lines = 0, first_pos = 0, history = 0;                       // of the chunk being collected; first_pos: payload position of its first triple
    auto flush = [&]() {
        if (segs.empty()) return;
        const uint64_t n = history + lines;
        triples.resize((size_t)n * 3);
        in.clear();
        in.seekg((std::streamoff)(idx.payload_offset() + (first_pos - history) * 12));
        in.read((char*)triples.data(), (std::streamsize)(n * 12));
        if ((uint64_t)in.gcount() != n * 12) die("Error: file truncated");
        const int fmt = expand_flag ? KQ_TABLE_CSV : KQ_TABLE_KWIG;
        uint64_t need = 0;
        int rc = kq_format_table(h, fmt, triples.data(), n, segs.data(), segs.size(), names.data(), names.size(), out.data(), out.size(), &need);
        if (rc == KQ_ERR_CAPACITY) {
            out.resize((size_t)(need + need / 4));
            rc = kq_format_table(h, fmt, triples.data(), n, segs.data(), segs.size(), names.data(), names.size(), out.data(), out.size(), &need);
        }
        kq_or_die(rc);
        std::cout.write(out.data(), (std::streamsize)need);
        segs.clear(); lines = 0;
    };
    for (size_t p = 0; p < idx.paths.size(); ++p)
        for (const BkwigComponent& comp : idx.paths[p].comps) {
            uint64_t done = 0;
            do {                                                          // (an empty component still prints its fixedStep line)
                const uint64_t take = std::min(comp.len - done, chunk - lines);
                if (segs.empty()) { first_pos = comp.byte_pos / 12 + done; history = expand_flag ? std::min<uint64_t>(done, (uint64_t)k - 1) : 0; }
                kq_table_seg s{};
                s.first = comp.byte_pos / 12 + done - (first_pos - history);
                s.n = take;
                s.abs_pos = comp.abs_pos + done;
                s.name_off = name_off[p]; s.name_len = (uint32_t)idx.paths[p].header.size();
                s.n_ctx = expand_flag ? (uint32_t)std::min<uint64_t>(done, (uint64_t)k - 1) : 0;
                s.flags = done == 0 ? KQ_TABLE_SEG_HEADER : 0;
                segs.push_back(s);
                lines += take; done += take;
                if (lines >= chunk) flush();
            } while (done < comp.len);
        }
    flush();
    std::cout.flush();
    kq_destroy(h);
    return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { printf("kreeq-decompressor [mode]\n-h for additional help.\n\nModes:\ninflate\nlookup\n"); return EXIT_SUCCESS; }
    const bool lookup = strcmp(argv[1], "lookup") == 0;
    if (!lookup && strcmp(argv[1], "inflate") != 0) die(std::string("Unrecognized mode: ") + argv[1]);
    const Options o = parse(argc, argv, lookup);
    if (cmd_flag) { for (int i = 0; i < argc; ++i) printf("%s ", argv[i]); printf("\n"); }
    if (o.input.empty()) die("Error: no input file (-i x.bkwig).");
    std::ifstream in(o.input, std::ios::in | std::ios::binary);
    if (!in) die("Error: cannot open " + o.input);
    in.seekg(0, std::ios::end);
    const uint64_t file_bytes = (uint64_t)in.tellg();
    in.seekg(0);
    BkwigIndex idx;
    std::string err;
    if (!read_bkwig_index(in, idx, err)) {
        if (!lookup) { std::cout << "Error: file truncated" << std::endl; return EXIT_FAILURE; }
        die("Error: " + err);
    }
    return lookup ? run_lookup(in, idx, o) : run_inflate(in, idx, file_bytes);
}
