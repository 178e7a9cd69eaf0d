// Stand-alone driver of kreeq_amd/host/gfa_out.h for tests/test_gfa_out_host.py (built with -fsanitize=address,undefined).
// argv[1]: a graph as lines -- "k <k>", "Q <bases>" (or "Q" alone), "S <seq_off> <head_key> <n_kmers> <cov> <head_rc>",
// "E <from> <to> <count> <from_rc> <to_rc>".  stdout: the GFA text, a line "==", the block; "invalid" for records out of bounds.
#include <cstdio>
#include <fstream>
#include <sstream>

#include "gfa_out.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: gfa_out <graph file>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    kqhost::GfaGraph g;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string kind;
        ls >> kind;
        if (kind == "k") ls >> g.k;
        else if (kind == "Q") ls >> g.seq;
        else if (kind == "S") {
            kq_gfa_segment s{};
            unsigned rc = 0;
            ls >> s.seq_off >> s.head_key >> s.n_kmers >> s.cov >> rc;
            s.head_rc = (uint8_t)rc;
            g.segs.push_back(s);
        } else if (kind == "E") {
            kq_gfa_edge e{};
            unsigned a = 0, b = 0;
            ls >> e.from >> e.to >> e.count >> a >> b;
            e.from_rc = (uint8_t)a; e.to_rc = (uint8_t)b;
            g.edges.push_back(e);
        } else if (!kind.empty()) { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
    }
    if (!kqhost::gfa_valid(g)) { printf("invalid\n"); return 0; }
    std::string text, block;
    kqhost::gfa_text(g, text);
    kqhost::gfa_block(kqhost::gfa_stats(g), block);
    fwrite(text.data(), 1, text.size(), stdout);
    printf("==\n");
    fwrite(block.data(), 1, block.size(), stdout);
    return 0;
}
