// The host's BGZF stream writer (kreeq_amd/host/bgzf_out.h) as a stand-alone program: prints n compressible bytes and n random
// bytes through a BgzfBuf into <file>, and the same text to stdout.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#include "bgzf_out.h"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: bgzf_out <n> <file>\n"); return 2; }
    const size_t n = (size_t)atoll(argv[1]);
    std::string text;
    for (size_t i = 0; i < n; ++i) text.push_back("12,7,7\n"[i % 7]);
    uint32_t x = 99;
    for (size_t i = 0; i < n; ++i) { x = x * 1664525u + 1013904223u; text.push_back((char)(x >> 24)); }
    std::ofstream file(argv[2], std::ios::binary | std::ios::trunc);
    kqhost::BgzfBuf gz(file);
    std::ostream os(&gz);
    // in pieces of changing size, some through operator<< of single characters
    for (size_t at = 0, step = 1; at < text.size(); at += step, step = step * 3 % 7919 + 1) {
        const size_t m = std::min(step, text.size() - at);
        if (m == 1) os << text[at]; else os.write(text.data() + at, (std::streamsize)m);
    }
    if (!gz.finish()) { fprintf(stderr, "write failed\n"); return 1; }
    fwrite(text.data(), 1, text.size(), stdout);
    return 0;
}
