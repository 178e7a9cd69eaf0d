// Stand-alone driver of the map-image header walk (kreeq_amd/csrc/kq_dbimage_host.h), meant to be built with
// -fsanitize=address,undefined: every file named on the command line must walk clean, and every malformed variant derived
// from it must be refused.  Each image is copied into an exactly-sized heap block so that a read past its end is caught.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "kq_dbimage_host.h"

using namespace kq;

static const char* walk(const std::vector<uint8_t>& v, uint64_t* total) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[v.size() ? v.size() : 1]);
    if (!v.empty()) memcpy(exact.get(), v.data(), v.size());
    DbiExtent ext[DBI_SUBMAPS];
    return dbi_walk(exact.get(), v.size(), ext, total);
}
static int expect_refused(const char* what, const std::vector<uint8_t>& v, const std::string& path) {
    uint64_t total = 0;
    if (walk(v, &total)) return 0;
    fprintf(stderr, "%s: variant '%s' was accepted\n", path.c_str(), what);
    return 1;
}

int main(int argc, char** argv) {
    int bad = 0, n_files = 0;
    for (int a = 1; a < argc; ++a) {
        std::ifstream f(argv[a], std::ios::binary);
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        const std::vector<uint8_t> img((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        uint64_t total = 0;
        if (const char* why = walk(img, &total)) { fprintf(stderr, "%s: %s\n", argv[a], why); ++bad; continue; }
        ++n_files;
        // the extents of a clean walk lie inside the image and account for `total` entries
        DbiExtent ext[DBI_SUBMAPS];
        uint64_t sum = 0, t2 = 0;
        dbi_walk(img.data(), img.size(), ext, &t2);
        size_t first_used = DBI_SUBMAPS;
        for (size_t s = 0; s < DBI_SUBMAPS; ++s) {
            sum += ext[s].size;
            if (ext[s].size && first_used == DBI_SUBMAPS) first_used = s;
            if (ext[s].size && (ext[s].ctrl_off + ext[s].cap + 17 != ext[s].slot_off || ext[s].slot_off + ext[s].cap * 24 + 8 > img.size())) ++bad;
        }
        if (sum != total) ++bad;
        std::vector<uint8_t> v;
        v = img; v.pop_back();                      bad += expect_refused("one byte short", v, argv[a]);
        v = img; v.push_back(0);                    bad += expect_refused("one trailing byte", v, argv[a]);
        v = img; v[8] ^= 1;                         bad += expect_refused("version word changed", v, argv[a]);
        v = img; v[0] ^= 1;                         bad += expect_refused("submap count changed", v, argv[a]);
        v = img; v.resize(img.size() / 2);          bad += expect_refused("cut in half", v, argv[a]);
        v = img; v.resize(7);                       bad += expect_refused("seven bytes", v, argv[a]);
        v.clear();                                  bad += expect_refused("empty", v, argv[a]);
        if (first_used < DBI_SUBMAPS) {
            const size_t hdr = (size_t)ext[first_used].ctrl_off - 24;          // version, size, capacity of that submap
            v = img; memset(v.data() + hdr + 16, 0xFF, 8);                     bad += expect_refused("capacity 2^64 - 1", v, argv[a]);
            v = img; v[hdr + 16] ^= 2;                                         bad += expect_refused("capacity no 2^n - 1", v, argv[a]);
            v = img; memset(v.data() + hdr + 8, 0xFF, 7);                      bad += expect_refused("size above capacity", v, argv[a]);
            v = img; { uint64_t c; memcpy(&c, v.data() + hdr + 16, 8); c = c * 2 + 1; memcpy(v.data() + hdr + 16, &c, 8); }
                                                                               bad += expect_refused("capacity doubled", v, argv[a]);
        }
    }
    printf("%d files walked, %d failures\n", n_files, bad);
    return bad ? 1 : 0;
}
