// Reading and writing .kreeq databases by map range, through the host (de)serialiser or the device images; see db_source.h.
#include "db_source.h"

#include <memory>

namespace kqhost {

namespace {

bool db_device() { return env_flag("KQ_DB_DEVICE"); }

struct DbTrace {
    const char* what; double t0 = now_s(); uint64_t pcie = 0;          // pcie: the bytes that crossed PCIe
    explicit DbTrace(const char* w) : what(w) {}
    ~DbTrace() {
        if (env_flag("KQ_DB_TRACE")) fprintf(stderr, "[db] %s: %.3f s, %llu bytes over PCIe (%s)\n", what, now_s() - t0, (unsigned long long)pcie, db_device() ? "device" : "host");
    }
};

// the files of maps [lo, hi) from the table of h, in sub-ranges whose image, entries and sort scratch fit the free HBM
uint64_t write_db_maps_device(kq_handle* h, int device, const std::string& db, int lo, int hi, std::vector<kq_entry>& hc_all) {
    ::mkdir(db.c_str(), 0777);
    std::vector<uint64_t> off((size_t)(hi - lo) + 1);
    uint64_t n_hc = 0, bytes_out = 0;
    kq_or_die(kq_export_map_images(h, (uint16_t)lo, (uint16_t)hi, nullptr, 0, off.data(), nullptr, 0, &n_hc));
    uint64_t free_b = 0, total_b = 0;
    if (kq_device_memory(device, &free_b, &total_b) != KQ_OK) free_b = 8ull << 30;
    // a slot is 24 bytes at a load of at most 7/8: an image of B bytes holds at most B / 27 k-mers, each of which takes
    // 48 B as an entry twice (unsorted, sorted), 24 B of sort keys and 16 B of split records beside the image: < 6 B in all
    const uint64_t budget = std::max<uint64_t>(free_b / 2 / 6, 1);
    std::vector<uint8_t> img;
    std::vector<kq_entry> hc;
    for (int a = lo; a < hi;) {
        int b = a + 1;
        while (b < hi && off[(size_t)(b + 1 - lo)] - off[(size_t)(a - lo)] <= budget) ++b;
        std::vector<uint64_t> o((size_t)(b - a) + 1);
        kq_or_die(kq_export_map_images(h, (uint16_t)a, (uint16_t)b, nullptr, 0, o.data(), nullptr, 0, &n_hc));
        img.resize((size_t)o.back());
        hc.resize((size_t)n_hc);
        kq_or_die(kq_export_map_images(h, (uint16_t)a, (uint16_t)b, img.data(), img.size(), o.data(), hc.data(), hc.size(), &n_hc));
        for (int m = a; m < b; ++m) {
            const std::string path = db + "/.map." + std::to_string(m) + ".bin";
            FILE* f = fopen(path.c_str(), "wb");
            const size_t len = (size_t)(o[(size_t)(m + 1 - a)] - o[(size_t)(m - a)]);
            if (!f || fwrite(img.data() + o[(size_t)(m - a)], 1, len, f) != len || fclose(f) != 0) die("Error: cannot write " + path);
        }
        hc_all.insert(hc_all.end(), hc.begin(), hc.end());
        bytes_out += img.size() + hc.size() * sizeof(kq_entry);
        a = b;
    }
    return bytes_out;
}

}  // namespace

void export_db_maps(kq_handle* h, int device, const std::string& db, int map_count, int lo, int hi, std::vector<kq_entry>& hc_all) {
    DbTrace tr("export + write maps");
    if (db_device()) { tr.pcie = write_db_maps_device(h, device, db, lo, hi, hc_all); return; }
    uint64_t n = 0;
    kq_or_die(kq_export(h, (uint16_t)lo, (uint16_t)hi, nullptr, 0, &n));
    std::vector<kq_entry> entries((size_t)n);
    if (n) kq_or_die(kq_export(h, (uint16_t)lo, (uint16_t)hi, entries.data(), n, &n));
    verbose("Table exported (" + std::to_string(n) + " k-mers)");
    tr.pcie = n * sizeof(kq_entry);
    write_db_maps(db, map_count, lo, hi, entries, hc_all);
}

uint64_t DbSource::entries_bound(int lo, int hi) const {
    uint64_t n = 0;
    for (int m = lo; m < hi; ++m) n += map_entries_bound(m);
    for (auto& e : hc) { const int m = (int)(e.key % (uint64_t)idx.map_count); n += m >= lo && m < hi; }
    return n;
}

// KQ_DB_DEVICE: every map file goes to the GPU as it lies on disk, through one reused page-locked buffer
uint64_t DbSource::import_into_device(kq_handle* h, int lo, int hi, uint64_t& pcie) const {
    uint64_t total = 0, n_tomb = 0, cap = 0;
    for (int m = lo; m < hi; ++m) cap = std::max(cap, file_size(map_path(m)));
    uint8_t* buf = (uint8_t*)kq_host_alloc(std::max<uint64_t>(cap, 1));
    if (!buf) die("Error: cannot allocate a page-locked buffer for the map files");
    for (int m = lo; m < hi; ++m) {
        const std::string path = map_path(m);
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) die("Error: cannot open " + path);
        const size_t len = fread(buf, 1, (size_t)cap, f);
        const bool whole = len < cap || fgetc(f) == EOF;            // the file did not grow behind the size taken above
        fclose(f);
        if (!whole) die("Error: " + path + " changed while it was read");
        uint64_t n = 0, t = 0;
        kq_or_die(kq_import_map_image(h, (uint16_t)m, buf, len, &n, &t));
        total += n; n_tomb += t; pcie += len;
    }
    kq_host_free(buf);
    std::vector<kq_entry> v;                                    // the range's high-copy entries, as read_db_maps appends them
    for (auto& e : hc) { const int m = (int)(e.key % (uint64_t)idx.map_count); if (m >= lo && m < hi) v.push_back(e); }
    if (n_tomb > v.size()) die("Error: int32 map missing 255 value from int8 map");   // src/kreeq.cpp:162
    kq_or_die(kq_import(h, v.data(), v.size()));
    pcie += v.size() * sizeof(kq_entry);
    return total + v.size();
}

uint64_t DbSource::import_into(kq_handle* h, int lo, int hi) const {
    DbTrace tr("read + import maps");
    if (db_device()) return import_into_device(h, lo, hi, tr.pcie);
    std::vector<kq_entry> v;
    uint64_t total = 0;
    const size_t chunk = (size_t)env_u64("KQ_DB_CHUNK_ENTRIES", (uint64_t)1 << 25);      // 1.6 GB of host memory
    for (int a = lo; a < hi;) {
        int b = a;
        uint64_t est = 0;
        do { est += map_entries_bound(b); ++b; } while (b < hi && est + map_entries_bound(b) <= chunk);
        v.clear();
        read_db_maps(dir, idx, a, b, hc, v);
        kq_or_die(kq_import(h, v.data(), v.size()));
        total += v.size();
        tr.pcie += v.size() * sizeof(kq_entry);
        a = b;
    }
    return total;
}

// A lookup round asks every range that owns one of its keys (the resident one first), the pre-filter is the OR of the
// ranges' scans (a k-mer is in exactly one range).  The reference's search loops over the map ranges in the same way
// (src/variants.cpp:78-84) with a cache of the entries it has seen (:199-210) -- here the host-side cache of
// find_candidate_errors.
GraphSource graph_of_db_ranges(kq_handle* h, const DbSource& db, int passes) {
    auto cur = std::make_shared<int>(-1);
    auto load = [h, &db, passes, cur](int p) {
        if (*cur == p) return;
        const auto r = pass_range(p, passes, db.idx.map_count);
        kq_or_die(kq_clear(h));
        db.import_into(h, r.first, r.second);
        *cur = p;
        verbose("Variant search: maps [" + std::to_string(r.first) + "," + std::to_string(r.second) + ") loaded");
    };
    GraphSource g;
    g.branch_scan = [h, passes, load](const std::string& joined, uint32_t cov_cutoff, std::vector<uint8_t>& flags) {
        std::vector<uint8_t> part(joined.size());
        std::fill(flags.begin(), flags.end(), 0);
        for (int p = 0; p < passes; ++p) {
            load(p);
            kq_or_die(kq_branch_scan(h, joined.data(), joined.size(), cov_cutoff, part.data()));
            for (size_t i = 0; i < flags.size(); ++i) flags[i] |= part[i];
        }
    };
    g.lookup = [h, &db, passes, load, cur](const std::vector<uint64_t>& want, std::vector<kq_entry>& got) {
        const int mc = db.idx.map_count;
        std::vector<std::vector<size_t>> by(passes);
        for (size_t i = 0; i < want.size(); ++i) {
            const int m = (int)(want[i] % (uint64_t)mc);
            int p = (int)(((long long)(m + 1) * passes - 1) / mc);          // the range [p mc / passes, (p + 1) mc / passes) that holds map m
            while (pass_range(p, passes, mc).first > m) --p;
            while (pass_range(p, passes, mc).second <= m) ++p;
            by[p].push_back(i);
        }
        std::vector<uint64_t> sub;
        std::vector<kq_entry> res;
        const int start = *cur < 0 ? 0 : *cur;
        for (int q = 0; q < passes; ++q) {
            const int p = (start + q) % passes;
            if (by[p].empty()) continue;
            load(p);
            sub.clear();
            for (size_t i : by[p]) sub.push_back(want[i]);
            res.resize(sub.size());
            kq_or_die(kq_lookup_keys(h, sub.data(), sub.size(), res.data()));
            for (size_t j = 0; j < sub.size(); ++j) got[by[p][j]] = res[j];
        }
    };
    return g;
}

}  // namespace kqhost
