// The QV table and the per-base outputs of `kreeq validate` (reference src/kreeq.cpp:78-106, src/kreeq-output.cpp:138-399):
// three host writers over the per-base vector, and the same four files from the device: from one lookup over a resident
// table, or accumulated over map ranges.
#include "per_base.h"

#include "bgzf_out.h"

#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <charconv>
#include <cmath>
#include <cstring>
#include <fstream>
#include <future>
#include <iostream>
#include <sstream>

namespace kqhost {

namespace {

double error_rate(uint64_t missing, uint64_t total, int k) { return 1 - pow(1 - (double)missing / total, (double)1 / k); }      // src/kreeq.cpp:36-40
const kq_dbgbase* bases_of(const Run& r, size_t s, uint64_t seg_start) { return r.per_base.data() + r.genome.offset[s] + seg_start; }

// .kwig (src/kreeq-output.cpp:243-303) and .bkwig (:305-399)
void write_kwig(const Run& r, const SegmentLists& segs, std::ostream& ofs, BgzfBuf* gz) {
    ofs << std::to_string(r.k) << "\n";
    if (gz) gz->cut();                                                   // the head line is a member of its own, as the device writer has it
    for (size_t s = 0; s < r.seqs.size(); ++s)
        for (auto& seg : segs[s]) {
            ofs << "fixedStep chrom=" << r.seqs[s].header << " start=" << seg.first << " step=1" << "\n";
            const kq_dbgbase* b = bases_of(r, s, seg.first);
            char line[33];                                               // three u32 of at most 10 digits, two commas, the line end
            for (uint64_t i = 0; i < seg.second; ++i) {
                const Triple t = oriented(b[i]);
                char* p = std::to_chars(line, line + 10, t.cov).ptr; *p++ = ',';
                p = std::to_chars(p, p + 10, t.fw).ptr; *p++ = ',';
                p = std::to_chars(p, p + 10, t.bw).ptr; *p++ = '\n';
                ofs.write(line, p - line);
            }
        }
}
void write_bkwig_index(std::ostream& ofs, const Run& r, const SegmentLists& segs) {
    uint8_t k8 = (uint8_t)r.k;
    ofs.write((const char*)&k8, 1);
    uint32_t nPaths = (uint32_t)r.seqs.size();
    ofs.write((const char*)&nPaths, 4);
    for (size_t s = 0; s < r.seqs.size(); ++s) {                                 // writeIndex :305-355
        uint16_t hl = (uint16_t)r.seqs[s].header.size();
        ofs.write((const char*)&hl, 2);
        ofs << r.seqs[s].header;
        uint32_t nc = (uint32_t)segs[s].size();
        ofs.write((const char*)&nc, 4);
        for (auto& seg : segs[s]) {
            uint8_t step = 1;
            ofs.write((const char*)&seg.first, 8);
            ofs.write((const char*)&seg.second, 8);
            ofs.write((const char*)&step, 1);
        }
    }
}
void write_bkwig(const Run& r, const SegmentLists& segs) {
    std::ofstream ofs(r.ui.outFile, std::ios::trunc | std::ios::out | std::ios::binary);
    write_bkwig_index(ofs, r, segs);
    for (size_t s = 0; s < r.seqs.size(); ++s)
        for (auto& seg : segs[s]) {
            const kq_dbgbase* b = bases_of(r, s, seg.first);
            for (uint64_t i = 0; i < seg.second; ++i) { const Triple t = oriented(b[i]); ofs.write((const char*)&t, sizeof t); }
        }
}
// .bed / .csvtable per-base table (src/kreeq-output.cpp:138-241): for every position the k most
// recent values of cov / fw-edge / bw-edge, oldest first.  No fixture of the reference pins this
// text (parity unpinned); it is restated from the writer's source.
void write_table(const Run& r, const SegmentLists& segs, std::ostream& ofs) {
    const int k = r.k;
    char colSep = ',', entrySep = ',';
    if (r.plan.table_format() == "bed") colSep = '\t', entrySep = ':';
    for (size_t s = 0; s < r.seqs.size(); ++s)
        for (auto& seg : segs[s]) {
            std::vector<uint32_t> kc(k - 1, 0), ef(k - 1, 0), eb(k - 1, 0);
            const kq_dbgbase* b = bases_of(r, s, seg.first);
            for (uint64_t i = 0; i < seg.second; ++i) {
                ofs << r.seqs[s].header << colSep << (seg.first + i) << colSep;
                const Triple t = oriented(b[i]);
                kc.push_back(t.cov); ef.push_back(t.fw); eb.push_back(t.bw);
                for (auto* v : {&kc, &ef, &eb}) {
                    for (int c = 0; c < k; ++c) { ofs << std::to_string((*v)[(size_t)c]); if (c < k - 1) ofs << entrySep; }
                    if (v != &eb) ofs << colSep;
                    v->erase(v->begin());
                }
                ofs << "\n";
            }
        }
}

// The file of the device writer, two page-locked buffers and the write in flight: the copy and the format of chunk j + 1 run
// while a writer thread hands chunk j to the file with one write() call.
struct TableOut {
    int fd = -1;
    char* buf[2] = {nullptr, nullptr};
    uint64_t cap[2] = {0, 0};
    std::future<double> pending;
    uint64_t n = 0, bytes = 0;
    double t_write = 0;
    ~TableOut() { if (pending.valid()) pending.wait(); for (char* p : buf) kq_host_free(p); if (fd >= 0) ::close(fd); }
    static double write_all(int fd, const char* p, uint64_t len) {
        const double t0 = now_s();
        while (len) {                                                // one call, unless the kernel takes less
            const ssize_t w = ::write(fd, p, (size_t)len);
            if (w < 0) { if (errno == EINTR) continue; die(std::string("Error: write failed: ") + strerror(errno)); }
            p += w; len -= (uint64_t)w;
        }
        return now_s() - t0;
    }
    void direct(const std::string& s) { wait(); t_write += write_all(fd, s.data(), s.size()); bytes += s.size(); }
    void wait() { if (pending.valid()) t_write += pending.get(); }
    // the buffer the next chunk goes to, with room for `need` bytes (its previous content has reached the file)
    char* next(uint64_t need) {
        const int b = (int)(n & 1);
        if (cap[b] < need) {
            kq_host_free(buf[b]);
            cap[b] = need + need / 8 + 4096;
            buf[b] = (char*)kq_host_alloc(cap[b]);
            if (!buf[b]) die("Error: no page-locked memory for " + std::to_string(cap[b]) + " bytes of table output");
        }
        return buf[b];
    }
    // the chunk in next()'s buffer is complete: wait for the write before it, start this one
    void submit(uint64_t len) {
        const int b = (int)(n & 1);
        wait();
        const int f = fd; const char* p = buf[b];
        pending = std::async(std::launch::async, [f, p, len] { return write_all(f, p, len); });
        bytes += len; ++n;
    }
};

// "Triples on the device -> file", the half that both device paths share: the file with its head (.kwig's k, .bkwig's index),
// and per call -- sequences [lo, hi), whose triples lie segment after segment at d_triples -- the payload copied out as it is
// (.bkwig) or formatted in chunks of at most KQ_TABLE_CHUNK_LINES positions (cut_table_chunks + kq_format_table_dev), through
// the two page-locked buffers of TableOut.  With a .gz name every formatted chunk is deflated on the device into BGZF members
// (kq_deflate_bgzf_dev) and only those cross to the host; the head line is a member of its own, finish() writes the marker.
struct DeviceTableFile {
    const Run& r;
    kq_handle* h;
    const SegmentLists& segs;
    const int fmt;                                                   // 0: .bkwig
    const uint64_t chunk = env_u64("KQ_TABLE_CHUNK_LINES", (uint64_t)1 << 20);
    TableOut out;
    std::string names;
    std::vector<uint32_t> name_off;
    char* d_text = nullptr;
    uint64_t d_text_cap = 0;
    const bool gz;                                                   // BGZF members instead of text
    char* d_gz = nullptr;
    uint64_t d_gz_cap = 0, text_bytes = 0;
    double t_format = 0, t_copy = 0, t_deflate = 0;
    static int format_of(const std::string& ext) { return ext == "kwig" ? KQ_TABLE_KWIG : ext == "bed" ? KQ_TABLE_BED : ext == "csvtable" ? KQ_TABLE_CSV : 0; }
    DeviceTableFile(const Run& run, const SegmentLists& sl) : r(run), h(run.h), segs(sl), fmt(format_of(run.plan.table_format())), gz(run.plan.table_gz) {
        out.fd = ::open(r.ui.outFile.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (out.fd < 0) die("Error: cannot write " + r.ui.outFile + ": " + strerror(errno));
        if (fmt == KQ_TABLE_KWIG) { const std::string head = std::to_string(r.k) + "\n"; text_bytes += head.size(); out.direct(gz ? bgzf_member(head.data(), head.size()) : head); }
        if (fmt == 0) { std::ostringstream index; write_bkwig_index(index, r, segs); out.direct(index.str()); }
        for (auto& s : r.seqs) { name_off.push_back((uint32_t)names.size()); names += s.header; }
        name_off.push_back((uint32_t)names.size());
    }
    ~DeviceTableFile() { kq_dev_free(h, d_text); kq_dev_free(h, d_gz); }
    // a chunk that lies on the device -> the next page-locked buffer -> the file; as BGZF members when the name asks for them
    void copy_out(const void* d_src, uint64_t bytes) {
        text_bytes += bytes;
        if (gz) {
            const uint64_t bound = kq_bgzf_bound(bytes, 0);
            if (bound > d_gz_cap) {
                kq_dev_free(h, d_gz); d_gz_cap = bound + bound / 8 + 4096; d_gz = (char*)kq_dev_alloc(h, d_gz_cap);
                if (!d_gz) die("Error: no device memory for " + std::to_string(d_gz_cap) + " bytes of compressed table output");
            }
            const double t0 = now_s();
            uint64_t n = 0;
            kq_or_die(kq_deflate_bgzf_dev(h, (const char*)d_src, bytes, d_gz, d_gz_cap, &n, 0));
            t_deflate += now_s() - t0;
            d_src = d_gz; bytes = n;
        }
        char* dst = out.next(bytes);
        const double t0 = now_s();
        kq_or_die(kq_copy_async(h, dst, d_src, bytes, KQ_COPY_TO_HOST));
        kq_or_die(kq_sync(h));
        t_copy += now_s() - t0;
        out.submit(bytes);
    }
    void write_call(size_t lo, size_t hi, const uint32_t* d_triples, uint64_t n_triples) {
        if (fmt == 0) {                                              // .bkwig: the payload is the triples
            for (uint64_t a = 0; a < n_triples; a += chunk) copy_out(d_triples + a * 3, std::min(chunk, n_triples - a) * 12);
            return;
        }
        for (auto& pieces : cut_table_chunks(segs, lo, hi, name_off, chunk, r.k, fmt == KQ_TABLE_BED || fmt == KQ_TABLE_CSV)) {      // the text, chunk by chunk
            uint64_t need = 0;
            const double t0 = now_s();
            kq_or_die(kq_format_table_dev(h, fmt, d_triples, n_triples, pieces.data(), pieces.size(), names.data(), names.size(), nullptr, 0, &need));
            if (need > d_text_cap) {
                kq_dev_free(h, d_text); d_text_cap = need + need / 8 + 4096; d_text = (char*)kq_dev_alloc(h, d_text_cap);
                if (!d_text) die("Error: no device memory for " + std::to_string(d_text_cap) + " bytes of the per-base table");
            }
            kq_or_die(kq_format_table_dev(h, fmt, d_triples, n_triples, pieces.data(), pieces.size(), names.data(), names.size(), d_text, d_text_cap, &need));
            t_format += now_s() - t0;
            copy_out(d_text, need);
        }
    }
    void finish() { if (gz) out.direct(bgzf_eof_marker()); out.wait(); }      // every chunk has reached the file
};

}  // namespace

void print_qv(const Run& r) {
    if (!r.plan.want_qv) return;
    const int k = r.k;
    const uint64_t missing = r.counters[0], total = r.counters[1], edge_missing = r.counters[2];
    std::cout << "Missing" << "\t" << "Total" << "\t" << "QV" << "\t" << "Error" << "\t" << "k" << "\t" << "Method" << std::endl;
    double merquryError = error_rate(missing, total, k), merquryQV = -10 * log10(merquryError);
    std::cout << missing << "\t" << total << "\t" << merquryQV << "\t" << merquryError << "\t" << std::to_string(k) << "\t"
              << "Merqury" << std::endl;
    double kreeqError = error_rate(missing + edge_missing, total, k), kreeqQV = -10 * log10(kreeqError);
    std::cout << missing + edge_missing << "\t" << total << "\t" << kreeqQV << "\t" << kreeqError << "\t" << std::to_string(k)
              << "\t" << "Kreeq" << std::endl;
}

bool table_device_wanted(const Run& r) { return env_flag("KQ_TABLE_DEVICE") && !r.ui.inSequence.empty() && all_fit(r.seqs, kDeviceCallBytes); }

// Whole sequences are grouped into calls of at most kDeviceCallBytes of joined text.  Per call the lookup fills a per-base
// array that stays on the device, kq_per_base_triples_dev makes the .bkwig payload of the call's segments from it, and
// DeviceTableFile takes that payload to the file.  KQ_TABLE_TRACE=1 prints the wall clock of the steps to stderr.
void write_per_base_device(Run& r) {
    verbose("per-base table written by the device formatter");
    if (r.plan.table_gz) verbose("per-base table compressed by the device deflater");
    verbose("Validating sequence");
    kq_handle* h = r.h;
    const SegmentLists segs = all_segments(r.seqs);
    DeviceTableFile file(r, segs);
    double t_lookup = 0;
    auto dev_alloc = [&](uint64_t bytes) { void* p = kq_dev_alloc(h, bytes); if (!p) die("Error: no device memory for " + std::to_string(bytes) + " bytes of the per-base table"); return p; };
    for (size_t lo = 0, hi; lo < r.seqs.size(); lo = hi) {
        hi = next_call(r.seqs, lo, kDeviceCallBytes);
        const uint64_t len = (hi < r.seqs.size() ? r.genome.offset[hi] : r.genome.text.size()) - r.genome.offset[lo];
        // 1. lookup with the per-base array on the device, 2. the triples of the call's segments
        const double t0 = now_s();
        std::vector<uint64_t> seg_start, seg_len;
        uint64_t n_triples = 0;
        for (size_t s = lo; s < hi; ++s)
            for (auto& seg : segs[s]) { seg_start.push_back(r.genome.offset[s] - r.genome.offset[lo] + seg.first); seg_len.push_back(seg.second); n_triples += seg.second; }
        char* d_bases = (char*)dev_alloc(len);
        kq_dbgbase* d_pb = (kq_dbgbase*)dev_alloc(len * sizeof(kq_dbgbase));                // (zero-filled)
        uint64_t* d_ctr = (uint64_t*)dev_alloc(3 * sizeof(uint64_t));
        uint32_t* d_triples = (uint32_t*)dev_alloc(n_triples * 12);
        kq_or_die(kq_copy_async(h, d_bases, r.genome.text.data() + r.genome.offset[lo], len, KQ_COPY_TO_DEVICE));
        kq_or_die(kq_lookup_sequence_dev(h, d_bases, len, r.ui.covCutOff, 0, (uint16_t)r.map_count, d_pb, d_ctr));
        kq_or_die(kq_per_base_triples_dev(h, d_pb, seg_start.data(), seg_len.data(), seg_start.size(), d_triples));
        uint64_t ctr[3] = {0, 0, 0};
        kq_or_die(kq_copy_async(h, ctr, d_ctr, sizeof ctr, KQ_COPY_TO_HOST));
        kq_or_die(kq_sync(h));
        for (int i = 0; i < 3; ++i) r.counters[i] += ctr[i];
        kq_dev_free(h, d_bases); kq_dev_free(h, d_pb); kq_dev_free(h, d_ctr);
        t_lookup += now_s() - t0;
        file.write_call(lo, hi, d_triples, n_triples);               // 3. the file
        kq_dev_free(h, d_triples);                                   // (every chunk of the call has left the device)
    }
    file.finish();
    print_qv(r);
    if (env_flag("KQ_TABLE_TRACE")) {
        fprintf(stderr, "[table] device: lookup %.3f s, format %.3f s, copy %.3f s, write %.3f s, %llu bytes", t_lookup, file.t_format, file.t_copy, file.out.t_write, (unsigned long long)(r.plan.table_gz ? file.text_bytes : file.out.bytes));
        if (r.plan.table_gz) fprintf(stderr, ", deflate %.3f s, %llu compressed bytes", file.t_deflate, (unsigned long long)file.out.bytes);
        fprintf(stderr, "\n");
    }
}

// ---- the same under map-range passes: the triples accumulate on the device ------------------------------------------------
bool table_passes_wanted(const Run& r) { return env_flag("KQ_TABLE_DEVICE") && env_flag("KQ_TABLE_DEVICE_PASSES") && !r.ui.inSequence.empty(); }

static void table_passes_free(Run& r, TablePasses& t) {
    kq_dev_free(r.h, t.d_acc); kq_dev_free(r.h, t.d_text); kq_dev_free(r.h, t.d_pb); kq_dev_free(r.h, t.d_ctr);
    t.d_acc = nullptr; t.d_text = nullptr; t.d_pb = nullptr; t.d_ctr = nullptr;
}

bool table_passes_begin(Run& r, TablePasses& t) {
    t.segs = all_segments(r.seqs);
    t.plan = plan_table_passes(r.seqs, t.segs, env_u64("KQ_TABLE_CALL_BYTES", kDeviceCallBytes));
    t.trace = env_flag("KQ_TABLE_TRACE");
    const uint64_t bytes = t.plan.device_bytes();
    auto fall_back = [&](const std::string& why) {
        table_passes_free(r, t);
        verbose("per-base table not accumulated on the device (" + std::to_string(bytes) + " bytes): " + why);
        return false;
    };
    if (!t.plan.fits) return fall_back("a sequence exceeds the call limit");
    if (bytes > env_u64("KQ_TABLE_ACC_MAX_BYTES", ~0ull)) return fall_back("more than KQ_TABLE_ACC_MAX_BYTES");
    t.d_acc = (uint32_t*)kq_dev_alloc(r.h, t.plan.acc_bytes);        // (all four zero-filled)
    t.d_text = (char*)kq_dev_alloc(r.h, t.plan.max_text);
    t.d_pb = (kq_dbgbase*)kq_dev_alloc(r.h, t.plan.max_per_base);
    t.d_ctr = (uint64_t*)kq_dev_alloc(r.h, 3 * sizeof(uint64_t));
    if (!t.d_acc || !t.d_text || !t.d_pb || !t.d_ctr) return fall_back("no device memory");
    return true;
}

void table_passes_range(Run& r, TablePasses& t, int lo, int hi) {
    kq_handle* h = r.h;
    for (const TableGroup& g : t.plan.groups) {
        double t0 = now_s();
        kq_or_die(kq_copy_async(h, t.d_text, r.genome.text.data() + g.text_off, g.text_len, KQ_COPY_TO_DEVICE));
        kq_or_die(kq_lookup_sequence_dev(h, t.d_text, g.text_len, r.ui.covCutOff, (uint16_t)lo, (uint16_t)hi, t.d_pb, t.d_ctr));
        if (t.trace) { kq_or_die(kq_sync(h)); t.t_lookup += now_s() - t0; t0 = now_s(); }      // (the steps are asynchronous: a trace waits to tell them apart)
        kq_or_die(kq_per_base_merge_dev(h, t.d_pb, g.seg_start.data(), g.seg_len.data(), g.seg_start.size(), t.d_acc + 3 * g.first_triple));
        if (t.trace) { kq_or_die(kq_sync(h)); t.t_merge += now_s() - t0; }
    }
    ++t.n_ranges;
}

void table_passes_write(Run& r, TablePasses& t) {
    verbose("per-base table written by the device formatter");
    if (r.plan.table_gz) verbose("per-base table compressed by the device deflater");
    verbose("per-base table accumulated on the device over " + std::to_string(t.n_ranges) + " map ranges in " + std::to_string(t.plan.groups.size()) + " calls");
    kq_handle* h = r.h;
    uint64_t ctr[3] = {0, 0, 0};
    kq_or_die(kq_copy_async(h, ctr, t.d_ctr, sizeof ctr, KQ_COPY_TO_HOST));
    kq_or_die(kq_sync(h));
    for (int i = 0; i < 3; ++i) r.counters[i] += ctr[i];
    kq_dev_free(h, t.d_text); kq_dev_free(h, t.d_pb); kq_dev_free(h, t.d_ctr);       // (room for the formatter's text)
    t.d_text = nullptr; t.d_pb = nullptr; t.d_ctr = nullptr;
    uint64_t bytes = 0, gz_bytes = 0;
    double t_format = 0, t_copy = 0, t_write = 0, t_deflate = 0;
    {
        DeviceTableFile file(r, t.segs);
        for (const TableGroup& g : t.plan.groups) file.write_call(g.lo, g.hi, t.d_acc + 3 * g.first_triple, g.n_triples);
        file.finish();
        bytes = r.plan.table_gz ? file.text_bytes : file.out.bytes; gz_bytes = file.out.bytes; t_format = file.t_format; t_copy = file.t_copy; t_write = file.out.t_write; t_deflate = file.t_deflate;
    }
    table_passes_free(r, t);
    if (t.trace) {
        fprintf(stderr, "[table] device passes: lookup %.3f s, merge %.3f s, format %.3f s, copy %.3f s, write %.3f s, %llu bytes, %d map ranges, %llu calls",
                t.t_lookup, t.t_merge, t_format, t_copy, t_write, (unsigned long long)bytes, t.n_ranges, (unsigned long long)t.plan.groups.size());
        if (r.plan.table_gz) fprintf(stderr, ", deflate %.3f s, %llu compressed bytes", t_deflate, (unsigned long long)gz_bytes);
        fprintf(stderr, "\n");
    }
}

void write_per_base_host(const Run& r) {
    verbose("per-base table written by the host writer");
    const double t0 = now_s();
    const SegmentLists segs = all_segments(r.seqs);
    const std::string& format = r.plan.table_format();
    if (format == "bkwig") write_bkwig(r, segs);
    else {
        std::ofstream file(r.ui.outFile, std::ios::trunc | std::ios::out | std::ios::binary);
        if (r.plan.table_gz) {                                       // the same text, through zlib into BGZF members
            verbose("per-base table compressed by the host (zlib)");
            BgzfBuf gz(file);
            std::ostream ofs(&gz);
            if (format == "kwig") write_kwig(r, segs, ofs, &gz); else write_table(r, segs, ofs);
            if (!gz.finish()) die("Error: cannot write " + r.ui.outFile);
        } else if (format == "kwig") write_kwig(r, segs, file, nullptr);
        else write_table(r, segs, file);
    }
    if (env_flag("KQ_TABLE_TRACE")) fprintf(stderr, "[table] host: write %.3f s\n", now_s() - t0);
}

}  // namespace kqhost
