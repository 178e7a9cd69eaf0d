// Candidate-error search of `kreeq validate -o vcf` (reference DBG::correctSequences / DBGtoVariants / searchVariants,
// src/variants.cpp:40-310) on top of the GPU table.
//
// Division of labour: the device answers "is this k-mer in the graph, and does the graph branch away from the sequence
// here?" for every position of the assembly in one pass (kq_branch_scan), so the bounded graph search -- pointer chasing,
// serial per source k-mer -- runs on the host only at the few positions where it can find something.  The searches of a
// batch advance in lockstep: each runs until it needs graph nodes that are not cached, the needed keys of all of them go
// to the device in ONE kq_lookup_keys call, and they resume.  Visiting order, distances, path reconstruction and the
// variant typing follow the reference statement by statement (line numbers cited below), including the order in which
// its Fibonacci heap (include/fibonacci-heap.h) hands out nodes of equal key.
//
// The VCF text is written by gfalibs' Report class in the reference, which is absent from the reference tree; the record
// layout here is inferred from its one golden file (validateFiles/test.50.tst) and documented at vcf_record().
#include "variants.h"

#include "cli_common.h"
#include "cli_plan.h"
#include "graph_search.h"

#include <algorithm>
#include <deque>
#include <stdexcept>
#include <thread>
#include <tuple>

namespace kqhost {

namespace {

struct Node { uint32_t fw[4], bw[4]; bool present; };

struct Search {
    // what DBGtoVariants hands to searchVariants (:136)
    uint64_t seg_id = 0, c = 0, source = 0, ref = 0;
    bool source_fw = false, has_ref = false;
    std::vector<uint64_t> targets_queue;
    std::vector<uint64_t> targets;                                       // targetsMap: at most maxSpan keys, sorted
    bool is_target(uint64_t key) const { return std::binary_search(targets.begin(), targets.end(), key); }
    // searchVariants' locals (:173-185)
    NodeQueue Q;
    FlatMap<uint8_t> dist;
    FlatMap<std::pair<uint64_t, bool>> prev;
    std::vector<uint64_t> destinations;
    int depth = 0;
    bool direction = true, started = false, done = false;
    // the node being expanded
    uint64_t u = 0;
    std::vector<std::tuple<uint64_t, bool, bool>> cand;
    bool have_u = false;
    std::vector<DbgPath> paths;
};

using Cache = FlatMap<Node>;

// Runs one search until it needs uncached nodes (their keys are appended to `want`) or is finished.
void advance(Search& s, const Cache& cache, int k, int kmer_depth, uint32_t cov_cutoff, std::vector<uint64_t>& want) {
    if (s.done) return;
    if (!s.started) {
        if (!cache.count(s.source)) { want.push_back(s.source); return; }
        s.dist[s.source] = 1;                                            // :180-181
        s.Q.insert(s.source, 1);
        s.started = true;
    }
    for (;;) {
        if (!s.have_u) {
            if (!(s.Q.size() > 0 && s.depth < kmer_depth + 1)) break;   // :187
            s.u = s.Q.extract_min();                                     // :192
            const auto* got = s.prev.find(s.u);                          // :193-196
            if (got) s.direction = got->second;
            const Node& nu = *cache.find(s.u);
            s.cand.clear();
            for (int i = 0; i < 4; ++i) {                                // :232-246
                if (s.depth == 0) s.direction = s.source_fw;
                // `direction ? fw[i] : bw[i] > covCutOff` == direction ? (fw[i] != 0) : (bw[i] > covCutOff)   (:237)
                const bool edge = s.direction ? nu.fw[i] != 0 : nu.bw[i] > cov_cutoff;
                if (!edge) continue;
                bool is_fw = false;
                const uint64_t key = next_key(s.u, i, s.direction, k, &is_fw);
                if (s.has_ref && key == s.ref) continue;                 // :241: the reference path is never rediscovered
                s.cand.emplace_back(key, is_fw, s.direction);
            }
            s.have_u = true;
        }
        bool missing = false;
        for (auto& cnd : s.cand) {
            const uint64_t key = std::get<0>(cnd);
            if (!s.is_target(key) && !cache.count(key)) { want.push_back(key); missing = true; }
        }
        if (missing) return;                                             // resumed after the batch lookup
        size_t explored_count = 0;
        for (auto& cnd : s.cand) {                                       // :247-260 with checkNext :197-228
            const uint64_t key = std::get<0>(cnd);
            const bool dirn = std::get<2>(cnd), cont = std::get<1>(cnd) ? dirn : !dirn;
            if (!s.is_target(key)) {
                uint8_t alt = s.dist[s.u];
                if (alt < 255) ++alt;
                if (!s.dist.count(key)) { s.dist[key] = 255; s.Q.insert(key, 0); }
                if (alt < s.dist[key]) { s.prev[key] = std::make_pair(s.u, cont); s.dist[key] = alt; }
            }
            ++explored_count;
            if (s.is_target(key)) { s.prev[key] = std::make_pair(s.u, dirn); s.destinations.push_back(key); }
        }
        (void)explored_count;                                            // every candidate is reachable (one map range): edgeCount == exploredCount
        ++s.depth;                                                       // :261
        s.have_u = false;
    }
    // paths from the destinations back to the source (:266-303)
    auto prev_of = [&](uint64_t key) { const auto* it = s.prev.find(key); return it ? *it : std::make_pair((uint64_t)0, false); };
    for (uint64_t dest : s.destinations) {
        DbgPath path;
        path.pos = s.c + (uint64_t)k;                                    // :139-140
        const auto where = std::find(s.targets_queue.begin(), s.targets_queue.end(), dest);
        const int ref_len = (int)(where - s.targets_queue.begin()) + k;
        int i = 0;
        uint64_t node = prev_of(dest).first;
        while (node != s.source) { node = prev_of(node).first; ++i; }
        node = prev_of(dest).first;
        bool dirn = prev_of(node).second;
        int b = i - ref_len;
        if (ref_len > k) { path.type = VAR_COM; path.ref_len = (uint32_t)(ref_len - k + 1); b = ref_len - k; }
        else if (i == ref_len) path.type = VAR_SNV;
        else if (i > ref_len) { path.type = VAR_DEL; --b; node = prev_of(node).first; dirn = prev_of(node).second; }
        else path.type = VAR_INS;
        while (b >= 0) {
            const std::string str = reverse_hash(node, k);
            path.sequence.push_back(dirn ? str[0] : rev_com(str[(size_t)k - 1]));
            node = prev_of(node).first;
            dirn = prev_of(node).second;
            --b;
        }
        std::reverse(path.sequence.begin(), path.sequence.end());
        s.paths.push_back(std::move(path));
    }
    s.done = true;
    // only the paths are read from here on
    s.dist.release(); s.prev.release(); s.Q = NodeQueue();
    std::vector<uint64_t>().swap(s.targets_queue); std::vector<uint64_t>().swap(s.targets); std::vector<uint64_t>().swap(s.destinations);
}

}  // namespace

GraphSource graph_of_handle(kq_handle* h) {
    GraphSource g;
    g.branch_scan = [h](const std::string& joined, uint32_t cov_cutoff, std::vector<uint8_t>& flags) {
        if (kq_branch_scan(h, joined.data(), joined.size(), cov_cutoff, flags.data()) != KQ_OK) throw std::runtime_error(std::string("Error: ") + kq_last_error());
    };
    g.lookup = [h](const std::vector<uint64_t>& want, std::vector<kq_entry>& got) {
        if (kq_lookup_keys(h, want.data(), want.size(), got.data()) != KQ_OK) throw std::runtime_error(std::string("Error: ") + kq_last_error());
    };
    g.resident = h;
    return g;
}

namespace {

// The searches of seqs[lo, hi) in one kq_search_variants call over their joined text -> sites appended to `out`
void device_call(kq_handle* h, const std::vector<SeqRecord>& seqs, size_t lo, size_t hi, int kmer_depth, int max_span, uint32_t cov_cutoff,
                 std::vector<kq_variant_path>& paths, std::vector<char>& bases, std::vector<VariantSite>& out, uint64_t& n_calls) {
    const auto [joined, offset] = join_sequences(seqs, lo, hi);
    uint64_t n_paths = 0, n_seq = 0;
    int rc = kq_search_variants(h, joined.data(), joined.size(), kmer_depth, max_span, cov_cutoff, paths.data(), paths.size(), &n_paths, bases.data(), bases.size(), &n_seq);
    ++n_calls;
    if (rc == KQ_ERR_CAPACITY) {                                         // once more with the sizes it reported (the searches run again)
        paths.resize((size_t)n_paths); bases.resize((size_t)n_seq);
        rc = kq_search_variants(h, joined.data(), joined.size(), kmer_depth, max_span, cov_cutoff, paths.data(), paths.size(), &n_paths, bases.data(), bases.size(), &n_seq);
        ++n_calls;
    }
    if (rc != KQ_OK) throw std::runtime_error(std::string("Error: ") + kq_last_error());
    for (uint64_t i = 0; i < n_paths; ++i) {
        const kq_variant_path& r = paths[(size_t)i];
        if (i == 0 || r.pos != paths[(size_t)i - 1].pos) {               // the paths of one position are one site
            const size_t si = (size_t)(std::upper_bound(offset.begin(), offset.end(), r.seg_start) - offset.begin()) - 1;
            VariantSite v;
            v.seq_index = lo + si;
            v.seg_start = r.seg_start - offset[si];
            out.push_back(std::move(v));
        }
        DbgPath p;
        p.type = (VariantType)r.type;                                    // KQ_VAR_* == VariantType
        p.pos = r.pos - r.seg_start;
        p.sequence.assign(bases.data() + r.seq_off, r.seq_len);
        p.ref_len = r.ref_len;
        out.back().paths.push_back(std::move(p));
    }
}

std::vector<VariantSite> find_candidate_errors_device(kq_handle* h, const std::vector<SeqRecord>& seqs, int kmer_depth, int max_span, uint32_t cov_cutoff,
                                                      const std::function<void(const std::string&)>& log) {
    static_assert((int)VAR_SNV == KQ_VAR_SNV && (int)VAR_INS == KQ_VAR_INS && (int)VAR_DEL == KQ_VAR_DEL && (int)VAR_COM == KQ_VAR_COM, "path types");
    const double t0 = now_s();
    std::vector<VariantSite> out;
    std::vector<kq_variant_path> paths(1 << 16);                         // modest caps; a call that needs more says how much
    std::vector<char> bases(1 << 22);
    uint64_t n_calls = 0, n_records = 0;
    for (size_t lo = 0, hi; lo < seqs.size(); lo = hi) {                 // whole sequences, at most kDeviceCallBytes of joined text per call
        hi = next_call(seqs, lo, kDeviceCallBytes);
        device_call(h, seqs, lo, hi, kmer_depth, max_span, cov_cutoff, paths, bases, out, n_calls);
    }
    for (auto& v : out) n_records += v.paths.size();
    if (log) log("Device searches: " + std::to_string(n_calls) + " calls, " + std::to_string(out.size()) + " sites, " + std::to_string(n_records) + " paths; " +
                 std::to_string(now_s() - t0) + " s");
    return out;
}

}  // namespace

std::vector<VariantSite> find_candidate_errors(const GraphSource& g, int k, const std::vector<SeqRecord>& seqs, int kmer_depth, int max_span,
                                               uint32_t cov_cutoff, const std::function<void(const std::string&)>& log) {
    if (env_flag("KQ_VCF_DEVICE")) {                                     // the searches run on the GPU, one per lane (kq_search_variants); off by default
        const bool fits = g.resident && kmer_depth >= 0 && kmer_depth <= kVcfDeviceMaxDepth && max_span >= kVcfDeviceMinSpan && max_span <= kVcfDeviceMaxSpan &&
                          all_fit(seqs, kDeviceCallBytes);
        if (fits) {
            if (log) log("candidate-error search ran as the device search");
            return find_candidate_errors_device(g.resident, seqs, kmer_depth, max_span, cov_cutoff, log);
        }
    }
    if (log) log("candidate-error search ran as the host search");
    // 1. device pre-filter over the whole assembly (sequences joined by a non-base byte)
    const auto [joined, offset] = join_sequences(seqs, 0, seqs.size());
    std::vector<uint8_t> flags(joined.size());
    g.branch_scan(joined, cov_cutoff, flags);

    // 2. one Search per flagged position, segment by segment (DBGtoVariants :53-169, single map range)
    std::vector<Search> searches;
    std::vector<std::tuple<size_t, uint64_t>> seg_of;                    // segment id -> (sequence index, start inside the sequence)
    uint64_t n_pos = 0;
    for (size_t si = 0; si < seqs.size(); ++si) {
        const std::string& seq = seqs[si].seq;
        for (auto& seg : segments_of(seq)) {
            const uint64_t i = seg.first, len = seg.second;
            if (len >= (uint64_t)k) {
                const uint64_t kcount = len - k + 1;
                std::vector<uint8_t> str(len);
                for (uint64_t p = 0; p < len; ++p) str[p] = (uint8_t)ctoi(seq[i + p]);
                const uint64_t seg_id = seg_of.size();
                seg_of.emplace_back(si, i);
                std::vector<uint64_t> seg_keys;                          // canonical key of every k-mer of the segment (filled on first use)
                auto fill_keys = [&] { if (seg_keys.empty()) { seg_keys.resize(kcount); for (uint64_t t = 0; t < kcount; ++t) seg_keys[t] = hash_kmer(str.data() + t, k, nullptr); } };
                const uint8_t* f = flags.data() + offset[si] + i;
                n_pos += kcount;
                for (uint64_t c = 0; c < kcount; ++c) {
                    if ((f[c] & 3) != 3) continue;                       // absent (:149-152) or no candidate at the source: nothing to find
                    fill_keys();
                    Search s;
                    s.seg_id = seg_id; s.c = c;
                    s.source = hash_kmer(str.data() + c, k, &s.source_fw);       // :114; isFw of k-mer c is what :136 passes on
                    if (c + 1 < kcount) { s.ref = hash_kmer(str.data() + c + 1, k, nullptr); s.has_ref = true; }
                    // the targets while c is processed: the k-mers starting at c+k+1 .. c+k+maxSpan (:92-110).  targetsMap
                    // loses a key when ANY occurrence of it leaves the window (:104) and gets it back with the next push
                    // (:108): a key is in the map iff no occurrence left after its latest one entered
                    const uint64_t w_lo = c + k + 1, w_hi = std::min<uint64_t>(c + k + (uint64_t)max_span, kcount - 1);
                    for (uint64_t t = w_lo; t <= w_hi; ++t) s.targets_queue.push_back(seg_keys[t]);
                    for (uint64_t t = w_lo; t <= w_hi; ++t) {
                        const uint64_t key = seg_keys[t];
                        uint64_t t_max = t;
                        for (uint64_t t2 = t + 1; t2 <= w_hi; ++t2) if (seg_keys[t2] == key) t_max = t2;
                        bool erased = false;                             // an occurrence popped at or after the push of t_max
                        const uint64_t from = t_max >= (uint64_t)max_span ? t_max - (uint64_t)max_span + 1 : 0;
                        for (uint64_t t1 = std::max<uint64_t>(from, (uint64_t)k); t1 <= c + k && !erased; ++t1) erased = seg_keys[t1] == key;
                        if (!erased) s.targets.push_back(key);
                    }
                    std::sort(s.targets.begin(), s.targets.end());
                    s.targets.erase(std::unique(s.targets.begin(), s.targets.end()), s.targets.end());
                    searches.push_back(std::move(s));
                }
            }
        }
    }
    if (log) log("Candidate positions after the device pre-filter: " + std::to_string(searches.size()) + " of " + std::to_string(n_pos));
    double t_adv = 0, t_sort = 0, t_look = 0, t_cache = 0;
    size_t n_rounds = 0, n_keys = 0;

    // 3. lockstep rounds: advance every search, fetch what they ask for in one batch
    Cache cache;
    std::vector<uint64_t> want;
    std::vector<kq_entry> got;
    const size_t kBatch = 1 << 16;
    for (size_t lo = 0; lo < searches.size(); lo += kBatch) {
        const size_t hi = std::min(searches.size(), lo + kBatch);
        for (;;) {
            want.clear();
            bool any = false;
            // the searches of a round are independent (each reads the cache and its own state): a few host threads share
            // them when there are enough (HiFi-scale inputs flag tens of thousands of positions per batch)
            const size_t n_live = hi - lo;
            double t0 = now_s();
            unsigned n_thr = std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
            if (n_live < 512) n_thr = 1;
            if (n_thr > 1) {
                std::vector<std::vector<uint64_t>> wants(n_thr);
                std::vector<std::thread> pool;
                for (unsigned t = 0; t < n_thr; ++t)
                    pool.emplace_back([&, t] {
                        const size_t a = lo + n_live * t / n_thr, b = lo + n_live * (t + 1) / n_thr;
                        for (size_t i = a; i < b; ++i) if (!searches[i].done) advance(searches[i], cache, k, kmer_depth, cov_cutoff, wants[t]);
                    });
                for (auto& th : pool) th.join();
                for (auto& w : wants) want.insert(want.end(), w.begin(), w.end());
            } else {
                for (size_t i = lo; i < hi; ++i) if (!searches[i].done) advance(searches[i], cache, k, kmer_depth, cov_cutoff, want);
            }
            for (size_t i = lo; i < hi && !any; ++i) any = !searches[i].done;
            t_adv += now_s() - t0; t0 = now_s();
            if (!any) break;
            std::sort(want.begin(), want.end());
            want.erase(std::unique(want.begin(), want.end()), want.end());
            if (want.empty()) throw std::runtime_error("candidate-error search stalled");
            t_sort += now_s() - t0; t0 = now_s();
            got.resize(want.size());
            g.lookup(want, got);
            t_look += now_s() - t0; t0 = now_s();
            cache.reserve(cache.size() + got.size());
            for (auto& e : got) {
                Node& n = cache[e.key];
                for (int w = 0; w < 4; ++w) { n.fw[w] = e.fw[w]; n.bw[w] = e.bw[w]; }
                n.present = e.cov != 0;
            }
            t_cache += now_s() - t0;
            ++n_rounds; n_keys += want.size();
        }
        if (cache.size() > (1u << 24)) cache.clear();                    // bounded memory on large assemblies
    }

    if (log) log("Search rounds: " + std::to_string(n_rounds) + ", keys fetched " + std::to_string(n_keys) + "; advance " + std::to_string(t_adv) + " s, sort " + std::to_string(t_sort) +
                 " s, lookup " + std::to_string(t_look) + " s, cache " + std::to_string(t_cache) + " s");
    // 4. sites in sequence / position order
    std::vector<VariantSite> out;
    for (auto& s : searches) {
        if (s.paths.empty()) continue;
        VariantSite v;
        v.seq_index = std::get<0>(seg_of[s.seg_id]);
        v.seg_start = std::get<1>(seg_of[s.seg_id]);
        v.paths = std::move(s.paths);
        out.push_back(std::move(v));
    }
    return out;
}

// One VCF record per path.  Layout inferred from validateFiles/test.50.tst:7-37 (the writer is gfalibs' Report):
//   SNV / COM : POS = pos + 1, REF = the refLen (1 for SNV) original bases from pos, ALT = the path's bases
//   INS / DEL : the base in front anchors the record: POS = pos, REF = anchor + base at pos,
//               ALT = anchor + the path's bases (+ the base at pos for DEL: it stays)
// QUAL 0, FILTER PASS, genotype 1/1 with quality 0, exactly as the golden prints them.
std::vector<std::string> vcf_lines(const std::vector<SeqRecord>& seqs, const std::vector<VariantSite>& sites) {
    std::vector<std::string> out = {"##fileformat=VCFv4.2",
                                    "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">",
                                    "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype Quality\">",
                                    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE"};
    for (auto& site : sites) {
        const SeqRecord& r = seqs[site.seq_index];
        for (auto& p : site.paths) {
            const uint64_t pos = site.seg_start + p.pos;
            uint64_t vpos;
            std::string ref, alt;
            if (p.type == VAR_SNV || p.type == VAR_COM) {
                const uint64_t n = p.type == VAR_COM ? p.ref_len : 1;
                vpos = pos + 1; ref = r.seq.substr(pos, n); alt = p.sequence;
            } else {
                const char anchor = r.seq[pos - 1];
                vpos = pos;
                ref = std::string(1, anchor) + r.seq[pos];
                alt = std::string(1, anchor) + p.sequence + (p.type == VAR_DEL ? std::string(1, r.seq[pos]) : std::string());
            }
            out.push_back(r.header + "\t" + std::to_string(vpos) + "\t.\t" + ref + "\t" + alt + "\t0\tPASS\t.\tGT:GQ\t1/1:0");
        }
    }
    return out;
}

}  // namespace kqhost
