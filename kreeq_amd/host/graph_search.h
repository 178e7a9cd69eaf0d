// Building blocks of the host-side graph searches (the candidate-error search of variants.cpp and the best-first search of
// subgraph.cpp): k-mer key arithmetic, a flat u64 map and the reference's Fibonacci heap.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace kqhost {

constexpr char kItoc[4] = {'A', 'C', 'G', 'T'};
inline int ctoi(char c) {
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; }
}
inline char rev_com(char c) { return kItoc[3 - ctoi(c)]; }

// gfalibs Kmap::hash: canonical 2-bit key of k base codes, first base in the low bits
inline uint64_t hash_kmer(const uint8_t* b, int k, bool* is_fw) {
    uint64_t fw = 0, rv = 0;
    for (int c = 0; c < k; ++c) { fw |= (uint64_t)b[c] << (2 * c); rv |= (uint64_t)(3 - b[c]) << (2 * (k - 1 - c)); }
    if (is_fw) *is_fw = fw < rv;
    return fw < rv ? fw : rv;
}
inline std::string reverse_hash(uint64_t key, int k) {
    std::string s((size_t)k, 'A');
    for (int c = 0; c < k; ++c) s[(size_t)c] = kItoc[(key >> (2 * c)) & 3];
    return s;
}
// DBG::buildNextKmer, src/subgraph.cpp:581-598: the k-mer one step along edge `base` of the canonical string of `key`
inline uint64_t next_key(uint64_t key, int base, bool fw, int k, bool* is_fw) {
    uint8_t codes[33];
    if (fw) { for (int c = 0; c + 1 < k; ++c) codes[c] = (uint8_t)((key >> (2 * (c + 1))) & 3); codes[k - 1] = (uint8_t)base; }
    else    { codes[0] = (uint8_t)base; for (int c = 1; c < k; ++c) codes[c] = (uint8_t)((key >> (2 * (c - 1))) & 3); }
    return hash_kmer(codes, k, is_fw);
}

// u64 -> T with open addressing (linear probing, power-of-two capacity, grown at load 1/2; no allocation before the first insert).
// The search never iterates over its maps, so any container with find / insert gives the reference's result; the node-based
// std::unordered_map cost 0.5 us per cached graph node and as much again to destroy (100 x the HiFi test: 5.7 of 9 s).
template <class T>
class FlatMap {
    std::vector<uint64_t> keys_;
    std::vector<T> vals_;
    std::vector<uint8_t> used_;
    size_t n_ = 0;
    static size_t mix(uint64_t k) { k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 29; return (size_t)k; }
    size_t slot(uint64_t k) const {                                     // the key's slot, or the free slot where it would go
        size_t i = mix(k) & (keys_.size() - 1);
        while (used_[i] && keys_[i] != k) i = (i + 1) & (keys_.size() - 1);
        return i;
    }
    void grow() {
        const size_t cap = keys_.empty() ? 16 : keys_.size() * 2;
        std::vector<uint64_t> ok(cap); std::vector<T> ov(cap); std::vector<uint8_t> ou(cap, 0);
        ok.swap(keys_); ov.swap(vals_); ou.swap(used_);
        for (size_t i = 0; i < ok.size(); ++i) if (ou[i]) { const size_t j = slot(ok[i]); keys_[j] = ok[i]; vals_[j] = std::move(ov[i]); used_[j] = 1; }
    }
public:
    size_t size() const { return n_; }
    void reserve(size_t n) { while (keys_.size() < 2 * n) grow(); }
    const T* find(uint64_t k) const { if (keys_.empty()) return nullptr; const size_t i = slot(k); return used_[i] ? &vals_[i] : nullptr; }
    T* find(uint64_t k) { if (keys_.empty()) return nullptr; const size_t i = slot(k); return used_[i] ? &vals_[i] : nullptr; }
    bool count(uint64_t k) const { return find(k) != nullptr; }
    T& operator[](uint64_t k) {                                         // inserts a value-initialised T when absent
        if (2 * (n_ + 1) > keys_.size()) grow();
        const size_t i = slot(k);
        if (!used_[i]) { used_[i] = 1; keys_[i] = k; vals_[i] = T(); ++n_; }
        return vals_[i];
    }
    void clear() { std::fill(used_.begin(), used_.end(), 0); n_ = 0; }
    void release() { std::vector<uint64_t>().swap(keys_); std::vector<T>().swap(vals_); std::vector<uint8_t>().swap(used_); n_ = 0; }
};

// The reference's priority queue, include/fibonacci-heap.h, on an index pool.  The search inserts every node except
// the source with key 0 and its decreaseKey refuses to raise a key (:141), so which of several queued nodes comes out
// next is decided by the shape of the root list alone: insert links a node left of the minimum (:72-80), extractMin
// promotes the children, steps to the right neighbour and consolidates equal degrees (:87-126, :218-268).
class NodeQueue {
    struct N { int degree, parent, child, left, right, key; bool mark; uint64_t obj; };
    std::vector<N> n_;
    std::vector<int> deg_;
    int min_ = -1, count_ = 0;

    void to_root(int x) {                                                // _existingToRoot :145-164
        n_[x].parent = -1; n_[x].mark = false;
        if (min_ >= 0) {
            const int ml = n_[min_].left;
            n_[min_].left = x; n_[x].right = min_; n_[x].left = ml; n_[ml].right = x;
            if (n_[min_].key > n_[x].key) min_ = x;
        } else { min_ = x; n_[x].left = n_[x].right = x; }
    }
    void unlink(int x) {                                                 // _removeNodeFromRoot :165-179
        if (n_[x].right != x) { n_[n_[x].right].left = n_[x].left; n_[n_[x].left].right = n_[x].right; }
        const int p = n_[x].parent;
        if (p >= 0) {
            n_[p].child = n_[p].degree == 1 ? -1 : n_[x].right;
            --n_[p].degree;
        }
    }
    void add_child(int p, int c) {                                       // _addChild :184-201
        if (n_[p].degree == 0) { n_[p].child = c; n_[c].left = n_[c].right = c; }
        else { const int c1 = n_[p].child, l = n_[c1].left; n_[c1].left = c; n_[c].right = c1; n_[c].left = l; n_[l].right = c; }
        n_[c].parent = p; ++n_[p].degree;
    }
    void consolidate() {                                                 // :218-268
        if (count_ <= 1) return;
        deg_.clear();
        int roots = 0, it = min_;
        do { ++roots; it = n_[it].right; } while (it != min_);
        int cur = min_;
        for (int r = 0; r < roots; ++r) {
            int x = cur;
            cur = n_[cur].right;
            int d = n_[x].degree;
            for (;;) {
                while (d >= (int)deg_.size()) deg_.push_back(-1);
                if (deg_[(size_t)d] < 0) { deg_[(size_t)d] = x; break; }
                int y = deg_[(size_t)d];
                if (n_[x].key > n_[y].key) std::swap(x, y);
                if (y == x) break;
                unlink(y); add_child(x, y); n_[y].mark = false;          // _link
                deg_[(size_t)d] = -1;
                ++d;
            }
        }
        min_ = -1;
        for (int x : deg_) if (x >= 0) to_root(x);
    }
public:
    int size() const { return count_; }
    void insert(uint64_t obj, int key) {                                 // :57-86
        const int x = (int)n_.size();
        n_.push_back(N{0, -1, -1, x, x, key, false, obj});
        if (min_ >= 0) { const int ml = n_[min_].left; n_[min_].left = x; n_[x].right = min_; n_[x].left = ml; n_[ml].right = x; }
        if (min_ < 0 || n_[min_].key > key) min_ = x;
        ++count_;
    }
    uint64_t extract_min() {                                             // :87-126
        const int m = min_;
        int c = n_[m].child;
        for (int i = 0, d = n_[m].degree; i < d; ++i) { const int rem = c; c = n_[c].right; to_root(rem); }
        unlink(m);
        --count_;
        if (count_ == 0) min_ = -1;
        else {
            min_ = n_[m].right;
            const int ml = n_[m].left;
            n_[min_].left = ml; n_[ml].right = min_;
            consolidate();
        }
        return n_[m].obj;
    }
    // decreaseKey (:127-142) only ever sees new keys >= 1 for nodes inserted with key 0 here: it returns at :141
};

}  // namespace kqhost
