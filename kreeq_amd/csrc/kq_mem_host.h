// kq_mem_host.h -- scoped owners of what the host side of the ABI takes from the HIP runtime: device memory, pinned memory,
// events, streams, and the device allocations of one call.  One rule: a resource is freed by the scope or the handle that
// holds it.  All owners are move-only (a move leaves the source empty); no destructor reports an error.
// Host only; includes nothing from HIP: whoever includes this has declared the runtime calls it uses (kreeq_amd.hip through
// <hip/hip_runtime.h>, tests/native/mem_owner_main.cpp through counting stand-ins).
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace kq {

// Pointer + byte count of one runtime allocation; Alloc / Free are the runtime's pair for that kind of memory.
template <class Ops>
class MemOwner {
    void* p_ = nullptr;
    size_t bytes_ = 0;
public:
    MemOwner() = default;
    MemOwner(const MemOwner&) = delete;
    MemOwner& operator=(const MemOwner&) = delete;
    MemOwner(MemOwner&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    MemOwner& operator=(MemOwner&& o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~MemOwner() { reset(); }
    void swap(MemOwner& o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); }
    friend void swap(MemOwner& a, MemOwner& b) noexcept { a.swap(b); }

    void reset() { if (p_) (void)Ops::release(p_); p_ = nullptr; bytes_ = 0; }
    // exactly `bytes`; what was held goes first.  On failure the owner is empty
    hipError_t alloc(size_t bytes) {
        reset();
        hipError_t e = Ops::take(&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        bytes_ = bytes;
        return hipSuccess;
    }
    // at least `need`: geometric growth for small buffers, bounded slack for multi-GB ones.  The old block is freed BEFORE the
    // new one is taken (the peak is one block, not two)
    hipError_t ensure(size_t need) {
        if (bytes_ >= need) return hipSuccess;
        return alloc(need + std::min<size_t>(need / 4, (size_t)256 << 20) + 4096);
    }
    void* get() const { return p_; }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
    template <class T> T* as() const { return static_cast<T*>(p_); }
};
struct DevOps {
    static hipError_t take(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t release(void* p) { return hipFree(p); }
};
struct PinnedOps {
    static hipError_t take(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t release(void* p) { return hipHostFree(p); }
};
using DevMem = MemOwner<DevOps>;          // hipMalloc / hipFree
using PinnedMem = MemOwner<PinnedOps>;    // hipHostMalloc / hipHostFree

// An event, created on demand with the caller's flags
class Event {
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); std::swap(e_, o.e_); } return *this; }
    ~Event() { reset(); }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    hipError_t create(unsigned flags) {
        reset();
        hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
    hipEvent_t get() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }
};
class Stream {
    hipStream_t s_ = nullptr;
public:
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); std::swap(s_, o.s_); } return *this; }
    ~Stream() { reset(); }
    void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
    hipError_t create(unsigned flags) {
        reset();
        hipError_t e = hipStreamCreateWithFlags(&s_, flags);
        if (e != hipSuccess) s_ = nullptr;
        return e;
    }
    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }
};

// device allocations of one call, freed on every way out
struct DevScope {
    std::vector<void*> v;
    DevScope() = default;
    DevScope(const DevScope&) = delete;
    DevScope& operator=(const DevScope&) = delete;
    DevScope(DevScope&& o) noexcept : v(std::move(o.v)) { o.v.clear(); }
    DevScope& operator=(DevScope&& o) noexcept { if (this != &o) { clear(); v = std::move(o.v); o.v.clear(); } return *this; }
    ~DevScope() { clear(); }
    void clear() { for (void* p : v) if (p) (void)hipFree(p); v.clear(); }
    hipError_t alloc(void** p, size_t bytes) {
        *p = nullptr;
        v.reserve(v.size() + 1);         // (no host allocation between taking the block and recording it)
        hipError_t e = hipMalloc(p, bytes ? bytes : 8);
        if (e == hipSuccess) v.push_back(*p); else { *p = nullptr; (void)hipGetLastError(); }
        return e;
    }
    void release(void* p) { if (p) for (void*& q : v) if (q == p) { (void)hipFree(q); q = nullptr; } }
};

}  // namespace kq
