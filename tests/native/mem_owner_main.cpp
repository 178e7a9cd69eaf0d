// Stand-alone check of the scoped owners (kreeq_amd/csrc/kq_mem_host.h), meant to be built with
// -fsanitize=address,undefined.  The runtime calls the header uses are counting stand-ins on the host heap (device and pinned
// memory = malloc / free, events and streams = small heap objects), and one global makes the n-th allocation fail: the
// sanitizer's leak and double-free checks therefore check the owners themselves.  Every scenario ends with nothing live.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

// ---- the stand-ins --------------------------------------------------------------------------------------------------
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
struct FakeEvent { unsigned flags; };
struct FakeStream { unsigned flags; };
typedef FakeEvent* hipEvent_t;
typedef FakeStream* hipStream_t;
constexpr unsigned hipHostMallocDefault = 0, hipEventDisableTiming = 2, hipStreamNonBlocking = 1;

static long n_alloc = 0, n_free = 0;            // successful allocations of any kind / frees of any kind
static long fail_at = 0;                        // fail the n-th allocation from now (1 = the next one); 0: none
static size_t last_bytes = 0;                   // size of the last allocation asked for
static std::vector<char> order;                 // 'a' / 'f' in the order of the calls
static int last_error_reads = 0;

static hipError_t take(void** p, size_t bytes) {
    last_bytes = bytes;
    if (fail_at && --fail_at == 0) { *p = (void*)0x1; return hipErrorOutOfMemory; }      // (a failed call may leave garbage behind)
    *p = malloc(bytes);
    ++n_alloc; order.push_back('a');
    return hipSuccess;
}
static hipError_t give(void* p) { free(p); ++n_free; order.push_back('f'); return hipSuccess; }
static hipError_t hipMalloc(void** p, size_t bytes) { return take(p, bytes); }
static hipError_t hipFree(void* p) { return give(p); }
static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return take(p, bytes); }
static hipError_t hipHostFree(void* p) { return give(p); }
static hipError_t hipGetLastError() { ++last_error_reads; return hipSuccess; }
static hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
    if (fail_at && --fail_at == 0) return hipErrorOutOfMemory;
    *e = new FakeEvent{flags}; ++n_alloc; return hipSuccess;
}
static hipError_t hipEventDestroy(hipEvent_t e) { delete e; ++n_free; return hipSuccess; }
static hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
    if (fail_at && --fail_at == 0) return hipErrorOutOfMemory;
    *s = new FakeStream{flags}; ++n_alloc; return hipSuccess;
}
static hipError_t hipStreamDestroy(hipStream_t s) { delete s; ++n_free; return hipSuccess; }

#include "kq_mem_host.h"

using namespace kq;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++bad; } } while (0)
static long live() { return n_alloc - n_free; }
static size_t grown(size_t need) { return need + std::min<size_t>(need / 4, (size_t)256 << 20) + 4096; }

// the ScratchSet case: a struct of owners, swapped with std::swap
struct Pair { DevMem a; PinnedMem b; Event e; };
// the hist_cache case: a vector of structs that own a DevMem
struct Entry { int key; DevMem m; };

template <class Mem> static void ensure_cases() {
    {
        Mem m;
        CHECK(!m && m.get() == nullptr && m.bytes() == 0);
        CHECK(m.ensure(1000) == hipSuccess);
        CHECK(m && m.bytes() == grown(1000) && last_bytes == grown(1000) && grown(1000) == 1000 + 250 + 4096);
        void* p = m.get();
        const long a0 = n_alloc;
        CHECK(m.ensure(10) == hipSuccess && m.get() == p);                       // below
        CHECK(m.ensure(grown(1000)) == hipSuccess && m.get() == p);              // at
        CHECK(n_alloc == a0);
        order.clear();
        CHECK(m.ensure(grown(1000) + 1) == hipSuccess);                          // above: free, then allocate
        CHECK(order.size() == 2 && order[0] == 'f' && order[1] == 'a');
        CHECK(m.bytes() == grown(grown(1000) + 1) && last_bytes == m.bytes());
        CHECK(live() == 1);
        order.clear();
        CHECK(m.alloc(64) == hipSuccess && m.bytes() == 64 && last_bytes == 64);  // exact size, the old block first
        CHECK(order.size() == 2 && order[0] == 'f' && order[1] == 'a');
        m.template as<char>()[63] = 1;
        // the slack of a multi-GB request is bounded (no allocation: the next one fails)
        fail_at = 1;
        CHECK(m.ensure((size_t)8 << 30) == hipErrorOutOfMemory);
        CHECK(last_bytes == ((size_t)8 << 30) + ((size_t)256 << 20) + 4096);
        CHECK(!m && m.get() == nullptr && m.bytes() == 0);                       // a failed ensure: empty, the old block gone
        CHECK(live() == 0);
        m.reset();                                                               // (reset of an empty owner: nothing)
        CHECK(m.ensure(0) == hipSuccess && !m);                                  // nothing needed, nothing taken
    }
    CHECK(live() == 0);
}

static hipError_t scope_early_return() {
    DevScope mem;
    void *a, *b, *c;
    hipError_t e;
    if ((e = mem.alloc(&a, 16)) != hipSuccess) return e;
    if ((e = mem.alloc(&b, 16)) != hipSuccess) return e;
    fail_at = 1;
    if ((e = mem.alloc(&c, 16)) != hipSuccess) { CHECK(c == nullptr && mem.v.size() == 2); return e; }
    CHECK(false);
    return hipSuccess;
}

int main() {
    ensure_cases<DevMem>();
    ensure_cases<PinnedMem>();
    CHECK(n_alloc == n_free);

    // moves and swaps
    {
        DevMem a;
        CHECK(a.alloc(100) == hipSuccess);
        void* pa = a.get();
        DevMem b(std::move(a));                                                  // move construction
        CHECK(!a && a.bytes() == 0 && b.get() == pa && b.bytes() == 100);
        DevMem c;
        CHECK(c.alloc(200) == hipSuccess);
        const long f0 = n_free;
        c = std::move(b);                                                        // move assignment onto a full owner
        CHECK(n_free == f0 + 1 && c.get() == pa && c.bytes() == 100 && !b && b.bytes() == 0);
        c.swap(c);                                                               // self-swap
        swap(c, c);
        CHECK(c.get() == pa && c.bytes() == 100 && live() == 1);
        DevMem& same = c;
        c = std::move(same);                                                     // self-assignment
        CHECK(c.get() == pa && live() == 1);
        a = std::move(b);                                                        // empty onto empty
        CHECK(!a && !b);
    }
    CHECK(live() == 0);
    {
        Pair x, y;
        CHECK(x.a.alloc(10) == hipSuccess && x.b.alloc(20) == hipSuccess && x.e.create(hipEventDisableTiming) == hipSuccess);
        CHECK(y.a.alloc(30) == hipSuccess);
        void *xa = x.a.get(), *xb = x.b.get(), *ya = y.a.get();
        hipEvent_t xe = x.e.get();
        const long a0 = n_alloc, f0 = n_free;
        std::swap(x, y);
        CHECK(n_alloc == a0 && n_free == f0);
        CHECK(x.a.get() == ya && x.a.bytes() == 30 && !x.b && !x.e);
        CHECK(y.a.get() == xa && y.a.bytes() == 10 && y.b.get() == xb && y.b.bytes() == 20 && y.e.get() == xe);
        std::swap(x, x);
        CHECK(x.a.get() == ya && live() == 4);
    }
    CHECK(live() == 0);

    // DevScope
    {
        DevScope mem;
        void *z = (void*)0x1, *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(mem.alloc(&z, 0) == hipSuccess && z != nullptr && last_bytes == 8);      // zero bytes -> 8
        CHECK(mem.alloc(&a, 32) == hipSuccess && mem.alloc(&b, 0) == hipSuccess && mem.alloc(&c, 48) == hipSuccess);
        CHECK(live() == 4);
        mem.release(b);                                                          // a middle element
        CHECK(live() == 3 && mem.v.size() == 4 && mem.v[2] == nullptr);
        int foreign = 0;
        mem.release(&foreign);                                                   // a foreign pointer, null, and one released before
        mem.release(nullptr);
        mem.release(b);
        CHECK(live() == 3);
        ((char*)c)[47] = 1;
        DevScope other(std::move(mem));
        CHECK(mem.v.empty() && other.v.size() == 4 && live() == 3);
        DevScope third;
        void* t = nullptr;
        CHECK(third.alloc(&t, 8) == hipSuccess);
        third = std::move(other);                                                // onto a full scope
        CHECK(live() == 3 && other.v.empty());
    }
    CHECK(live() == 0);
    const int reads0 = last_error_reads;
    CHECK(scope_early_return() == hipErrorOutOfMemory);                          // a failed third allocation, then an early return
    CHECK(last_error_reads == reads0 + 1 && live() == 0);

    // a vector of owning structs: grown (the elements move), erased from, cleared
    {
        std::vector<Entry> cache;
        for (int i = 0; i < 37; ++i) {
            DevMem m;
            CHECK(m.alloc(64 + i) == hipSuccess);
            cache.push_back(Entry{i, std::move(m)});
        }
        CHECK(live() == 37);
        for (int i = 0; i < 37; ++i) { CHECK(cache[i].key == i && cache[i].m.bytes() == (size_t)(64 + i)); cache[i].m.as<char>()[63 + i] = 1; }
        cache.erase(cache.begin() + 5);
        CHECK(live() == 36 && cache[5].key == 6 && cache[5].m.bytes() == 70);
        cache.clear();
        CHECK(live() == 0);
    }

    // events and streams: created, moved, destroyed once
    {
        Event e;
        Stream s;
        CHECK(!e && !s && e.get() == nullptr && s.get() == nullptr);
        CHECK(e.create(hipEventDisableTiming) == hipSuccess && e.get()->flags == hipEventDisableTiming);
        CHECK(s.create(hipStreamNonBlocking) == hipSuccess && s.get()->flags == hipStreamNonBlocking);
        hipEvent_t raw_e = e.get();
        hipStream_t raw_s = s.get();
        Event e2(std::move(e));
        Stream s2(std::move(s));
        CHECK(!e && !s && e2.get() == raw_e && s2.get() == raw_s && live() == 2);
        Event e3;
        Stream s3;
        CHECK(e3.create(0) == hipSuccess && s3.create(0) == hipSuccess && live() == 4);
        e3 = std::move(e2);
        s3 = std::move(s2);
        CHECK(e3.get() == raw_e && s3.get() == raw_s && !e2 && !s2 && live() == 2);
        fail_at = 1;
        CHECK(e.create(0) == hipErrorOutOfMemory && !e);
        fail_at = 1;
        CHECK(s.create(0) == hipErrorOutOfMemory && !s);
        std::vector<Event> ring(8);                                              // the in_copied case
        for (auto& x : ring) CHECK(x.create(hipEventDisableTiming) == hipSuccess);
        CHECK(live() == 10);
        Event grid[3];                                                           // the ev_ring case: created on demand
        CHECK(grid[1].create(hipEventDisableTiming) == hipSuccess && !grid[0] && !grid[2]);
    }
    CHECK(live() == 0);
    CHECK(n_alloc == n_free && n_alloc > 0);
    CHECK(fail_at == 0);

    printf("owners: %ld allocations, %ld frees\n", n_alloc, n_free);
    printf("%d failures\n", bad);
    return bad ? 1 : 0;
}
