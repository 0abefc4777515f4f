// csrc/bufs.h alone, against tests/hip_stub: built by tests/test_bufs_cpu.py with g++ and the address / undefined-behaviour
// sanitizers and run directly.  Exit status 0 and no sanitizer report mean pass; a failed CHECK prints its line and exits 1.
#include <cstdio>
#include <cstring>
#include <utility>

#include "bufs.h"

static int failures = 0;
#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) { std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond); ++failures; } \
    } while (0)

static int live() { return hip_stub::live_dev + hip_stub::live_host; }

// what common.h's grow does with a buffer, without the handle: nothing when it is large enough
template <class B> static hipError_t grow_like(B &b, size_t count, bool *grew)
{
    *grew = false;
    if (b.size() >= count) return hipSuccess;
    const hipError_t e = b.reset(count);
    if (e == hipSuccess) *grew = true;
    return e;
}

template <class B> static void grow_regrow_shrink(B &b)
{
    bool grew;
    const int held = live();      // by other buffers
    CHECK(b.get() == nullptr && b.size() == 0);
    CHECK(grow_like(b, 0, &grew) == hipSuccess && !grew && b.get() == nullptr);      // nothing asked for: nothing allocated
    CHECK(grow_like(b, 16, &grew) == hipSuccess && grew && b.size() == 16 && b.get());
    std::memset(b.get(), 0x5a, 16);                                                  // (every byte of it is ours)
    void *first = b.get();
    const long allocs = hip_stub::allocs;
    CHECK(grow_like(b, 16, &grew) == hipSuccess && !grew && b.get() == first);       // the same size again
    CHECK(grow_like(b, 3, &grew) == hipSuccess && !grew && b.get() == first && b.size() == 16);      // a smaller one
    CHECK(hip_stub::allocs == allocs);
    CHECK(grow_like(b, 40, &grew) == hipSuccess && grew && b.size() == 40);
    CHECK(hip_stub::allocs == allocs + 1 && live() == held + 1);                           // the old block went first
    std::memset(b.get(), 0x5a, 40);
}

static void reset_failure()
{
    DevBuf<double> d;
    CHECK(d.reset(8) == hipSuccess && live() == 1);
    hip_stub::fail_nth_from_now(1);
    CHECK(d.reset(64) != hipSuccess);
    CHECK(d.get() == nullptr && d.size() == 0 && live() == 0);                       // empty, and the old block is gone
    CHECK(d.reset(64) == hipSuccess && d.size() == 64 && live() == 1);
    d.get()[63] = 1.0;
    HostBuf m(true);
    hip_stub::fail_nth_from_now(1);
    CHECK(m.reset(32) != hipSuccess && m.get() == nullptr && m.dev() == nullptr && m.size() == 0);
    CHECK(m.reset(32) == hipSuccess && m.size() == 32 && live() == 2);
}

// a pair grown together: the second allocation fails, both go out of scope
static void failed_second_of_a_pair()
{
    const int before = live();
    {
        DevBuf<long> a;
        DevBuf<double> b;
        hip_stub::fail_nth_from_now(2);
        CHECK(a.reset(10) == hipSuccess);
        CHECK(b.reset(10) != hipSuccess);
        CHECK(a.size() == 10 && b.size() == 0 && live() == before + 1);
    }
    CHECK(live() == before);
}

static void moves()
{
    DevBuf<int> a;
    CHECK(a.reset(5) == hipSuccess);
    int *pa = a.get();
    DevBuf<int> b(std::move(a));                                                     // move construction
    CHECK(a.get() == nullptr && a.size() == 0 && b.get() == pa && b.size() == 5 && live() == 1);
    DevBuf<int> c;
    c = std::move(b);                                                                // assignment into an empty target
    CHECK(b.get() == nullptr && b.size() == 0 && c.get() == pa && c.size() == 5 && live() == 1);
    DevBuf<int> d;
    CHECK(d.reset(7) == hipSuccess && live() == 2);
    d = std::move(c);                                                                // into a non-empty target: its block is freed
    CHECK(c.get() == nullptr && d.get() == pa && d.size() == 5 && live() == 1);
    DevBuf<int> &self = d;
    d = std::move(self);                                                             // self-move-assignment: nothing happens
    CHECK(d.get() == pa && d.size() == 5 && live() == 1);
    d.get()[4] = 3;
    CHECK(a.reset(2) == hipSuccess && live() == 2);                                  // a moved-from buffer is an empty one
    std::swap(a, d);
    CHECK(a.get() == pa && a.size() == 5 && d.size() == 2 && live() == 2);

    HostBuf h(true);
    CHECK(h.reset(24) == hipSuccess);
    void *ph = h.get();
    HostBuf g(std::move(h));
    CHECK(h.get() == nullptr && h.dev() == nullptr && h.size() == 0 && g.get() == ph && g.dev() == ph && g.size() == 24);
    HostBuf plain(false);
    CHECK(plain.reset(8) == hipSuccess && live() == 4);
    plain = std::move(g);                                                            // the kind travels with the block
    CHECK(g.get() == nullptr && plain.get() == ph && plain.dev() == ph && plain.size() == 24 && live() == 3);
    HostBuf &hs = plain;
    plain = std::move(hs);
    CHECK(plain.get() == ph && plain.size() == 24 && live() == 3);
}

static void release_and_kinds()
{
    DevBuf<char> d;
    d.release();                                                                     // releasing nothing
    CHECK(d.reset(9) == hipSuccess && live() == 1);
    d.release();
    CHECK(d.get() == nullptr && d.size() == 0 && live() == 0);
    d.release();
    HostBuf mapped(true), plain(false);
    CHECK(mapped.reset(64) == hipSuccess && hip_stub::last_host_flags == hipHostMallocMapped);
    CHECK(mapped.dev() != nullptr && mapped.dev() == mapped.get());                  // (the stub's device view is the host address)
    CHECK(plain.reset(64) == hipSuccess && hip_stub::last_host_flags == hipHostMallocDefault);
    CHECK(plain.get() != nullptr && plain.dev() == nullptr);
    std::memset(mapped.get(), 1, 64);
    std::memset(plain.get(), 1, 64);
    mapped.release();
    CHECK(mapped.get() == nullptr && mapped.dev() == nullptr && mapped.size() == 0 && live() == 1);
}

int main()
{
    {
        DevBuf<double> d;
        grow_regrow_shrink(d);
    }
    CHECK(live() == 0);
    {
        HostBuf m(true);
        grow_regrow_shrink(m);
        HostBuf p(false);
        grow_regrow_shrink(p);
    }
    CHECK(live() == 0);
    reset_failure();
    CHECK(live() == 0);
    failed_second_of_a_pair();
    moves();
    CHECK(live() == 0);
    release_and_kinds();
    CHECK(live() == 0 && hip_stub::live_dev == 0 && hip_stub::live_host == 0 && hip_stub::allocs == hip_stub::frees);
    if (failures) return 1;
    std::printf("bufs ok: %ld allocations, all freed\n", hip_stub::allocs);
    return 0;
}
