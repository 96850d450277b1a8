// The owners of radiativetransfer_amd/csrc/ftte_device.h against a stub of the HIP runtime (tests/host/stub), under the address and
// undefined-behaviour sanitizers with leak detection: what is released, when, how often, and what a failed allocation leaves.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "ftte_device.h"

using namespace ftte;

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); }       \
    } while (0)

// the library's counter and the stub's agree, and both stand at `want`
static void live_is(long want)
{
    CHECK(stub().live == want);
    CHECK(g_device_objects.load() == stub().live);
}

template <class B> static void check_buffer()
{
    const long base = stub().live;
    {
        B b;
        CHECK(b.get() == nullptr && b.capacity() == 0);
        live_is(base);
        bool fresh = false;
        CHECK(b.reserve(100, &fresh) == hipSuccess);
        CHECK(fresh && b.get() && b.capacity() == 100);
        b.get()[99] = {}; // the block has 100 elements (else the address sanitizer stops here)
        live_is(base + 1);

        // enough room: the pointer stays, not fresh
        auto *const p = b.get();
        CHECK(b.reserve(60, &fresh) == hipSuccess);
        CHECK(!fresh && b.get() == p && b.capacity() == 100);
        CHECK(b.reserve(100, &fresh) == hipSuccess && !fresh && b.get() == p);
        live_is(base + 1);

        // growing: the old block is gone before the new one is asked for
        long released = stub().released;
        CHECK(b.reserve(101, &fresh) == hipSuccess);
        CHECK(fresh && b.capacity() == 101);
        CHECK(stub().live_at_last_request == base && stub().released == released + 1);
        b.get()[100] = {};
        live_is(base + 1);

        // no elements asked of an empty buffer: a block all the same (kernels are handed a valid pointer), capacity 0
        B z;
        CHECK(z.reserve(0, &fresh) == hipSuccess && fresh && z.get() && z.capacity() == 0);
        CHECK(z.reserve(0, &fresh) == hipSuccess && !fresh);
        live_is(base + 2);
        z.reset();
        CHECK(z.get() == nullptr && z.capacity() == 0);
        live_is(base + 1);
        z.reset(); // twice is once
        live_is(base + 1);

        // moving: the source is empty, one block between the two
        B m(std::move(b));
        CHECK(b.get() == nullptr && b.capacity() == 0 && m.capacity() == 101 && m.get());
        live_is(base + 1);
        B a;
        CHECK(a.reserve(7) == hipSuccess);
        live_is(base + 2);
        released = stub().released;
        a = std::move(m); // a's own block goes, m's arrives
        CHECK(m.get() == nullptr && m.capacity() == 0 && a.capacity() == 101);
        CHECK(stub().released == released + 1);
        live_is(base + 1);
        released = stub().released;
        m.reset(); b.reset();
        CHECK(stub().released == released);
        a.reset();
        CHECK(stub().released == released + 1);
        live_is(base);

        // a failed allocation: the stub's error, an empty buffer without capacity, the old block freed exactly once
        CHECK(a.reserve(10) == hipSuccess);
        live_is(base + 1);
        released = stub().released;
        stub().fail_next = true;
        CHECK(a.reserve(20, &fresh) == hipErrorOutOfMemory);
        CHECK(!fresh && a.get() == nullptr && a.capacity() == 0);
        CHECK(stub().released == released + 1 && stub().live_at_last_request == base);
        live_is(base);
        // ... and a smaller request afterwards allocates instead of passing a capacity test
        CHECK(a.reserve(5, &fresh) == hipSuccess && fresh && a.get() && a.capacity() == 5);
        live_is(base + 1);
        // a failed first allocation
        B f;
        stub().fail_next = true;
        CHECK(f.reserve(3) == hipErrorOutOfMemory && f.get() == nullptr && f.capacity() == 0);
        live_is(base + 1);
        CHECK(f.reserve(3) == hipSuccess);
        live_is(base + 2);
    } // a and f go out of scope with a block each
    live_is(base);
}

template <class H> static void check_created()
{
    const long base = stub().live;
    {
        H h;
        CHECK(h.get() == nullptr);
        CHECK(h.create() == hipSuccess && h.get());
        live_is(base + 1);
        const auto first = h.get();
        CHECK(h.create() == hipSuccess && h.get() == first); // exists: nothing happens
        live_is(base + 1);
        h.reset();
        CHECK(h.get() == nullptr);
        live_is(base);
        h.reset();
        live_is(base);

        stub().fail_next = true;
        CHECK(h.create() == hipErrorOutOfMemory && h.get() == nullptr);
        live_is(base);
        CHECK(h.create() == hipSuccess);

        H m(std::move(h));
        CHECK(h.get() == nullptr && m.get());
        live_is(base + 1);
        H a;
        CHECK(a.create() == hipSuccess);
        live_is(base + 2);
        long released = stub().released;
        a = std::move(m);
        CHECK(m.get() == nullptr && a.get() && stub().released == released + 1);
        live_is(base + 1);
        released = stub().released;
        h.reset(); m.reset();
        CHECK(stub().released == released);
    } // a goes out of scope with its handle
    live_is(base);
}

template <class H, class Raw> static void check_adopted(Raw (*make)())
{
    const long base = stub().live;
    {
        H g;
        g.adopt(make());
        CHECK(g.get());
        live_is(base + 1);
        long released = stub().released;
        g.adopt(make()); // the one held before is destroyed
        CHECK(stub().released == released + 1);
        live_is(base + 1);
        H m(std::move(g));
        CHECK(g.get() == nullptr && m.get());
        g = H{}; // what `plan = HybridPlan{}` does to a member
        live_is(base + 1);
        m = H{};
        CHECK(m.get() == nullptr);
        live_is(base);
        m.adopt(make());
        m.reset();
        live_is(base);
        m.adopt(make());
    }
    live_is(base);
}

int main()
{
    live_is(0);
    check_buffer<DeviceBuffer<double>>();
    check_buffer<DeviceBuffer<char>>();
    check_buffer<PinnedBuffer<unsigned>>();
    check_created<Event>();
    check_created<Stream>();
    check_adopted<Graph, hipGraph_t>(stub_new_graph);
    check_adopted<GraphExec, hipGraphExec_t>(stub_new_graph_exec);
    {   // containers of owners, as the context keeps them
        struct Both { DeviceBuffer<int> a; Event e; };
        Both x;
        CHECK(x.a.reserve(4) == hipSuccess && x.e.create(hipEventDisableTiming) == hipSuccess);
        live_is(2);
        x = Both{};
        live_is(0);
    }
    live_is(0);
    std::printf("device owners under the sanitizers: ok\n");
    return 0;
}
