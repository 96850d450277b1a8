// MediumField (radiativetransfer_amd/csrc/ftte_medium.h) against a stub of the HIP runtime (tests/host/stub), under the address and
// undefined-behaviour sanitizers with leak detection: the call sequences the library performs on a field of the medium, and after
// each step which of its copies are current.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "ftte_medium.h"

using namespace ftte;
using F = MediumField;

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); }       \
    } while (0)

static const F::Copy kAll[] = {F::kLayout1, F::kLayout2, F::kBricks0, F::kBricks1, F::kBricks2, F::kCellMajor};

// no copy is current, whatever it is asked for
static bool all_stale(const F &f)
{
    for (F::Copy x : kAll)
        for (long long p : {0LL, 1LL, 2LL, 8LL, 16LL})
            if (f.current(x, p)) return false;
    return true;
}

// what a sweep does for a copy: room, then (the launch,) then the stamp
static void make(F &f, F::Copy x, long long param = 0, size_t need = 0)
{
    CHECK(f.reserve(x, need) == hipSuccess);
    CHECK(f.copy(x) != nullptr);
    f.copy(x)[(need ? need : f.capacity()) - 1] = 0.0; // the block is that large (else the address sanitizer stops here)
    f.made(x, param);
}

int main()
{
    const long base = stub().live;
    {
        F f;
        CHECK(!f.valid() && f.source() == nullptr && f.capacity() == 0 && all_stale(f));

        // ftte_set_opacity: room, upload, set -> a valid source, every copy stale
        CHECK(f.reserve_source(1000) == hipSuccess);
        CHECK(f.source() && f.capacity() == 1000 && !f.valid() && all_stale(f));
        f.set();
        CHECK(f.valid() && all_stale(f));
        CHECK(f.in_layout(0) == f.source() && f.in_layout(2) == nullptr);
        CHECK(stub().live == base + 1);

        // a sweep makes layouts 1 and 2, sized by the source
        make(f, F::layout(1));
        make(f, F::layout(2));
        CHECK(f.current(F::kLayout1) && f.current(F::kLayout2) && !f.current(F::kCellMajor) && !f.current(F::kBricks2));
        CHECK(f.in_layout(1) == f.copy(F::kLayout1) && f.in_layout(2) == f.copy(F::kLayout2));
        CHECK(stub().live == base + 3);
        // the next sweep finds them: nothing is allocated, nothing goes stale
        double *const l2 = f.copy(F::kLayout2);
        CHECK(f.reserve(F::kLayout2) == hipSuccess && f.copy(F::kLayout2) == l2 && f.current(F::kLayout2));

        // set again (same size: the buffers stay) -> stale
        CHECK(f.reserve_source(1000) == hipSuccess && f.reserve_source(500) == hipSuccess);
        CHECK(f.current(F::kLayout1) && f.current(F::kLayout2)); // (room alone changes nothing)
        f.set();
        CHECK(f.valid() && all_stale(f) && f.copy(F::kLayout2) == l2);
        CHECK(stub().live == base + 3);

        // brick order (option "tiled") and the cell-major copy of the whole tree beside the layouts
        make(f, F::layout(1));
        make(f, F::layout(2));
        make(f, F::bricks(0), 16);
        make(f, F::bricks(2), 0);
        make(f, F::kCellMajor, 0, 1000);
        CHECK(f.current(F::kBricks0, 16) && !f.current(F::kBricks0, 8) && !f.current(F::kBricks0, 0));
        CHECK(f.current(F::kBricks2, 0) && !f.current(F::kBricks2, 16) && !f.current(F::kBricks1, 0) && !f.current(F::kBricks1, 16));
        make(f, F::bricks(0), 8); // made anew for other pieces
        CHECK(f.current(F::kBricks0, 8) && !f.current(F::kBricks0, 16));

        // ftte_set_opacity_device, one pass that writes layout 2 with the source: it stays current, nothing else does
        f.set();
        f.made(F::kLayout2);
        CHECK(f.current(F::kLayout2) && !f.current(F::kLayout1) && !f.current(F::kCellMajor) && !f.current(F::kBricks0, 8) &&
              !f.current(F::kBricks2, 0));
        // ... and with layouts 1 and 2 (the tile engine keeps both)
        make(f, F::layout(1));
        make(f, F::kCellMajor, 0, 1000);
        make(f, F::bricks(0), 8);
        f.set();
        f.made(F::kLayout2);
        f.made(F::kLayout1);
        CHECK(f.current(F::kLayout1) && f.current(F::kLayout2) && !f.current(F::kCellMajor) && !f.current(F::kBricks0, 8));

        // the cell-major copy: every leaf (0) or the leaves of list 1, 2, ... of the hybrid plan
        make(f, F::kCellMajor, 0, 1000);
        CHECK(f.current(F::kCellMajor, 0) && !f.current(F::kCellMajor, 1));
        make(f, F::kCellMajor, 1, 300); // (the buffer is large enough: it stays)
        CHECK(f.current(F::kCellMajor, 1) && !f.current(F::kCellMajor, 0));
        CHECK(!f.current(F::kCellMajor, 2)); // a new list of the same length
        make(f, F::kCellMajor, 2, 300);
        CHECK(f.current(F::kCellMajor, 2) && !f.current(F::kCellMajor, 1) && f.current(F::kLayout2));

        // a copy's own buffer grows (a longer leaf list): that copy is stale and no other
        CHECK(stub().live == base + 6);
        long released = stub().released;
        CHECK(f.reserve(F::kCellMajor, 2000) == hipSuccess);
        CHECK(stub().released == released + 1 && stub().live == base + 6);
        CHECK(!f.current(F::kCellMajor, 2) && f.current(F::kLayout1) && f.current(F::kLayout2));
        f.made(F::kCellMajor, 2);
        CHECK(f.current(F::kCellMajor, 2));

        // more frequency groups than the source holds: the source and every copy are released before the new source is
        // asked for, and nothing is current or valid
        released = stub().released;
        CHECK(f.reserve_source(1001) == hipSuccess);
        CHECK(stub().released == released + 6 && stub().live_at_last_request == base && stub().live == base + 1);
        CHECK(f.capacity() == 1001 && !f.valid() && all_stale(f));
        for (F::Copy x : kAll) CHECK(f.copy(x) == nullptr);
        f.set();
        CHECK(all_stale(f));
        make(f, F::layout(2)); // sized by the new source
        CHECK(f.current(F::kLayout2));

        // ftte_diffuse_iteration: no valid source while the lanes bring it, their layouts reserved but not made; when every lane has
        // been issued the source is set and the layouts the lanes transposed are made
        f.invalidate();
        CHECK(!f.valid() && all_stale(f));
        CHECK(f.reserve(F::layout(2)) == hipSuccess);
        CHECK(!f.valid() && all_stale(f));
        f.set();
        CHECK(f.valid() && all_stale(f));
        f.made(F::layout(2));
        CHECK(f.current(F::kLayout2) && !f.current(F::kLayout1));
        // ... or the sweep failed half way: no valid source, nothing current, and the next setter starts over
        f.invalidate();
        CHECK(!f.valid() && all_stale(f));
        f.set();
        CHECK(f.valid() && all_stale(f));

        // a copy that cannot be had: its buffer is empty, it is stale, the others are untouched, and the next call goes through
        make(f, F::layout(2));
        make(f, F::kCellMajor, 0, 10);
        stub().fail_next = true;
        CHECK(f.reserve(F::kCellMajor, 5000) == hipErrorOutOfMemory);
        CHECK(f.copy(F::kCellMajor) == nullptr && !f.current(F::kCellMajor, 0) && f.current(F::kLayout2) && f.valid());
        f.made(F::kCellMajor, 0); // (even a stamp does not make an empty buffer current)
        CHECK(!f.current(F::kCellMajor, 0));
        make(f, F::kCellMajor, 0, 5000);
        CHECK(f.current(F::kCellMajor, 0));
        stub().fail_next = true;
        CHECK(f.reserve(F::layout(1)) == hipErrorOutOfMemory); // a first allocation
        CHECK(f.copy(F::kLayout1) == nullptr && !f.current(F::kLayout1) && f.current(F::kLayout2));

        // a source that cannot be had: the field is empty -- what depended on it went with it -- and usable
        CHECK(stub().live == base + 3);
        stub().fail_next = true;
        CHECK(f.reserve_source(9000) == hipErrorOutOfMemory);
        CHECK(stub().live == base && f.source() == nullptr && f.capacity() == 0 && !f.valid() && all_stale(f));
        for (F::Copy x : kAll) CHECK(f.copy(x) == nullptr);
        CHECK(f.reserve_source(9000) == hipSuccess);
        f.set();
        make(f, F::layout(2));
        CHECK(f.valid() && f.current(F::kLayout2) && f.capacity() == 9000 && stub().live == base + 2);

        // moved: the buffers travel, the object left behind has none and nothing current
        F g(std::move(f));
        CHECK(g.current(F::kLayout2) && g.valid() && g.capacity() == 9000);
        CHECK(f.source() == nullptr && f.copy(F::kLayout2) == nullptr && all_stale(f));
        CHECK(stub().live == base + 2);

        // ftte_set_grid to another grid: everything goes
        make(g, F::bricks(1), 16);
        make(g, F::kCellMajor, 3, 40);
        CHECK(stub().live == base + 4);
        g.release();
        CHECK(stub().live == base && !g.valid() && all_stale(g) && g.source() == nullptr);
        g.release(); // twice is once
        CHECK(stub().live == base);
        // ... and the destructor releases what is there
        CHECK(g.reserve_source(10) == hipSuccess);
        g.set();
        make(g, F::layout(1));
    }
    CHECK(stub().live == base && g_device_objects.load() == stub().live);
    std::printf("medium field under the sanitizers: ok\n");
    return 0;
}
