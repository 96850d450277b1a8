// GasState, ChemState (radiativetransfer_amd/csrc/ftte_gas.h) and TableSets (ftte_point.h) against a stub of the HIP runtime
// (tests/host/stub), under the address and undefined-behaviour sanitizers with leak detection: the call sequences the library performs
// on the species medium, the chemistry's buffers and the rate tables, and after each step whether the gas is ready, ready with a
// density, and whether the tracer's packed copy is current.
#include <cstdio>
#include <cstdlib>

#include "ftte_gas.h"
#include "ftte_point.h"

using namespace ftte;

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); }       \
    } while (0)

// ready for ncell cells, ready with a density, packed copy current
static bool is(const GasState &g, int64_t ncell, bool ready, bool density, bool packed)
{
    return g.ready(ncell) == ready && g.ready_with_density(ncell) == density && g.packed_current() == packed;
}

// point_set_medium: room, (the copies,) then the stamp.  Writes each field's last cell: the block is that large.
static void fill(GasState &g, int64_t ncell, bool with_rho, int dust = 0)
{
    CHECK(g.reserve(ncell) == hipSuccess);
    CHECK(!g.packed_current()); // from the moment the fill starts
    for (int f = 0; f < GasState::kFields; ++f) {
        CHECK(g.field(f) != nullptr);
        g.field(f)[ncell - 1] = 0.0;
    }
    g.filled(ncell, dust, with_rho);
}

// point_trace: room for the packed copy, the launch where it is not current, the stamp
static bool pack(GasState &g, int64_t ncell)
{
    CHECK(g.reserve_packed(kCellRec) == hipSuccess);
    if (g.packed_current()) return false;
    g.packed()[(size_t)kCellRec * ncell - 1] = 0.0;
    g.packed_made();
    return true;
}

// what the table calls do with a set: room for n, then (upload, launch, synchronise) count = n
static void put(TableSets &s, int n)
{
    CHECK(s.reserve(n) == hipSuccess);
    s.count = 0;
    s.tables[(size_t)n * kSetDoubles - 1] = 0.0;
    s.logtab[(size_t)n * kSetDoubles - 1] = 0.0;
    s.count = n;
}

int main()
{
    const long base = stub().live;
    {
        GasState g;
        CHECK(is(g, 64, false, false, false) && is(g, 0, false, false, false) && g.packed() == nullptr);

        // fill, then pack: ftte_set_medium with rho, ftte_point_sources twice
        fill(g, 64, true, 2);
        CHECK(is(g, 64, true, true, false) && !g.ready(65) && !g.ready(0) && g.dust() == 2);
        CHECK(stub().live == base + 5);
        CHECK(pack(g, 64) && is(g, 64, true, true, true) && stub().live == base + 6);
        CHECK(!pack(g, 64) && is(g, 64, true, true, true) && stub().live == base + 6); // the second trace finds it

        // species changed (a committed update), then stale; the next trace packs again into the same buffer
        double *const packed = g.packed();
        g.species_changed();
        CHECK(is(g, 64, true, true, false));
        CHECK(pack(g, 64) && g.packed() == packed && is(g, 64, true, true, true));

        // a new medium for the same grid: the buffers stay, the packed copy is stale
        double *const HI = g.field(GasState::kHI);
        fill(g, 64, true, 0);
        CHECK(g.field(GasState::kHI) == HI && g.packed() == packed && is(g, 64, true, true, false) && g.dust() == 0);
        CHECK(pack(g, 64) && stub().live == base + 6);

        // fill with another cell count: everything is released before the first new buffer is asked for, and the packed copy is
        // not current on its fresh buffer whatever the versions say
        long released = stub().released;
        CHECK(g.reserve(100) == hipSuccess);
        CHECK(stub().released == released + 6 && stub().live == base + 5);
        CHECK(is(g, 64, false, false, false) && is(g, 100, false, false, false) && g.packed() == nullptr); // not ready until filled
        g.filled(100, 1, true);
        CHECK(is(g, 100, true, true, false) && !g.ready(64));
        g.packed_made(); // (even a stamp does not make a missing buffer current)
        CHECK(!g.packed_current());
        CHECK(g.reserve_packed(kCellRec) == hipSuccess && !g.packed_current());
        g.packed()[(size_t)kCellRec * 100 - 1] = 0.0;
        g.packed_made();
        CHECK(is(g, 100, true, true, true));

        // fill without rho: ready, but not for the chemistry, the census or the thin limit
        fill(g, 100, false, 1);
        CHECK(is(g, 100, true, false, false));
        CHECK(pack(g, 100) && is(g, 100, true, false, true));
        fill(g, 100, true, 1);
        CHECK(is(g, 100, true, true, false));

        // failed allocation: a first buffer, and one in the middle of a fill for another grid -> empty, not ready, nothing held
        CHECK(pack(g, 100) && stub().live == base + 6);
        stub().fail_next = true;
        CHECK(g.reserve(200) == hipErrorOutOfMemory);
        CHECK(stub().live == base && is(g, 100, false, false, false) && is(g, 200, false, false, false) && g.packed() == nullptr);
        for (int f = 0; f < GasState::kFields; ++f) CHECK(g.field(f) == nullptr);
        fill(g, 200, true);
        CHECK(is(g, 200, true, true, false) && stub().live == base + 5);
        // ... the packed copy cannot be had: not current, the gas as ready as before, and the next trace goes through
        CHECK(pack(g, 200));
        g.drop();
        fill(g, 200, true);
        stub().fail_next = true;
        CHECK(g.reserve_packed(kCellRec) == hipErrorOutOfMemory);
        CHECK(g.packed() == nullptr && is(g, 200, true, true, false));
        CHECK(pack(g, 200) && is(g, 200, true, true, true));

        // drop() (ftte_set_grid to another grid): nothing is kept; twice is once; usable afterwards
        g.drop();
        CHECK(stub().live == base && is(g, 200, false, false, false) && g.packed() == nullptr);
        g.drop();
        CHECK(stub().live == base);
        fill(g, 8, false);
        CHECK(pack(g, 8) && is(g, 8, true, false, true)); // (the destructor releases these)

        // the chemistry across a grid change: what the grid sizes goes and the temperature with it, the coefficients stay
        ChemState k;
        CHECK(k.k.reserve(6 * 100) == hipSuccess && k.level.reserve(64) == hipSuccess && k.logtem.reserve(64) == hipSuccess);
        CHECK(k.out.reserve(3 * 64) == hipSuccess && k.J.reserve(3 * 64) == hipSuccess && k.counters.reserve(4) == hipSuccess);
        CHECK(k.mass.reserve(10) == hipSuccess);
        k.nratec = 100; k.temperature_set = true; k.steps = 7;
        const long before = stub().live;
        k.drop_grid();
        CHECK(stub().live == before - 4 && !k.level && !k.logtem && !k.out && !k.J && !k.temperature_set);
        CHECK(k.k && k.nratec == 100 && k.counters && k.mass);
        k.drop_grid();
        CHECK(stub().live == before - 4);
        CHECK(k.level.reserve(200) == hipSuccess); // the first update on the new grid

        // a table set: the current tables (count 0 or 1) ...
        TableSets cur;
        CHECK(cur.count == 0 && !cur.tables && !cur.logtab);
        put(cur, 1);
        double *const t1 = cur.tables;
        put(cur, 1); // set again: the buffers stay
        CHECK(cur.count == 1 && cur.tables == t1);
        // ... and the slots growing from 1 to 3 sets and back
        TableSets slots;
        put(slots, 1);
        CHECK(slots.count == 1);
        released = stub().released;
        CHECK(slots.reserve(3) == hipSuccess);
        CHECK(slots.count == 0 && stub().released == released + 2); // replaced: no set is held until the new ones are filled
        slots.tables[3 * kSetDoubles - 1] = 0.0;
        slots.count = 3;
        double *const t3 = slots.tables;
        CHECK(slots.reserve(3) == hipSuccess && slots.count == 3); // room alone changes nothing
        CHECK(slots.reserve(1) == hipSuccess && slots.count == 3 && slots.tables == t3 && stub().released == released + 2);
        put(slots, 1);
        CHECK(slots.count == 1 && slots.tables == t3 && slots.tables.capacity() == 3 * kSetDoubles);
        // a set that cannot be had: nothing is held, whichever of the two buffers it was, and the next call goes through
        stub().fail_next = true;
        CHECK(slots.reserve(5) == hipErrorOutOfMemory);
        CHECK(slots.count == 0 && !slots.tables && !slots.logtab);
        put(slots, 2);
        const long live = stub().live;
        slots.logtab.reset();
        stub().fail_next = true; // (the first buffer has room and asks for nothing: the refusal meets the second)
        CHECK(slots.reserve(2) == hipErrorOutOfMemory);
        CHECK(slots.count == 0 && !slots.tables && !slots.logtab && stub().live == live - 2);
        put(slots, 3);
        CHECK(slots.count == 3);
    }
    CHECK(stub().live == base && g_device_objects.load() == stub().live);
    std::printf("gas state under the sanitizers: ok\n");
    return 0;
}
