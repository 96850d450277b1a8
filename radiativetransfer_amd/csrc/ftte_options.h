// ftte_options.h -- every option of ftte_set_option: where it is stored (Options), what it accepts, what it is refused with and
// whether the plans depend on it (kOptionTable), and the one function that sets one (set).  The brick and the hybrid sweep's options
// keep the rules that resolve them (BrickOptions, HybridOptions); the rest are plain values that the sweeps read at launch time.
// A context holds one Options (ftte_ctx::opt) and shares it with nobody.  Host only; reads no context and launches nothing.
#pragma once

#include <cstring>
#include <string>

#include "ftte_bricks.h"
#include "ftte_hybrid.h"
#include "ftte_tiles.h"

namespace ftte {

// the ray-following tiles (engine 1): built variants rows x stack = 4x{1,4,8}, 8x{1,2,4}, 16x1
struct TileOptions { int rows = 8, slots = 8, waves = 4, stack = 1; };

// what the sweeps read when they launch
struct LaunchOptions {
    int brick_waves = 4, pair_waves = 4; // waves per SIMD the brick kernel, workgroups per SIMD the pair kernel is built for
    int atomic_acc = 0;                  // later visitors of an accumulator add with fp64 atomics instead of read-add-store
    int nu_deal = 16;                    // run length of the deal of a stage launch's frequency groups over the XCDs (brick_deal); 0: work % nnu
    int ablate = 0;                      // diagnostic: parts of the brick kernel's memory traffic left out (wrong J; timing only)
    int tiled = 0;                       // opacities and accumulators stored brick by brick (measured: no gain)
    int merge_overlap = 1;               // brick sweep: J merged block by block as the stages finish the blocks; 0 = one merge after the last stage
    int forest_fuse = 4096;              // levels of a forest with at most this many (segment, group) pairs in one launch (0: a launch per level)
    int lds_pad = 0;                     // diagnostic "ldspad": extra bytes of dynamic LDS per workgroup, to cap residency
    // nothing set that the whole-brick form of the stage launches lacks (launch_brick; BrickOptions::visits)
    bool plain() const { return brick_waves == 4 && !atomic_acc && !ablate && !tiled; }
};

// who sweeps: 0 = the default = 2 = cell-fixed bricks (brick_kernel), 1 = ray-following tiles (sweep_kernel); forest = 1: the
// segment forests on a uniform grid too, for cross-checks
struct RouteOptions { int engine = 0, forest = 0; };

struct Options {
    BrickOptions brick;   // what a brick plan depends on: chunk, group, share, team, lanes, dataflow, queue_mix
    HybridOptions hybrid; // the hybrid sweep of a refined cell array
    TileOptions tile;
    LaunchOptions launch;
    RouteOptions route;
};

// One option: accepted are the values of [lo, hi] that `also` (where there is one) lets through
struct OptionRow {
    const char *name;
    int lo, hi;
    bool (*also)(int);
    const char *refusal;
    int &(*at)(Options &);
    bool invalidates; // the plans are dropped when it is set
};

inline bool power_of_two(int v) { return (v & (v - 1)) == 0; }
inline bool not_one(int v) { return v != 1; }
inline bool divides_64(int v) { return 64 % v == 0; }

#define FTTE_AT(member) [](Options &o) -> int & { return o.member; }
inline const OptionRow kOptionTable[] = {
    {"rows", 4, 16, power_of_two, "rows must be 4, 8 or 16", FTTE_AT(tile.rows), true},
    {"slots", 1, kMaxSlots, nullptr, "slots must be 1..16", FTTE_AT(tile.slots), true},
    {"waves", 2, 6, nullptr, "waves must be 2..6", FTTE_AT(tile.waves), true},
    {"stack", 1, 8, power_of_two, "stack must be 1, 2, 4 or 8", FTTE_AT(tile.stack), true},
    {"engine", 0, 2, nullptr, "engine must be 0 (automatic), 1 (ray-following tiles) or 2 (cell-fixed bricks)", FTTE_AT(route.engine), true},
    {"forest", 0, 1, nullptr, "forest must be 0 or 1", FTTE_AT(route.forest), true},
    {"ldspad", 0, 160 * 1024, nullptr, "ldspad must be 0..163840 bytes", FTTE_AT(launch.lds_pad), true},
    {"chunk", 0, 4096, nullptr, "chunk (layers per brick) must be 1..4096, or 0 for the default", FTTE_AT(brick.chunk), true},
    {"group", 0, kBrickMaxDirs, nullptr, "group (directions sharing a brick pass) must be 1..8, or 0 for the default", FTTE_AT(brick.group), true},
    {"share", 0, 2, nullptr, "share (groups sharing a J accumulator) must be 0 (none), 1 (passes of one izone) or 2 (and izone pairs)", FTTE_AT(brick.share), true},
    {"lanes", 1, 16, nullptr, "lanes (streams the brick sweep spreads its frequency groups over) must be 1..16", FTTE_AT(brick.lanes), true},
    {"team", -1, 2, not_one, "team must be -1 (by the number of frequency groups: 2 up to four, else 0), 0 (one wavefront sweeps a group's directions in turn) or 2 (two wavefronts per brick, four rows each); 1 (a wavefront per direction) lost everywhere and is gone", FTTE_AT(brick.team), true},
    {"dataflow", 0, 3, nullptr, "dataflow must be 0 (a launch per stage), 1 (one launch, bricks wait for each other), 2 (the same with write-through stores) or 3 (persistent workgroups, a task queue per XCD)", FTTE_AT(brick.dataflow), true},
    {"queue_mix", 0, 2, nullptr, "queue_mix must be 0, 1 or 2", FTTE_AT(brick.queue_mix), true},
    {"brick_waves", 2, 4, nullptr, "brick_waves must be 2..4", FTTE_AT(launch.brick_waves), true},
    {"pair_waves", 2, 4, nullptr, "pair_waves (workgroups of two wavefronts per SIMD the pair kernel is built for) must be 2..4", FTTE_AT(launch.pair_waves), true},
    {"atomic_acc", 0, 1, nullptr, "atomic_acc must be 0 or 1", FTTE_AT(launch.atomic_acc), true},
    // (a launch-time choice: no plan depends on it; a captured hybrid sweep, option "graph", keeps the placement it was captured with -- same J)
    {"nu_deal", 0, 4096, nullptr, "nu_deal (tasks of one frequency group that follow each other on an XCD) must be 1..4096, or 0 for workgroup b -> group b mod nnu", FTTE_AT(launch.nu_deal), false},
    {"ablate", 0, 63, nullptr, "ablate is a mask of 6 bits", FTTE_AT(launch.ablate), true},
    {"tiled", 0, 2, nullptr, "tiled must be 0 (default), 1 (bricks: opacities and accumulators stored brick by brick where the grid is made of whole bricks: a brick's layer in one piece) or 2 (the whole brick in one piece)", FTTE_AT(launch.tiled), true},
    {"merge_overlap", 0, 1, nullptr, "merge_overlap must be 0 (the brick sweep merges J after its last stage) or 1 (block by block as the stages finish them)", FTTE_AT(launch.merge_overlap), true},
    {"forest_fuse", 0, 1 << 24, nullptr, "forest_fuse must be 0 (a launch per level) .. 16777216", FTTE_AT(launch.forest_fuse), true},
    {"hybrid", 0, 1, nullptr, "hybrid must be 0 (a refined cell array goes through the forest path as a whole) or 1 (bricks outside a box around the refined cells)", FTTE_AT(hybrid.hybrid), true},
    {"hybrid_slots", 0, 2, nullptr, "hybrid_slots must be 0 (phases), 1 (slots where there are several passes) or 2 (slots always)", FTTE_AT(hybrid.slots), true},
    {"graph", 0, 1, nullptr, "graph must be 0 (every launch of the hybrid sweep issued every time) or 1 (captured once, replayed)", FTTE_AT(hybrid.graph), true},
    {"box_lanes", 1, 64, divides_64, "box_lanes (the boxes of the hybrid sweep end on multiples of it along a brick's 64 lanes) must divide 64", FTTE_AT(hybrid.lanes), true},
    {"forest_batch", 0, 65535, nullptr, "forest_batch (directions per launch of the segment forests) must be 1..65535, or 0 for the default", FTTE_AT(hybrid.forest_batch), true},
    {"pipelines", 1, kMaxPipes, nullptr, "pipelines (independent bricks-forests-bricks sequences of the hybrid sweep, each on a stream of its own) must be 1..4", FTTE_AT(hybrid.pipelines), true},
    {"fine_bricks", 0, 1, nullptr, "fine_bricks must be 0 (a fully refined block stays in the segment forest) or 1 (bricks of its own on the fine level where the block allows it)", FTTE_AT(hybrid.fine_bricks), true},
    {"fine_chunk", 0, 4096, nullptr, "fine_chunk (layers per brick on the fine level of a refined block) must be 1..4096, or 0 for the base bricks' chunk", FTTE_AT(hybrid.fine_chunk), true},
};
#undef FTTE_AT

inline bool accepts(const OptionRow &row, int value) { return value >= row.lo && value <= row.hi && (!row.also || row.also(value)); }

// Sets option `key`.  Refused (an unknown key, a value outside the row's set): *why says so and `opt` stays as it was.  A stored
// value says whether the caller's plans go with it -- also where it is the value already there.
enum class OptionSet { refused, stored, stored_invalidate };
inline OptionSet set(Options &opt, const char *key, int value, std::string *why)
{
    for (const OptionRow &row : kOptionTable) {
        if (std::strcmp(key, row.name)) continue;
        if (!accepts(row, value)) { *why = row.refusal; return OptionSet::refused; }
        row.at(opt) = value;
        return row.invalidates ? OptionSet::stored_invalidate : OptionSet::stored;
    }
    *why = std::string("unknown option: ") + key;
    return OptionSet::refused;
}

} // namespace ftte
