// ftte_tiles.h -- the host side of the ray-following tile sweep (ftte::sweep_kernel, option "engine" = 1): its plan (directions,
// layer tables, work items, launches) and the entry point of its context-free planner (ftte_planner.cpp).
// Host only; launches nothing.
#pragma once

#include "ftte_bricks.h"
#include "ftte_layer_rec.h"
#include "ftte_tile_rec.h"

namespace ftte {

struct LaunchPlan {
    int layout = 0;
    bool first = false;
    std::vector<int> dirs; // indices into Plan::dirs, position = slot
    int acc_base = 0;      // slot s of this launch accumulates into acc[layout][acc_base + s]
    size_t item_off = 0;
    int nitems = 0;
    int64_t updates = 0;
};

struct Plan {
    bool valid = false;
    // key
    int n = 0, rows = 0, slots = 0, stack = 0;
    double box = 0;
    std::vector<double> phi, theta, w;
    // content
    std::vector<DirPlan> dirs;
    std::vector<LayerRec> layers;
    std::vector<WorkItem> items;
    std::vector<LaunchPlan> launches;
    bool used[3][kMaxSlots] = {};
};

// ---- ftte_planner.cpp.  P.valid with the outcome, or an ftte_status with *err saying why.
struct TileInputs { int n; double box; int rows, stack, slots; int ndir; const double *phi, *theta, *w; };
int plan_tiles(const TileInputs &in, Plan &P, std::string *err);

} // namespace ftte
