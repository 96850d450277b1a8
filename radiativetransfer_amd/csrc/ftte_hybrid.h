// ftte_hybrid.h -- the hybrid sweep's own state: its options (HybridOptions), what the planner makes of a tree and a direction
// list (HybridPlan: host data only; ftte_planner.cpp), and what a plan and a tree put on the device (HybridDevice: the
// directions' forests, the leaf list, the fine block's tables, the dense copies of the medium, the fine accumulators, the
// captured graph).  Host only; launches nothing.
#pragma once

#include <string>
#include <vector>

#include "ftte_bricks.h"
#include "ftte_forests.h"

namespace ftte {

constexpr int kMaxPipes = 4; // most pipelines of a hybrid sweep (option "pipelines")

struct HybridOptions {
    int hybrid = 1;       // option: 0 = the whole tree through the forest path
    int slots = 1;        // option "hybrid_slots": 0 = a phase of brick stages per pass even with several passes
    int graph = 0;        // option "graph": replay the sweep's launches from a captured hipGraph (measured slower)
    int forest_batch = 0; // option: most directions per forest batch (0: what the path and the memory allow)
    int lanes = 1;        // option "box_lanes": along u the boxes end on multiples of this many lanes
    int pipelines = 3;    // option "pipelines": independent sequences on streams of their own (1..kMaxPipes)
    int fine_bricks = 1, fine_chunk = 0; // options "fine_bricks", "fine_chunk" (0: the base bricks' chunk)
    // What a plan depends on, with the grid's and the brick options' part of it.  (`hybrid` and `graph` decide who sweeps and how
    // the launches are issued, not what is planned.)
    std::vector<double> plan_key(double box, int chunk, int gmax, int share, int ndir, const double *phi, const double *theta, const double *w) const
    {
        std::vector<double> key = {box, (double)chunk, (double)gmax, (double)share, (double)pipelines, (double)lanes, (double)slots,
                                   (double)forest_batch, (double)fine_bricks, (double)fine_chunk};
        key.insert(key.end(), phi, phi + ndir);
        key.insert(key.end(), theta, theta + ndir);
        key.insert(key.end(), w, w + ndir);
        return key;
    }
};

struct HybridPlan {
    bool valid = false, worthwhile = false;
    std::vector<double> key;          // HybridOptions::plan_key
    BrickPlan bricks;                 // groups, tasks of the bricks outside the boxes
    size_t phase1_stages = 0;         // stage lists per phase
    bool slots = false;               // several passes: launch lists by slot (earliest launch a brick's inputs allow), not by phase
    std::vector<std::vector<int>> pass_at; // [pipeline][pass] the list in front of which the pass's forests are launched
    int most_boxes = 0;               // boxes of the izone that has most
    int npass = 1;                    // passes of the forests (boxes behind other boxes wait for the bricks in between); the
                                      // bricks run in npass + 1 phases: before pass 0, after pass 0, ..., after the last
    size_t nlist = 0;                 // stage lists per pipeline
    int nhalves = 1;                  // pipelines: the groups of an accumulator stay in one; they share nothing but kappa and J
    std::vector<std::vector<int>> half_dirs; // directions of each pipeline, list order
    std::vector<size_t> stage_off;    // into bricks.tasks: [whole | masked][pipeline][list]
    int64_t brick_updates = 0;        // cell.direction updates the bricks perform (per frequency group)
    // A fully refined block swept by bricks of its own on the fine level (option "fine_bricks"; one cluster that is a cube of
    // base cells refined exactly once, twice its side a multiple of 64): inside it the fine cells are a uniform grid
    // with a pattern per sub-layer, and the forest keeps only what lies around it (ftte_amr.h: ForestRegion::has_fine)
    struct Fine {
        bool active = false;
        int n = 0;                          // fine cells a side
        int lo[3] = {0, 0, 0};              // the block's first base cell, storage coordinates (1-based)
        BrickPlan plan;                     // the fine grid's groups (those of `bricks`, an accumulator each) and tasks
        std::vector<size_t> stage_off;      // into plan.tasks: list l = pipeline * nstages + stage is [stage_off[l], stage_off[l + 1])
        int nstages = 0;
        int64_t face_base = 0;              // where the fine face block starts inside a direction's face block (= bricks.face_elems)
        int64_t updates = 0;                // cell.direction updates the fine bricks perform (per frequency group)
        std::vector<int32_t> leaf_of_fine;  // [n^3], fine cell in storage order -> leaf
    } fine;
    // The host side of a direction's forest, restricted to the boxes and numbered by place in `cells`, until it is uploaded
    struct Dir {
        std::vector<SegRec> rec; std::vector<uint8_t> active; std::vector<AmrExport> exports; std::vector<AmrImport> imports;
        std::vector<int64_t> depth_off; std::vector<int32_t> pass_first; std::vector<int64_t> export_first;
    };
    std::vector<Dir> dirs;
    std::vector<int32_t> cells;       // the leaves inside the box of at least one direction, ascending
    std::vector<std::vector<ForestRegion>> regions; // [group] its boxes as the forests are restricted to them (sweep frame)
    // what the planner did, for the counters of whoever called it (also after a failure)
    int brick_plans_made = 0; bool forests_linked = false;

    void invalidate() { valid = false; }
    // the counters "hybrid_boxes", "hybrid_passes", "fine_block": 0 while no plan sweeps
    bool sweeps() const { return valid && worthwhile; }
    long long boxes() const { return sweeps() ? most_boxes : 0; }
    long long passes() const { return sweeps() ? npass : 0; }
    long long fine_block() const { return sweeps() && fine.active ? fine.n : 0; }
};

// Three layouts of one size: where one of them is too small all three are released before the first is allocated anew
struct LayoutSet {
    DeviceBuffer<double> buf[3];
    double *operator[](int l) const { return buf[l]; }
    hipError_t reserve(size_t need)
    {
        if (std::min({buf[0].capacity(), buf[1].capacity(), buf[2].capacity()}) < need)
            for (auto &b : buf) b.reset();
        hipError_t e = hipSuccess;
        for (auto &b : buf) if ((e = b.reserve(need)) != hipSuccess) break;
        return e;
    }
    void sign(std::vector<uintptr_t> &sig) const { for (const auto &b : buf) sig.push_back((uintptr_t)b.get()); }
};

inline void sign_tables(const BrickTables &T, std::vector<uintptr_t> &sig)
{
    for (const void *p : {(const void *)T.layers.get(), (const void *)T.tasks.get(), (const void *)T.groups.get()}) sig.push_back((uintptr_t)p);
}

struct HybridDevice {
    // ---- what follows the plan
    std::vector<ForestTables> dirs;
    DeviceBuffer<int32_t> cells; int64_t ncells = 0;
    long long cells_id = 0;           // which leaf list of this context that is: what the medium's cell-major copies follow
    DeviceBuffer<int32_t> leaf_of_fine;
    BrickTables fine_tables;          // the device side of HybridPlan::Fine::plan
    GraphExec graph_exec;             // the launches of one sweep, captured (hybrid_sweep)
    std::vector<uintptr_t> graph_sig; // what they name
    // ---- what follows the tree
    DeviceBuffer<int32_t> leaf_of_base;
    // ---- sized by what the sweeps ask for, kept from grid to grid
    LayoutSet base_kappa, base_emis;  // the base cells' opacities and emissivity / source function, dense, in the three layouts
    LayoutSet fine_kappa, fine_emis;  // the fine block's
    DeviceBuffer<double> fine_acc[3][kMaxAcc]; // its groups' J accumulators
    Event ev_combine[kMaxPipes];      // pipeline k's forest means are in J

    void drop_graph() { graph_exec.reset(); graph_sig.clear(); }
    void drop_plan()
    {
        dirs.clear();
        cells.reset(); ncells = 0; cells_id = 0;
        leaf_of_fine.reset();
        fine_tables = BrickTables();
        drop_graph();
    }
    void drop_grid() { drop_plan(); leaf_of_base.reset(); }

    // The plan's forests, leaf list and fine block on the device, as leaf list `list`; the host copies of the forests are released
    // as they go.  On failure the caller drops the plan.
    hipError_t upload(HybridPlan &H, const std::vector<double> &w, long long list)
    {
        drop_plan();
        hipError_t e;
        ncells = (int64_t)H.cells.size();
        cells_id = list;
        if ((e = to_device(cells, H.cells)) != hipSuccess) return e;
        dirs.resize(H.dirs.size());
        for (size_t d = 0; d < H.dirs.size(); ++d) {
            HybridPlan::Dir &S = H.dirs[d];
            ForestTables &D = dirs[d];
            D.w = w[d];
            D.nexports = (int64_t)S.exports.size(); D.nimports = (int64_t)S.imports.size();
            if ((e = to_device(D.rec, S.rec)) != hipSuccess || (e = to_device(D.active, S.active)) != hipSuccess ||
                (e = to_device(D.exports, S.exports)) != hipSuccess || (D.nimports && (e = to_device(D.imports, S.imports)) != hipSuccess))
                return e;
            D.depth_off = std::move(S.depth_off); D.pass_first = std::move(S.pass_first); D.export_first = std::move(S.export_first);
            S = HybridPlan::Dir();
        }
        if (H.fine.active) {
            if ((e = to_device(leaf_of_fine, H.fine.leaf_of_fine)) != hipSuccess || (e = fine_tables.upload(H.fine.plan)) != hipSuccess) return e;
            std::vector<int32_t>().swap(H.fine.leaf_of_fine);
        }
        return hipSuccess;
    }
    // the addresses a captured sweep names that this owner holds (the fine block's only where the plan has one)
    void sign(std::vector<uintptr_t> &sig, bool fine, const int (&fine_nacc)[3]) const
    {
        sig.push_back((uintptr_t)cells.get()); sig.push_back((uintptr_t)ncells); sig.push_back((uintptr_t)leaf_of_base.get());
        for (const ForestTables &D : dirs)
            for (const void *p : {(const void *)D.rec.get(), (const void *)D.active.get(), (const void *)D.exports.get(), (const void *)D.imports.get()}) sig.push_back((uintptr_t)p);
        base_kappa.sign(sig); base_emis.sign(sig);
        if (!fine) return;
        sig.push_back((uintptr_t)leaf_of_fine.get());
        sign_tables(fine_tables, sig);
        fine_kappa.sign(sig); fine_emis.sign(sig);
        for (int l = 0; l < 3; ++l) for (int s = 0; s < fine_nacc[l]; ++s) sig.push_back((uintptr_t)fine_acc[l][s].get());
    }
};

// ---- ftte_planner.cpp: the hybrid planner.  Pure host work: it reads what it is given and reports failure with a status and *err.
struct HybridInputs {
    int n; double box; const AmrTree *tree;
    HybridOptions opt;
    int chunk, gmax, share;
    int ndir; const double *phi, *theta, *w;
};
// H.valid with the outcome, or an ftte_status and *err; the caller drops the plan then.  (H.key is the caller's.)
int plan_hybrid(const HybridInputs &in, HybridPlan &H, std::string *err);

} // namespace ftte
