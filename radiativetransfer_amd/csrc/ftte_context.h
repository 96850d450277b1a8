// ftte_context.h -- what the translation units behind include/ftte.h share: the context, and the internal entry points of the
// planners' cached callers (ftte_plan.cpp; the planners themselves read no context: ftte_planner.cpp), the sweeps
// (ftte_sweeps.cpp: segment forests, cell-fixed bricks), the hybrid sweep of refined cell arrays (ftte_hybrid.cpp) and the
// host-array transfers (ftte_host_arrays.cpp).  ftte_api.cpp is the C ABI itself, ftte_chem.cpp its part that reads or writes the
// species medium, ftte_leaf_pass.cpp the per-leaf updates of the species and the temperature.
//
// Every device buffer, pinned buffer, stream, event and graph of the context is a member that owns it (ftte_device.h): a buffer's
// capacity travels with its pointer, `delete c` releases everything, and a new buffer is added by declaring it.  What a buffer
// holds has an owner as well: the medium's fields (ftte_medium.h), the gas (ftte_gas.h), every option of ftte_set_option with its
// range, its refusal and whether the plans depend on it (ftte_options.h: ftte_ctx::opt, this context's alone), for the brick sweeps
// the rules that resolve their options, the plan, its tables, the buffers that remember what they were sent and the state of
// the one-launch forms (ftte_bricks.h), for the ray-following tiles their plan (ftte_tiles.h), and for the sweeps of
// a refined cell array the forests, their scratch and their cache (ftte_forests.h) and the hybrid sweep's options, plan and device
// state (ftte_hybrid.h), for host arrays the staging blocks and the registered ranges (ftte_host.h), for the tree its copy on the
// device (ftte_device_tree.h), and for point sources the rate tables with their output cross-sections, the accumulated rates, the
// tracer's scratch and the escape record of the last trace (ftte_point.h), and for the star catalogue its scratch and the sources of
// the last catalogue (ftte_star_catalogue.h), and for the sightline spectra the velocity field and their working memory (ftte_spectra.h).  The reference's table mathematics reads no context and no HIP (ftte_tables.cpp).
//
// There is no CPU fallback behind any of this: every entry point that computes on the grid needs a HIP device and fails with
// FTTE_ERR_NO_DEVICE otherwise.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/ftte.h"
#include "ftte_amr.h"
#include "ftte_analysis.h"
#include "ftte_brick_rec.h"
#include "ftte_bricks.h"
#include "ftte_chem.h"
#include "ftte_forest_rec.h"
#include "ftte_gas.h"
#include "ftte_geometry.h"
#include "ftte_host.h"
#include "ftte_hybrid.h"
#include "ftte_lambda.h"
#include "ftte_layout.h"
#include "ftte_medium.h"
#include "ftte_options.h"
#include "ftte_point.h"
#include "ftte_point_rec.h"
#include "ftte_spectra.h"
#include "ftte_star_catalogue.h"
#include "ftte_tile_rec.h"
#include "ftte_tiles.h"


namespace ftte {


extern std::string g_create_error; // what ftte_last_error(NULL) returns

struct LaunchTiming {
    Event start, stop;
    int64_t updates = 0;
    // brick sweep with per-lane layouts and merges: the stage launches of lane k lie between first[k] and last[k] (recorded on the
    // lane's stream); the phase is from the earliest first to the latest last, both measured from `start`
    std::vector<Event> first, last;
    int lanes = 0;
};


} // namespace ftte

using namespace ftte; // this header is the library's own: every unit that includes it lives in ftte or implements the C ABI


namespace ftte { struct Multi; }

struct ftte_ctx {
    ftte::Multi *multi = nullptr;   // ftte_create with ndev > 1: this context only routes to one single-device context per device (ftte_multi.cpp)
    int device = 0;
    Stream stream;                  // (declared in front of the other owners: it goes last)
    std::string err;

    bool grid_set = false;
    int n = 0;
    int64_t ncell = 0;
    double box = 0;

    Options opt; // every option of ftte_set_option (ftte_options.h)

    int nnu = 0;
    MediumField kappa; // the opacities, and their copies in the other layouts, in brick order and cell-major (ftte_medium.h)

    // emissivity (mode 1: the reference's eta) or source function (mode 2): sized as the opacities, the same copies
    int emit_mode = 0;
    MediumField emis;

    DeviceBuffer<double> acc[3][kMaxAcc]; // one size for all of them (accumulator_size)

    int last_brick_form = -1, last_brick_dataflow = -1, last_brick_whole = 0, last_brick_duo = 0; // of the last uniform-grid sweep of the brick engine (ftte_counter)
    std::vector<Stream> lane_stream;        // extra streams of the brick sweep (frequency groups are independent)
    std::vector<Event> pipe_up;             // ftte_diffuse_iteration: lane k's opacities have arrived
    std::vector<Event> lane_done;
    Event ev_fork;
    BrickDataflow bflow;              // flags, tickets and error word of the one-launch forms: brick_sweep prepares, wait_sweep checks
    int xcc_count = -1;               // XCC ids this device reports (census, ftte_brick.hip); -1: not taken yet
    int8_t xcc_queue[16] = {};        // XCC id -> 0 .. xcc_count - 1, or -1
    long long brick_plans = 0;        // brick plans built so far (BrickPlan::id counts from 1)
    BrickPlan bplan;
    BrickTables btables;              // the device side of bplan, or of the hybrid sweep's base plan (hplan.bricks): whichever swept last
    DeviceBuffer<double> d_faces;

    Plan plan;
    DeviceBuffer<LayerRec> d_layers;
    DeviceBuffer<WorkItem> d_items;
    Sent<double> d_uvb;               // the background of the last sweep, whichever path it took
    bool plan_uploaded = false;

    std::vector<LaunchTiming> timing;
    int timing_used = 0;

    // refined cell arrays: the tree, and the per-direction segment forests resident on the device
    AmrTree tree;
    DeviceTree dtree;         // its nodes on the device, for the point-source tracer and the maps (ftte_device_tree.h)
    bool use_forest() const { return (grid_set && tree.refined()) || opt.route.forest; } // refined grid (or option "forest" = 1 on a uniform one, for cross-checks)
    ForestCache forests;      // the whole tree's, per direction (forest_sweep)
    ForestScratch fscratch;   // segment scratch, batch records and per-depth tables of both paths

    // partial merges run beside the sweeps of the next layout on their own (non-blocking) stream
    Stream merge_stream;
    Event ev_layout_done, ev_merge_done, ev_layouts_ready;
    // brick sweep, option "merge_overlap" (1 = default): J merged block by block on merge_stream as the stages finish the blocks
    // (BrickPlan::merge_blocks), behind ev_merge_point[lane * points + m] of each lane; 0 = one merge after the last stage
    std::vector<Event> ev_merge_point;
    // end of the last sweep on whatever stream the caller gave it: the setters and the next sweep wait for it before they
    // overwrite what that sweep reads
    Event ev_sweep_done;
    bool sweep_pending = false;

    // Hybrid sweep of a refined cell array: bricks outside a box around the refined cells, the segment forest inside it
    HybridPlan hplan;
    HybridDevice hdev;                // what hplan and the tree put on the device
    long long leaf_lists = 0;         // leaf lists built so far (HybridDevice::cells_id counts from 1)

    // The species medium (ftte_gas.h): ftte_set_medium fills it; the tracer, the chemistry, the census, ftte_compute_opacities and
    // the thin limit read it; the chemistry's updates write its species and say so
    GasState gas;
    PointState point; // point sources: rate tables, rates, tracer scratch, escape record (ftte_point.h)

    HostBoundary host; // host arrays (ftte_set_opacity / ftte_diffuse_sweep): staging blocks, registered arrays, J on the device (ftte_host.h)

    // instrumentation (ftte_counter): how often the expensive host-side builds ran
    long long n_grid_builds = 0, n_plan_builds = 0, n_forest_builds = 0;

    std::vector<int8_t> leaf_level;  // per leaf, as handed to ftte_set_grid
    ChemState chem;                  // ionisation equilibrium (ftte_chem.cpp)
    AnalysisState analysis;          // maps and censuses of the medium (ftte_analysis.cpp)
    SpectraState spectra;            // the velocity field, and the working memory of the sightline spectra (ftte_spectra.cpp)

    // accelerated source iteration (ftte_lambda_host.cpp): the segment-length tables of the last direction list, the leaves' places on
    // their levels (made for the tree of grid build lambda_leaves_grid) with the sub-layers that hold a leaf, the update's statistics
    DeviceBuffer<LambdaRec> d_lambda_table;
    DeviceBuffer<LambdaDir> d_lambda_dirs;
    DeviceBuffer<LambdaLeaf> d_lambda_leaves;
    long long lambda_leaves_grid = -1;
    std::vector<uint8_t> lambda_used;  // [3 axes][level after level][position]
    DeviceBuffer<double> d_lambda_host; // ftte_lambda_diagonal: the diagonal on its way to the caller's host array
    DeviceBuffer<unsigned long long> d_update_stats;
    PinnedBuffer<unsigned long long> h_update_stats;

    StarCatalogue catalogue; // stars -> host leaves -> merged sources (ftte_star_catalogue.h)
};

namespace ftte {

int fail(ftte_ctx *c, int code, const std::string &msg);

#define FTTE_HIP(c, call)                                                                                          \
    do {                                                                                                           \
        hipError_t e_ = (call);                                                                                    \
        if (e_ != hipSuccess)                                                                                      \
            return fail((c), FTTE_ERR_NO_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_));               \
    } while (0)

// For the entry points that need no grid: 0, or what a missing or a multi-device context is refused with (check_ready does the
// same as its first act)
int check_single(ftte_ctx *c);

// ---- ftte_plan.cpp
int build_plan(ftte_ctx *c, int rows, int stack, int ndir, const double *phi, const double *theta, const double *w);
int build_brick_plan(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w);
int xcc_census(ftte_ctx *c); // fills ftte_ctx::xcc_count, xcc_queue (once per context)

// ---- ftte_sweeps.cpp
int ensure_kappa(ftte_ctx *c, int nnu);
int check_ready(ftte_ctx *c, bool need_kappa);
int wait_sweep(ftte_ctx *c);
int mark_sweep(ftte_ctx *c, hipStream_t stream);
int ensure_timing(ftte_ctx *c, size_t count); // at least `count` launch records with both events
// The cell-major copy of a field current on `stream`: every leaf in cell-array order, or (list: HybridDevice::cells_id) the leaves `cells`
int make_cell_major(ftte_ctx *c, MediumField &f, hipStream_t stream, const int32_t *cells = nullptr, int64_t ncells = 0, long long list = 0);
// Group g of a brick plan as the kernel reads it: its arrays in the layout it marches through, its directions' layer tables from
// `layers` and face blocks from `faces`, face_stride elements per direction
void fill_brick_group(BrickGroup &G, const BrickPlan &P, size_t g, const double *kappa, const double *emis, double *J, const LayerRec *layers,
                      double *faces, size_t face_stride);
// The accumulators of a set (ftte_ctx::acc, HybridDevice::fine_acc) have one size.  Where that is less than per_acc elements every one of them is
// released; returns the size to reserve for those a sweep uses.
size_t accumulator_size(DeviceBuffer<double> (&acc)[3][kMaxAcc], size_t per_acc);

// A forest pass made ready: the per-direction records and the per-depth tables are in device memory (a batch of 96 would not
// fit the kernel arguments), what is left is a list of launches.
struct ForestRun {
    struct Pass { size_t table_at = 0, most_at = 0, maxdepth = 0, export_at = 0; int64_t most_exports = 0; };
    struct Batch { int d0 = 0, nb = 0; std::vector<Pass> passes; };
    std::vector<Batch> batches;
    std::vector<int64_t> most_of;
    size_t dir_at = 0;
};

int prepare_forests(ftte_ctx *c, hipStream_t stream, const std::vector<std::vector<ForestDir>> &sets, const std::vector<int> &slot0,
                    int batch, size_t per_dir, std::vector<ForestRun> *runs);
int launch_forest_pass(ftte_ctx *c, hipStream_t stream, const ForestRun &R, size_t b, size_t p, AmrLevelRec A);
int launch_forest_combine(ftte_ctx *c, hipStream_t stream, const ForestRun &R, size_t b, AmrLevelRec A, double *J_dev, bool zero_first);
int launch_forests(ftte_ctx *c, hipStream_t stream, const ForestRun &R, AmrLevelRec A, double *J_dev, bool zero_first, bool time_batches,
                   hipEvent_t before_combine, hipEvent_t after_combine);
int run_forests(ftte_ctx *c, hipStream_t stream, const std::vector<ForestDir> &dirs, int batch, size_t per_dir, AmrLevelRec A,
                double *J_dev, bool zero_first, bool time_batches);
int forest_sweep(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, const double *uvb,
                 double *J_dev, hipStream_t stream);

// The sweep of a uniform grid by cell-fixed bricks (ftte_brick.hip): one launch per stage, then one merge of the groups'
// accumulators (layout after layout, group after group: a fixed order) into J.
// Host arrays handed over with the sweep (ftte_diffuse_iteration): the opacities go up and J comes back one lane of frequency
// groups at a time, on the lane's own stream, so that the first lane is swept while the second one's opacities are still on the
// PCIe link and its J travels back while the second is swept.
struct HostPipe { const double *kappa; double *J; };
int brick_sweep(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, const double *uvb, double *J_dev,
                hipStream_t stream, const HostPipe *pipe = nullptr);

int tile_sweep(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, const double *uvb, double *J_dev,
               hipStream_t stream);

// ---- ftte_hybrid.cpp
int hybrid_sweep(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, const double *uvb, double *J_dev,
                 hipStream_t stream, bool *done);

// ---- ftte_multi.cpp: several devices behind one context
int multi_create(ftte_ctx **out, int ndev, const int *dev_ids);
int multi_destroy(ftte_ctx *c);
int multi_set_grid(ftte_ctx *c, int nx, int ny, int nz, int64_t ncell, const int32_t *level, double box_cm);
int multi_set_opacity(ftte_ctx *c, int nnu, const double *kappa);
int multi_set_emission(ftte_ctx *c, int mode, const double *values);
int multi_set_option(ftte_ctx *c, const char *key, int value);
int multi_sweep(ftte_ctx *c, int ndir, const double *phi, const double *theta, const double *w, const double *uvb, double *J);
int multi_iteration(ftte_ctx *c, int nnu, const double *kappa, int ndir, const double *phi, const double *theta, const double *w,
                    const double *uvb, double *J);
long long multi_counter(const ftte_ctx *c, const char *name);
const char *multi_how(const ftte_ctx *c);
ftte_ctx *multi_first(const ftte_ctx *c);
int multi_host_register(ftte_ctx *c, void *ptr, size_t bytes, bool on);

// ---- ftte_leaf_pass.cpp
int ensure_level(ftte_ctx *c); // the leaves' levels in ChemState::level (uploaded on first use after ftte_set_grid)
int hydrogen_mass(ftte_ctx *c, const double *HI_dev, double *neutral, double *total, const char *who); // computeMass over the leaves of HI [msun]

// ---- ftte_host_arrays.cpp
bool is_registered(const ftte_ctx *c, const void *p, size_t bytes);
int upload(ftte_ctx *c, void *dst_dev, const void *src_host, size_t bytes);
int download(ftte_ctx *c, void *dst_host, const void *src_dev, size_t bytes);
int upload_on(ftte_ctx *c, hipStream_t q, void *dst_dev, const void *src_host, size_t bytes);
int download_on(ftte_ctx *c, hipStream_t q, void *dst_host, const void *src_dev, size_t bytes);

} // namespace ftte
