// ftte_bricks.h -- the host side of a brick sweep (ftte_brick.hip): the options a brick plan depends on and what they resolve to
// (BrickOptions, BrickKey), the plan, the device tables that hold a plan (BrickTables), a buffer that knows the bytes it was sent
// (Sent<T>), the launch record filled from plan and tables (brick_launch), the accumulator list of a merge (acc_list), a lane's
// frequency slice (lane_slice), the lanes' streams and events, what the one-launch forms keep between a sweep and the wait for it
// (BrickDataflow), and the entry points of the context-free planners (ftte_planner.cpp).
// Host only; launches nothing.
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/ftte.h"
#include "ftte_brick_rec.h"
#include "ftte_device.h"
#include "ftte_layout.h"

namespace ftte {

// one planned direction
struct DirPlan {
    int izone = 0, layout = 0;
    double phi = 0, theta = 0, w = 0;
    int64_t org = 0;
    int si = 0, sv = 0, su = 0;
    int u_lo = 1, v_lo = 1, ntu = 0, ntv = 0;
    int du_mid = 0, dv_mid = 0; // drift at the middle layer: where a tile's rays are halfway through the grid
    size_t layer_off = 0; // into the layer table
    int slot = 0;
};

// What a brick plan of the uniform grid depends on beside its directions: the grid, and what the options resolve to for it
// (BrickOptions::resolve).  Two sweeps with equal keys and direction lists share a plan.
struct BrickKey {
    int n = 0;
    double box = 0;
    int chunk = 0, gmax = 0, share = 0;        // layers per brick, most directions per group, who shares an accumulator
    int want_dataflow = 0, want_glanes = 0;    // 0 a launch per stage, 1 one launch, 3 persistent workgroups; streams the groups are dealt to
    int nnu = 0, xcc_count = 0, queue_mix = 0; // what the persistent form's queues are cut for (want_dataflow == 3), else 0
    int duo = 0;                               // 1: two passes of an izone cross a brick in one visit where an izone has two (BrickOptions::visits)
    bool operator==(const BrickKey &o) const
    {
        return n == o.n && box == o.box && chunk == o.chunk && gmax == o.gmax && share == o.share && want_dataflow == o.want_dataflow &&
               want_glanes == o.want_glanes && nnu == o.nnu && xcc_count == o.xcc_count && queue_mix == o.queue_mix && duo == o.duo;
    }
};

// The options a brick plan depends on (ftte_set_option; 0 or -1: by the parallelism there is), and the rules that turn them into
// a plan's parameters.  What the sweep reads when it launches (brick_waves, pair_waves, atomic_acc, nu_deal, ablate, tiled,
// merge_overlap, the LDS pad) is LaunchOptions; both are members of the context's Options, with every option's range (ftte_options.h).
struct BrickOptions {
    int chunk = 0, group = 0; // layers per brick, most directions per group
    int share = 2, team = -1, lanes = 2;
    // 0 = a launch per stage; 1, 2 = the bricks of a sweep in ONE launch where the grid allows it, a workgroup per brick, waiting
    // for each other through flags (cross-XCD hand-overs: L2 write-back per brick, or write-through stores); 3 = one launch of
    // persistent workgroups that draw bricks from a queue per XCD (hand-overs stay behind one L2: plain stores)
    int dataflow = 0;
    int queue_mix = 0;        // persistent form: 0 = a frequency group per queue where they divide, else by load; 1 = by load; 2 = (group + accumulator) mod queues

    // Which form of the brick kernel sweeps: 0 one wavefront per brick, 2 a pair of wavefronts per brick.
    // Option "team" = -1 (the default) leaves it to the parallelism: with four frequency groups or fewer on this GPU (a rank of a
    // frequency-sharded run) the stages are narrow, and the pair form's twice as many wavefronts fill them better (5 / 7 / 9 %
    // at 4 / 2 / 1 groups); at eight the single wavefront is 1.5 % ahead.  The dataflow launch is built for form 0 only.
    // (With the reference's emissivity term -- its log-mean needs a division and two polynomials per piece -- the pair form is ahead
    // at eight groups as well: 103 instead of 162 VGPRs; a source function costs three instructions per piece and goes as no emission.)
    int brick_form(int nnu, int emit_mode) const { return team >= 0 ? team : (((nnu <= 4 || emit_mode) && !dataflow) ? 2 : 0); }

    // The uniform grid's plan.  Unset options follow the parallelism there is: a stage offers (bricks of a plane) x groups x
    // frequency groups tasks, and with few frequency groups on this GPU shorter bricks and smaller groups keep the stages wide
    // enough; the groups are then dealt to the streams instead of the frequency groups.  One launch (want_dataflow 1) needs whole
    // bricks, form 0 and no emission; whether it becomes the persistent form is settled by persistent() once the XCDs are counted.
    // (key.box is the caller's.)
    BrickKey resolve(int n, int nnu, int emit_mode) const
    {
        BrickKey k;
        const int form = brick_form(nnu, emit_mode);
        k.n = n;
        k.chunk = std::min(chunk > 0 ? chunk : (nnu >= 4 ? 16 : nnu >= 2 ? 8 : 4), n);
        k.gmax = group > 0 ? group : (nnu >= 2 || form == 2 ? 3 : 2);
        k.share = share;
        k.want_dataflow = (dataflow && n % 64 == 0 && n % kBrickRows == 0 && n % k.chunk == 0 && form == 0 && !emit_mode) ? 1 : 0;
        k.want_glanes = k.want_dataflow ? 1 : (nnu >= lanes ? 1 : lanes);
        return k;
    }
    // Option "dataflow" = 3 on a grid that allows one launch: persistent workgroups, a queue per XCD, where the device reports
    // 1 .. kBrickQueues of them; else the one-launch form stays
    void persistent(BrickKey &k, int nnu, int xcc_count) const
    {
        if (!k.want_dataflow || dataflow != 3 || xcc_count < 1 || xcc_count > kBrickQueues) return;
        k.want_dataflow = 3; k.nnu = nnu; k.xcc_count = xcc_count; k.queue_mix = queue_mix;
    }
    // Two passes of an izone per visit (brick_duo_kernel), a step of its own like persistent(): only the whole-brick form of the
    // stage launches has it -- one wavefront per brick, no emission, a launch per stage, passes that share accumulators, a grid
    // of whole bricks, and a launch with none of the options that form lacks (`plain_launch`: LaunchOptions::plain()).
    void visits(BrickKey &k, int nnu, int emit_mode, bool plain_launch) const
    {
        if (brick_form(nnu, emit_mode) != 0 || emit_mode || k.want_dataflow || k.share < 1 || !plain_launch) return;
        if (k.n % 64 || k.n % kBrickRows || k.n % k.chunk || k.n / k.chunk >= kBrickLinked) return;
        k.duo = 1;
    }
    // The hybrid sweep's base plan: short bricks (the box is widened by one brick on every side, and what lies inside it costs
    // several times a brick's bytes), the group size by the frequency groups alone (the pair form does not sweep it), a launch
    // per stage: its chunk, gmax and share enter HybridOptions::plan_key
    BrickKey resolve_hybrid(int n, int nnu) const
    {
        BrickKey k;
        k.n = n;
        k.chunk = std::min(chunk > 0 ? chunk : 4, n);
        k.gmax = group > 0 ? group : (nnu >= 2 ? 3 : 2);
        k.share = share;
        return k;
    }
};

// The brick organisation of the same sweep (ftte_brick.hip): directions grouped by izone, bricks ordered into stages
struct BrickPlan {
    bool valid = false;
    long long id = 0;                  // which plan built in this context this is (ftte_ctx::brick_plans): what BrickTables::holds compares
    BrickKey key;                      // the uniform grid's plan: what it was built for, with the directions (a hybrid sweep's plans: HybridPlan::key)
    std::vector<double> phi, theta, w;
    // content
    int n = 0, chunk = 0;              // cells a side, layers per brick
    std::vector<DirPlan> dirs;
    std::vector<LayerRec> layers;
    // (partner, helper -- two passes per visit: the pass this one crosses every brick with, or -1; the one of the two that never touches J)
    struct Group { int izone = 0, layout = 0, acc = 0, offset = 0, lane = 0; std::vector<int> dirs; int partner = -1; bool helper = false; };
    std::vector<Group> groups;
    std::vector<BrickTask> tasks;      // stage after stage
    // Two passes per visit (key.duo, and an izone with two passes): the passes of an izone linked two by two into visits, a visit where
    // a pass stands today (one accumulator, one stage offset, one store-or-accumulate bit per brick); each stage's tasks dealt to seats
    bool duo = false;
    std::vector<BrickSeat> seats;      // stage after stage, the seats with the most directions first
    std::vector<size_t> seat_off;      // [glanes][nstages + 1] into seats
    int nvisits = 0, nlinked = 0;      // visits (passes where nobody is linked); seats that hold a linked visit
    bool dataflow = false;             // one launch, bricks wait for each other through flags (needs whole bricks: n % 64 == 0)
    std::vector<int32_t> deps;         // [tasks][kBrickDeps]
    // persistent form (option "dataflow" = 3): one queue of (task, frequency slot) pairs per XCD, whole dependency chains each
    bool persistent = false;           // (cut for key.nnu frequency groups, key.xcc_count XCDs and key.queue_mix)
    std::vector<uint32_t> queue;       // work ids task * nnu + slot, queue after queue
    uint32_t qoff[kBrickQueues] = {}, qlen[kBrickQueues] = {};
    int64_t qload[kBrickQueues] = {};  // cell.direction.frequency updates per queue (balance: instrumentation)
    int ut = kBrickRows, uw = 0;       // u-face ring: doubles per brick and layer, per layer
    int64_t uqface_off = 0;            // BrickLaunch::uqface_off
    int nslot = 2;                     // face slots along the march (BrickLaunch::nslot)
    int glanes = 1, nstages = 0;       // the groups are dealt to `glanes` streams (the groups of one accumulator stay together)
    std::vector<size_t> stage_off;     // [glanes][nstages + 1] into tasks
    int64_t updates = 0;               // cell.direction updates of a sweep (per frequency group)
    int ntu = 0, ntv = 0, nti = 0, up = 0, vp = 0, max_dirs = 0;
    int64_t face_elems = 0, vface_off = 0, iface_off = 0;
    int nacc[3] = {0, 0, 0};
    // Merge blocks (option "merge_overlap", stages on one lane of groups): kMergeBlock^3 cells aligned with merge_kernel's tiles.
    // Merge point m runs after stage merge_stage[m] and sums the blocks merge_blocks[merge_off[m] .. merge_off[m + 1]) (block id
    // (bi * nmb + bj) * nmb + bk, bi along ic): those whose last writer is in a stage after merge_stage[m - 1] and not after merge_stage[m].
    int nmb = 0;
    std::vector<int32_t> merge_blocks;
    std::vector<int> merge_stage;
    std::vector<size_t> merge_off;
};

// ---- ftte_planner.cpp: the part of the planners that reads no context.  0, or an ftte_status with *err saying why.
// A cubic sub-grid planned like a grid of its own (the fine cells of a fully refined block): side, cell size, and where the layers'
// patterns come from (`patterns` fills n of them for direction d, folded to phi, theta, izone; returns 0 or an ftte_status)
struct SubGridPlan {
    int n = 0;
    double cell = 0;
    std::function<int(int d, double phi, double theta, int izone, ftte_pattern *out)> patterns;
};
int plan_direction(int n, double box, int d, double phi_d, double theta_d, double w_d, int tile_rows, std::vector<ftte_pattern> &pat,
                   std::vector<int> &du_cum, std::vector<int> &dv_cum, DirPlan &D, LayerRec *layers, size_t layer_off, const SubGridPlan *sub,
                   std::string *err);
// The uniform grid's brick plan, step by step: groups, lanes of groups, stage lists, what a brick waits for (one-launch forms),
// merge blocks and merge points, the persistent form's queues.  P.valid with the outcome.
struct BrickInputs { BrickKey key; int ndir; const double *phi, *theta, *w; };
int plan_bricks(const BrickInputs &in, BrickPlan &P, std::string *err);
// (the plan's id stays 0: whoever counts the plans of a context stamps it)
int plan_brick_groups(BrickPlan &P, int n, double box, int ndir, const double *phi, const double *theta, const double *w, int chunk, int gmax,
                      int share, int want_dataflow, bool whole_faces, const SubGridPlan *sub, std::string *err);

// whether a plan's copy of a direction array is the caller's list
inline bool same_list(const std::vector<double> &held, const double *now, int ndir)
{
    return (int)held.size() == ndir && (ndir == 0 || !std::memcmp(held.data(), now, sizeof(double) * ndir));
}

inline const ftte_consts kMath = FTTE_CONSTS_INIT; // the constants of ftte_math.h as the launch records carry them

// `src` in `dst`: room for it, then a blocking copy (none of an empty vector)
template <typename T> hipError_t to_device(DeviceBuffer<T> &dst, const std::vector<T> &src)
{
    const hipError_t e = dst.reserve(src.size());
    if (e != hipSuccess || src.empty()) return e;
    return hipMemcpy(dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice);
}

// A device buffer and the bytes it is known to hold: send() skips the blocking copy when the device already holds exactly these
// (the group records and the background of every iteration after the first).  A buffer that grew or was reset holds nothing.
template <typename T> class Sent {
public:
    T *get() const { return buf_; }
    operator T *() const { return get(); }
    void reset() { buf_.reset(); held_.clear(); }
    hipError_t send(const T *src, size_t count)
    {
        bool fresh = false;
        hipError_t e = buf_.reserve(count, &fresh);
        if (fresh || e != hipSuccess) held_.clear();
        const size_t bytes = sizeof(T) * count;
        if (e != hipSuccess || !bytes || (held_.size() == bytes && !std::memcmp(held_.data(), src, bytes))) return e;
        held_.clear();
        if ((e = hipMemcpy(buf_, src, bytes, hipMemcpyHostToDevice)) == hipSuccess) held_.assign((const char *)src, (const char *)src + bytes);
        return e;
    }
private:
    DeviceBuffer<T> buf_;
    std::vector<char> held_;
};

// The device side of one BrickPlan: layers, tasks, the group records (rebuilt per sweep: they name buffers), and for the uniform
// grid's plan the dependencies, the merge blocks and the persistent form's queues (a queue cut for another nnu is another plan).
// The tables know which plan they hold by its id: plans that share one set of tables (the uniform grid's and the hybrid sweep's)
// displace each other, and whoever comes back uploads again.
struct BrickTables {
    DeviceBuffer<LayerRec> layers; DeviceBuffer<BrickTask> tasks; Sent<BrickGroup> groups;
    DeviceBuffer<int32_t> deps, merge_blocks; DeviceBuffer<uint32_t> queue; // the uniform grid's plan only
    DeviceBuffer<BrickSeat> seats;                                          // ... with two passes per visit
    bool holds(const BrickPlan &P) const { return held_ != 0 && held_ == P.id; }
    hipError_t upload(const BrickPlan &P)
    {
        if (holds(P)) return hipSuccess;
        held_ = 0;
        hipError_t e;
        if ((e = to_device(layers, P.layers)) != hipSuccess || (e = to_device(tasks, P.tasks)) != hipSuccess) return e;
        if (P.dataflow && !P.deps.empty() && (e = to_device(deps, P.deps)) != hipSuccess) return e;
        if (!P.merge_blocks.empty() && (e = to_device(merge_blocks, P.merge_blocks)) != hipSuccess) return e;
        if (P.persistent && !P.queue.empty() && (e = to_device(queue, P.queue)) != hipSuccess) return e;
        if (P.duo && (e = to_device(seats, P.seats)) != hipSuccess) return e;
        held_ = P.id;
        return hipSuccess;
    }
private:
    long long held_ = 0;
};

// The launch record of tasks [task0, task1) of plan P for the frequency groups [nu0, nu1): everything that comes from the plan, its
// tables and the context.  What belongs to one caller -- the dataflow and persistent fields, through, tiled, ablate, atomic_acc, sub -- stays
// zero.  (uqface_off: only masked bricks read it.)
inline BrickLaunch brick_launch(const BrickPlan &P, const BrickTables &T, size_t task0, size_t task1, int nu0, int nu1, int64_t group_stride,
                                int64_t face_stride, const double *uvb, int emit)
{
    BrickLaunch L;
    std::memset(&L, 0, sizeof L);
    L.groups = T.groups; L.tasks = T.tasks + task0; L.uvb = uvb;
    L.group_stride = group_stride; L.face_stride = face_stride;
    L.vface_off = P.vface_off; L.iface_off = P.iface_off; L.uqface_off = P.uqface_off;
    L.n = P.n; L.ntasks = (int)(task1 - task0); L.nnu = nu1 - nu0; L.nu0 = nu0; L.chunk = P.chunk;
    L.up = P.up; L.vp = P.vp; L.uw = P.uw; L.ut = P.ut; L.nslot = P.nslot;
    L.emit = emit; L.math = kMath;
    return L;
}

// What a merge sums, in its fixed order: layout after layout, slot after slot.  frame[l]: the layout the accumulators of layout l
// are stored in; offset: elements into each (a lane's first frequency group).
struct AccList { const double *acc[3 * kMaxAcc]; int layout[3 * kMaxAcc]; int count = 0; };
inline AccList acc_list(const DeviceBuffer<double> (&set)[3][kMaxAcc], const int (&nacc)[3], const int (&frame)[3], size_t offset = 0)
{
    AccList A;
    for (int l = 0; l < 3; ++l)
        for (int s = 0; s < nacc[l]; ++s) { A.acc[A.count] = set[l][s] + offset; A.layout[A.count++] = frame[l]; }
    return A;
}
constexpr int kOwnFrame[3] = {0, 1, 2};

// The frequency groups [nu0, nu1) of lane `lane` of `lanes`, and where they lie in an array of [nnu][ncell] doubles
struct LaneSlice { int nu0, nu1; size_t first, bytes; };
inline LaneSlice lane_slice(int nnu, int lane, int lanes, int64_t ncell)
{
    const int nu0 = (int)((int64_t)nnu * lane / lanes), nu1 = (int)((int64_t)nnu * (lane + 1) / lanes);
    return {nu0, nu1, (size_t)nu0 * (size_t)ncell, sizeof(double) * (size_t)(nu1 - nu0) * (size_t)ncell};
}

// at least `count` events (H = Event; or streams) in `v`
template <typename H> hipError_t ensure_events(std::vector<H> &v, size_t count, unsigned flags)
{
    for (hipError_t rc; v.size() < count;) {
        H h;
        if ((rc = h.create(flags)) != hipSuccess) return rc;
        v.push_back(std::move(h));
    }
    return hipSuccess;
}
// ... and at least `count` extra streams, each with the event that says it is done
inline hipError_t ensure_lanes(std::vector<Stream> &streams, std::vector<Event> &done, size_t count)
{
    const hipError_t rc = ensure_events(streams, count, hipStreamNonBlocking);
    return rc != hipSuccess ? rc : ensure_events(done, count, hipEventDisableTiming);
}

// The one-launch forms of the brick sweep (options "dataflow" 1..3): the flags bricks publish, the tickets and the error word, and
// their pinned copy that the wait for the sweep reads.
struct BrickDataflow {
    static constexpr size_t kSyncWords = 32 * (kBrickQueues + 1);
    DeviceBuffer<uint32_t> done;      // [tasks][nnu]: `epoch` where a brick has finished
    DeviceBuffer<uint32_t> sync;      // [32 q] ticket of queue q (one counter, [0], without queues), [32 kBrickQueues] error
    PinnedBuffer<uint32_t> error;     // what `sync` held at the end of the last such sweep, copied back behind it
    uint32_t qlen[kBrickQueues] = {}; // what those tickets must have reached (0: no persistent sweep pending)
    uint32_t epoch = 0;

    // Room for `nflags` flags, tickets and error word zeroed on `stream`; the flags are zeroed when they are (re)allocated and when
    // the epoch wraps, never in between.  Then the next epoch, into L with the rest of what the kernel waits and signals through.
    hipError_t prepare(BrickLaunch &L, const BrickTables &T, size_t nflags, hipStream_t stream)
    {
        bool fresh = false;
        hipError_t e = done.reserve(nflags, &fresh);
        if (e != hipSuccess) return e;
        if (fresh || epoch == 0xffffffffu) {
            if ((e = hipMemsetAsync(done, 0, sizeof(uint32_t) * done.capacity(), stream)) != hipSuccess) return e;
            epoch = 0;
        }
        if ((e = sync.reserve(kSyncWords)) != hipSuccess || (e = error.reserve(kSyncWords, &fresh)) != hipSuccess) return e;
        if (fresh) std::memset(error, 0, sizeof(uint32_t) * kSyncWords);
        L.ticket = sync; L.error = sync + 32 * kBrickQueues; L.done = done; L.deps = T.deps; L.epoch = ++epoch;
        return hipMemsetAsync(sync, 0, sizeof(uint32_t) * kSyncWords, stream);
    }
    // behind the launch: tickets and error word on their way back; what the queues of a persistent sweep must reach
    hipError_t read_back(const BrickPlan &P, hipStream_t stream)
    {
        if (P.persistent) std::memcpy(qlen, P.qlen, sizeof qlen);
        return hipMemcpyAsync(error, sync, sizeof(uint32_t) * kSyncWords, hipMemcpyDeviceToHost, stream);
    }
    // The sweep is over: null, or why its J is not valid.  (qload: BrickPlan::qload, for the FTTE_QUEUE_STATS print.)
    const char *check_after_sweep(const int64_t *qload)
    {
        if (error && error[32 * kBrickQueues]) {
            error[32 * kBrickQueues] = 0;
            std::memset(qlen, 0, sizeof qlen);
            return "the previous sweep gave up: a brick waited for the bricks it depends on while nothing moved (its J is not valid)";
        }
        if (error && qlen[0] && std::getenv("FTTE_QUEUE_STATS")) { // instrumentation of the persistent form, per queue
            unsigned long long began = 0;
            std::memcpy(&began, error + 32 * kBrickQueues + 2, 8); began = ~began;
            for (int q = 0; q < kBrickQueues; ++q) {
                unsigned long long fin = 0, waited = 0;
                std::memcpy(&fin, error + 32 * q + 2, 8);
                std::memcpy(&waited, error + 32 * q + 4, 8);
                std::fprintf(stderr, "[ftte] queue %d: %u tasks, %u workgroups, drained after %.3f ms, %.1f polls per task, load %lld updates\n", q, qlen[q],
                             error[32 * q + 6], (double)(fin - began) * 1e-5, qlen[q] ? (double)waited / qlen[q] : 0.0, (long long)qload[q]);
            }
        }
        for (int q = 0; q < kBrickQueues; ++q) {
            const uint32_t want = qlen[q];
            qlen[q] = 0;
            if (want && error && error[32 * q] < want)
                return "the previous sweep left a task queue undrained: no workgroup ran on that queue's XCD (its J is not valid)";
        }
        return nullptr;
    }
};

} // namespace ftte
