// ftte_brick_rec.h -- records and launch wrappers of ftte_brick.hip, the cell-fixed brick sweep, and the deal of a stage launch's
// workgroups (brick_deal: the function the kernels call, for the host too).  Plain structs; the launches are asynchronous on `stream`
// and return 0, -1 bad argument, -2 launch failure.  The host side is ftte_bricks.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "ftte_layer_rec.h"
#include "ftte_math.h"

namespace ftte {

// ---- cell-fixed bricks (brick_kernel) -----------------------------------------------------------------
// The second organisation of the uniform-grid sweep.  A brick is a block of cells fixed in space, 64 cells along u (the
// wave's lanes) x kBrickRows along v (registers) x `chunk` layers along the march axis, swept by one wavefront for ALL
// the directions of one group (directions that share an izone, hence a memory frame and a sweep order), layer by layer:
// the opacity of a layer is loaded once and its J row stored once for the whole group, nothing is recomputed (no halo),
// and the rays that cross a brick face travel through small ring buffers in memory.  A brick needs its three upstream
// neighbours (u-1, v-1, chunk-1) to be done: bricks with equal tu + tv + ti form a stage, one launch per stage.
constexpr int kBrickRows = 8;
constexpr int kBrickDeps = 6;    // the bricks a brick waits for: u-1, v-1, chunk-1, the previous writer of its J tile, the readers of the two ring slots it reuses
constexpr int kBrickQueues = 8;  // task queues of the persistent form: one per XCD of an MI355X
constexpr int kBrickMaxDirs = 8; // directions of one group (their ray state waits in LDS: 4 KB per direction and wave)

struct BrickDir {
    const LayerRec *layers; // [n]
    double *faces;          // this direction's face rings, frequency group 0: [uface | vface | iface] (BrickLaunch)
    double w;
    double pad;
};

struct BrickGroup {
    BrickDir dir[kBrickMaxDirs];
    const double *kappa; // opacity in the layout of this izone's march axis, frequency group 0
    const double *emis;  // emissivity or source function in the same layout (BrickLaunch::emit), else null
    double *J;           // this group's accumulator (same layout); shared with other groups only as BrickTask says
    int64_t org;         // as DirRec
    int32_t si, sv, su;
    int32_t ndir;
    int32_t bu, bv;      // brick-ordered storage (BrickLaunch::tiled): elements from a brick to the next one along u, along v
    int64_t bi;          // tiled == 2 (a whole brick in one piece): what a step to the next brick along the march adds beyond chunk * si
};

// ti: chunk index; bit 14 set (kBrickAccumulate): another group that shares this group's accumulator has been through this
// brick in an earlier launch, so J is read, added to and stored instead of stored
struct BrickTask { int16_t group, tu, tv, ti; };
constexpr int kBrickAccumulate = 0x4000;
// A task that sweeps a range of lanes only (hybrid sweep, brick_kernel<..., MASKED>): tu bits 0-9 the brick, bits 10-15 the first
// lane; group bits 0-7 the group, bits 8-13 the last lane
// lane; tv bits 0-9 the brick, bits 10-14 the box whose face rings the lanes' ends use
constexpr int kBrickTuMask = 0x3ff, kBrickLaneLoShift = 10, kBrickGroupMask = 0xff, kBrickLaneHiShift = 8;
constexpr int kBrickTvMask = 0x3ff, kBrickBoxShift = 10, kBrickBoxMask = 31;
static_assert(sizeof(BrickTask) == 8, "BrickTask must be 8 bytes");
// A seat of the two-wavefront stage launch (brick_duo_kernel): wavefront w of the workgroup sweeps place[w].  Linked (bit 13 of both
// places' ti, kBrickLinked): two passes of one izone cross the same brick together, place 0 the owner of the cells' J, place 1 the
// helper, whose sums reach J through the owner.  Not linked: two tasks that merely share a workgroup, or one and an empty place
// (group -1).
struct BrickSeat { BrickTask place[2]; };
constexpr int kBrickLinked = 0x2000;
static_assert(sizeof(BrickSeat) == 16, "BrickSeat must be 16 bytes");
// dynamic LDS of a seat: the pad, each wavefront's parked rays (4 KB per direction but one), the 4 KB a helper's sums cross in
constexpr size_t brick_duo_lds(int max_dirs, int lds_pad) { return (size_t)lds_pad + 2 * (size_t)(max_dirs - 1) * kBrickRows * 64 * 8 + (size_t)kBrickRows * 64 * 8; }

struct BrickLaunch {
    const BrickGroup *groups;
    const BrickTask *tasks;   // of this stage
    const double *uvb;        // [nnu]
    int64_t group_stride;     // elements between frequency groups in kappa / J
    int64_t face_stride;      // elements between frequency groups in a direction's face rings
    int64_t vface_off, iface_off; // where the v-face and i-face rings start inside a direction's block (u-face ring at 0)
    int64_t uqface_off;       // more rings laid out like the u-faces of ONE column of bricks, two per box of the direction: the near and
                              // the far u-face of the box where they lie inside a brick (masked bricks of the hybrid sweep)
    int32_t n, ntasks, nnu, chunk; // nnu: frequency groups THIS launch sweeps, nu0, nu0 + 1, ...
    int32_t nu0;
    int32_t emit;             // 0 none, 1 BrickGroup::emis is the reference's eta, 2 a source function (LaunchRec::emit)
    int32_t up, vp;           // padded extents: 64 * ntu, kBrickRows * ntv
    int32_t nslot;            // face slots along the march: 2 = rings over two chunks (a brick's consumers run one stage later), or the
                              // number of chunks (hybrid sweep of a refined cell array: the forest pass reads faces written many stages earlier)
    int32_t uw, ut;           // u-face ring: doubles per layer (ntv * ut) and per brick (ut = kBrickRows, or 16 = one 128-byte line
                              // of its own per brick and layer when bricks of one launch hand rays to each other)
    // Dataflow form (ticket != nullptr): ONE launch holds every brick of the sweep; a workgroup draws the next task of the
    // (topologically ordered) list from `ticket`, waits until the tasks it depends on have published `epoch` in `done`, and
    // publishes its own when its stores are visible.  deps: [ntasks][kBrickDeps] task indices or -1.
    uint32_t *ticket, *done, *error;
    const int32_t *deps;
    uint32_t epoch;
    int32_t through;          // one launch with flags, option "dataflow" = 2: hand-overs by write-through stores instead of an L2 write-back per brick
    // kappa and the accumulators stored brick by brick: the eight rows of a brick's layer in one piece of 4 KB, the pieces of a
    // layer in brick order (v, then u), layers as in the frame.  Whole bricks only (n a multiple of 64 and of kBrickRows).  The
    // group's org, sv, bu, bv are then those of this order (tiled_index, ftte_layout.hip); si is the same in both.  tiled == 2: the
    // `chunk` layers of a brick follow each other as well (the whole brick in one piece of chunk x 4 KB; n a multiple of the chunk).
    int32_t tiled, ablate;    // ablate: diagnostic option "ablate", parts of the memory traffic left out (ftte_brick.hip)
    // Persistent form (queue != nullptr, ftte_brick.hip): as many workgroups as the GPU holds at once, each bound to the XCD it runs
    // on (read from HW_REG_XCC_ID); a workgroup draws (task, frequency group) pairs from ITS XCD's queue only, in queue order, until
    // the queue is empty.  A queue holds whole chains of dependent bricks (everything a brick waits for lies earlier in the same
    // queue), so every ray face and accumulator row a brick reads was written by a CU behind the same L2: plain stores, a drained
    // store counter and a flag suffice, no write-through and no L2 write-back.  Tickets 32 words apart: ticket[32 q].
    const uint32_t *queue;                        // work ids (task index * nnu + frequency slot), queue after queue, each in stage order
    uint32_t qoff[kBrickQueues], qlen[kBrickQueues];
    int8_t xcc_queue[16];                         // XCC id -> queue, from the census of the device's XCC ids (-1: an id the census did not see)
    // A brick that comes second to an accumulator's cells (kBrickAccumulate) adds its sums with fp64 atomic adds instead of reading
    // the earlier ones first: nothing to wait for.  One brick per cell and launch (or, in one launch, in dependency order), so the
    // additions still happen in a fixed order: J stays reproducible bit for bit.
    int32_t atomic_acc;
    // A sweep of a SUB-GRID that has neighbours on every side (the fine cells of a fully refined block of a refined cell array,
    // swept by bricks of their own, ftte_hybrid.cpp): the bricks at the sub-grid's upstream faces take their rays from face rings
    // like everybody else -- ring `ntu` (`ntv`) stands for the missing brick column to the left (row below), chunk slot 0 for the
    // chunk before the first; somebody has filled them (amr_fine_import_kernel) --, and the bricks at its downstream faces leave
    // theirs in their own rings and in chunk slot nti (nslot = nti + 1: no wrap), where the forest behind picks them up.
    int32_t sub;
    // Stage launches (no ticket, no queue): how the launch's workgroups are dealt to (task, frequency slot) pairs, brick_deal below
    // (option "nu_deal"; 0: workgroup b sweeps slot b % nnu of task b / nnu)
    int32_t deal;
    const BrickSeat *seats;   // two passes per visit (brick_duo_kernel): the stage's seats, `ntasks` of them; `tasks` is then not read
    ftte_consts math;
};

// Which (task, frequency slot) pair workgroup `work` of a stage launch sweeps.  Workgroups are dealt round-robin over the XCDs
// (observed behaviour, not a contract), so with slot = work % nnu a launch of 4 groups always puts group nu0 + k on XCDs k and
// k + 4, and the groups are not equally expensive: the optically thick ones pay the thick path of the segment.  Here the slots are
// turned by one after every run of P * deal tasks, P = kXcds / gcd(nnu, kXcds) the tasks after which work % kXcds comes round
// again: over a launch every XCD then sweeps every slot equally often, to within `deal` workgroups, and `deal` neighbouring tasks
// of a slot stay behind one L2.  A bijection on (task, slot) for any nnu and deal; deal = 0: slot = work % nnu.
constexpr unsigned kXcds = 8; // XCDs of gfx950 (MI355X).  Only the balance depends on it, no result does.
struct BrickWork { unsigned task, slot; };
FTTE_HD BrickWork brick_deal(unsigned work, unsigned nnu, unsigned deal)
{
    BrickWork W;
    W.task = work / nnu;
    W.slot = work - W.task * nnu;
    if (deal) {
        const unsigned low = nnu & (0u - nnu), g = low < kXcds ? low : kXcds; // gcd(nnu, kXcds): kXcds is a power of two
        W.slot = (W.slot + W.task / (kXcds / g * deal)) % nnu;
    }
    return W;
}

// one stage of the cell-fixed brick sweep; max_dirs: directions of the launch's largest group (sizes the LDS); waves 2..4
// persistent > 0 (BrickLaunch::queue set): the whole sweep in one launch of that many workgroups, a task queue per XCD
int launch_brick(const BrickLaunch &L, int max_dirs, int waves, int lds_pad, hipStream_t stream, bool masked = false, int persistent = 0);
// a stage of a plan with two passes per visit (BrickLaunch::seats): a workgroup of two wavefronts per seat, whole bricks only;
// launch_brick hands such a launch on to it
int launch_brick_duo(const BrickLaunch &L, int max_dirs, int lds_pad, hipStream_t stream);
bool brick_whole_form(const BrickLaunch &L, int waves, bool masked = false); // does launch_brick take brick_kernel's WHOLE form for this launch?
int launch_xcc_census(unsigned *mask_dev, hipStream_t stream); // bit x of *mask_dev set: some workgroup ran on the XCD whose HW_REG_XCC_ID is x
int launch_brick_pair(const BrickLaunch &L, int max_dirs, int waves, int lds_pad, hipStream_t stream); // two wavefronts per brick, four rows each

} // namespace ftte
