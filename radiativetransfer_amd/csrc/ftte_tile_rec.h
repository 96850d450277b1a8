// ftte_tile_rec.h -- records and launch wrapper of ftte_tile.hip, the ray-following tile sweep (option "engine" = 1).  Plain structs;
// the launch is asynchronous on `stream` and returns 0, -1 bad argument, -2 launch failure.  The host side is ftte_tiles.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "ftte_layer_rec.h"
#include "ftte_math.h"

namespace ftte {

// One direction as a launch sees it.
struct DirRec {
    const LayerRec *layers; // [n], device memory
    const double *kappa;    // opacity in the layout of this direction's march axis, group 0
    double *J;              // accumulator of this direction's slot, same layout, group 0
    const double *emis;     // emissivity or source function in the same layout (LaunchRec::emit), else null
    int64_t org;            // element offset of the virtual cell (i, v, column position) = (0,0,0)
    int32_t si, sv, su;     // element strides along march and v (signed: reflections); su = +1, or -1 when the
                            // u axis is mirrored: the column position of cell u is then n+1-u (stride +1 either way)
    int32_t u_lo, v_lo;     // label of the first owned ray along u / v
    int32_t first;          // 1: J receives a plain store (first direction into this accumulator)
    double w;               // quadrature weight
};

// One wave's work: a tile of 64 x ROWS rays (lane 0 and row 0 are read-only halo) of one
// direction, marched from layer i_first to i_last.
struct WorkItem {
    int16_t slot;    // index into LaunchRec::dir
    int16_t tu, tv;  // tile coordinates
    int16_t i_first, i_last;
    int16_t pad;
};
static_assert(sizeof(WorkItem) == 12, "WorkItem must be 12 bytes");

constexpr int kMaxSlots = 16; // directions of one tile-kernel launch

struct LaunchRec {
    DirRec dir[kMaxSlots];
    const WorkItem *items;
    const double *uvb;  // [nnu], device memory
    int64_t group_stride; // elements between consecutive frequency groups (= ncell)
    int32_t n;          // grid size
    int32_t nitems;
    int32_t nnu;        // frequency groups; workgroup b handles group b % nnu of work item b / nnu
    int32_t emit;       // 0 none, 1 DirRec::emis is the reference's eta, 2 a source function
    ftte_consts math;   // constants of ftte_math.h, delivered through scalar registers
};

// rows x stack: 4x{1,4,8}, 8x{1,2,4}, 16x1; waves: 2, 3, 4, 6
// lds_pad, here and in the brick launches: the caller's option "ldspad", extra bytes of dynamic LDS per workgroup, to cap residency
int launch_sweep(const LaunchRec &L, int rows, int waves, int stack, int nnu, int lds_pad, hipStream_t stream);

} // namespace ftte
