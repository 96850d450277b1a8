// ftte_layer_rec.h -- what the tile sweep, the brick sweep and their planners share: the ray classes of the kernel frame and the
// record of one layer of one direction.  Plain structs, no HIP types.
#pragma once
#include <cstdint>

namespace ftte {

// ---- kernel-frame ray classes --------------------------------------------------------------
// In the sweep frame of the reference a layer's ray is one of five chains
// (setPattern, transportRoutinesModule.f90:7-85):  xy | xy->yz | xy->xz | xy->yz->xz | xy->xz->yz,
// a yz segment living one cell further along sweep-k, an xz segment one cell further along
// sweep-j.  The kernel works in a (u, v) frame: u = whichever of sweep-j / sweep-k is contiguous
// in memory for the direction's izone (the wave's lane axis), v = the other one (rows held in
// registers).  In that frame a chain is described by where its 2nd/3rd segments sit:
enum RayClass : int {
    RC_ONE = 0,     // xy only
    RC_TWO_U = 1,   // 2nd segment in cell (v, u+1)
    RC_TWO_V = 2,   // 2nd segment in cell (v+1, u)
    RC_THREE_U = 3, // 2nd in (v, u+1), 3rd in (v+1, u+1)
    RC_THREE_V = 4, // 2nd in (v+1, u), 3rd in (v+1, u+1)
    // same shapes, but the cell's mean adds the chain's 3rd piece before its 2nd: the reference sums
    // xy, xz, yz whatever the chain order (transportRoutinesModule.f90:695-941)
    RC_THREE_U_SWAP = 5,
    RC_THREE_V_SWAP = 6
};

// One layer of one direction, 32 bytes, read with a single scalar load.
struct LayerRec {
    double dpath[3];  // cell size * segment length, chain order (transportRoutinesModule.f90:651)
    int32_t info;     // bits 0-2 RayClass
    int32_t drift;    // cumulative drift of the rays up to this layer: low 16 bits along u, high 16 along v
};
static_assert(sizeof(LayerRec) == 32, "LayerRec must be 32 bytes");

} // namespace ftte
