// ftte_forest_rec.h -- records and launch wrappers of ftte_forest.hip: the segment forests of refined cell arrays (ftte_amr.h) as the
// device reads them.  Plain structs; the launches are asynchronous on `stream` and return 0, -1 bad argument, -2 launch failure.
// The host side is ftte_forests.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "ftte_math.h"

namespace ftte {

constexpr int kAmrBatch = 96; // most directions in flight in the forest path (what fits the device memory decides)

// One active segment of a direction's forest, in processing order (sorted by depth)
struct SegRec {
    int32_t seg;     // 3 * leaf + slot: where its outgoing intensity and mean are stored
    int32_t up, up2; // upstream segment (AmrForest::kInflow: the boundary; kImport: a face buffer), second one of the mean-of-two rule or -1
    int32_t at;      // kImport: element of the direction's face block where the ray waits
    double dpath;    // cell size * segment length
};

struct AmrExport { int32_t at, seg; }; // face element <- outgoing intensity of a segment (a ray leaving the forest's region)
// face element of a fine block's own brick sweep <- what the coarser leaf upstream hands over: the outgoing intensity of segment `up`,
// the mean with `up2` where the coarse-neighbour rule asks for it (transportRoutinesModule.f90:612-634), the inflow for up = -1
struct AmrImport { int32_t at, up, up2; };

struct AmrDirRec {
    const SegRec *rec;       // [active segments], depth after depth
    const uint8_t *active;   // [ncell] bit 0: the leaf has an xz segment, bit 1: a yz segment, bit 2: the leaf lies outside the
                             // region this direction's forest is restricted to (hybrid sweep: a brick computed its J)
    double *faces;           // hybrid sweep: this direction's face block (BrickDir::faces), else nullptr
    const AmrExport *exports;
    int64_t nexports;
    const AmrImport *imports; // hybrid sweep with fine blocks swept by bricks: the rays entering the blocks from the forest
    int64_t nimports;
    double *Iout, *mean;     // [3 ncell][nnu] scratch of this direction's slot
    double w;
};

struct AmrLevelRec {
    const AmrDirRec *dir;         // [ndir], device memory
    const int64_t *count;         // [ndir] segments of this depth per direction, device memory
    const int64_t *begin;         // [ndir] where this depth starts in each direction's `rec`, device memory
    int64_t most;                 // largest count[] of this depth (sizes the launch)
    const double *kappa, *uvb, *emis; // element (group g, cell c) at g * group_stride + c * cell_stride
    int64_t group_stride, cell_stride;
    int64_t ncell;
    const int32_t *cells;    // hybrid sweep: the leaves that lie in the region of at least one direction, else nullptr: every leaf.
    int64_t ncells;          // With a list, segments, opacities, activity bytes and scratch are numbered by POSITION in the list
                             // (segment 3 * position + piece): plan and scratch memory follow the regions, not the tree
    int64_t face_stride;     // elements between frequency groups in a direction's face block
    int32_t ndir, nnu, emit;
    ftte_consts math;
};

// refined cell arrays: one depth of the segment forest of up to kAmrBatch directions; then the per-leaf means into J
int launch_cell_major(const double *src, double *dst, long ncell, int nnu, hipStream_t stream, const int32_t *cells = nullptr, long count = 0);
int launch_amr_level(const AmrLevelRec &A, hipStream_t stream);
// levels depth0 .. depth0 + ndepth - 1 in one launch, a workgroup per direction (tables: those levels' [count[ndir], begin[ndir]] pairs)
int launch_amr_levels(const AmrLevelRec &A, const int64_t *tables, int ndepth, hipStream_t stream);
int launch_amr_combine(const AmrLevelRec &A, double *J, bool zero_first, hipStream_t stream);
// hybrid sweep of a refined cell array: leaf-ordered values -> values of the base cells; the rays leaving the forest's region
int launch_base_cells(const double *leaf_values, const int32_t *leaf_of_base, double *base_values, long nbase, long ncell, int nnu,
                      hipStream_t stream);
int launch_amr_export(const AmrLevelRec &A, int64_t most_exports, hipStream_t stream);
int launch_amr_fine_import(const AmrLevelRec &A, int64_t most_imports, hipStream_t stream); // forest -> the face rings of a fine block's bricks

} // namespace ftte
