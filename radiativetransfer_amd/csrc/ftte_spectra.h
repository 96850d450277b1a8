// ftte_spectra.h -- absorption spectra along the pixel columns of the projected map: the optical depth of one line in velocity
// space, tau(v), and per sightline the column density N, the equivalent width W and the velocity width dv90 (the statement:
// ftte_spectra_math.h).  Nothing of this is the reference's; the sightlines are those of ftte_project_map (ftte_analysis.h: the
// same axis tables, the same depth, the same leaves in the same order).  Here: what the context keeps for it (SpectraState: the
// velocity field and the working memory), the records the kernels of ftte_spectra.hip read, and the context-free batch rule.
#pragma once

#include <cstddef>
#include <cstdint>

#include "ftte_analysis.h"
#include "ftte_device.h"
#include "ftte_node_rec.h"
#include "ftte_spectra_math.h"

namespace ftte {

constexpr int kSpectraLanes = 256;          // one workgroup per sightline
constexpr int kSpectraChunk = 512;          // segments of a sightline in LDS at a time: 16 KiB of records
constexpr int kSpectraPixelsPerLane = 4;    // tau of a lane's pixels p = tid + 256 r in registers
constexpr int kSpectraPassPixels = kSpectraLanes * kSpectraPixelsPerLane;
constexpr size_t kSpectraWorkBytes = (size_t)64 << 20; // tau of a batch (where it is staged) and its segment spill stay below this
static_assert(sizeof(ftte_spectra_seg) == 32, "a segment record is four doubles");
static_assert((size_t)kSpectraChunk * sizeof(ftte_spectra_seg) >= 2 * sizeof(double) * kSpectraPassPixels, "the summaries stage a pass in the records' LDS");
static_assert((size_t)kSpectraChunk * sizeof(ftte_spectra_seg) + 2 * sizeof(int32_t) * kSpectraLanes <= 64 * 1024, "static LDS");

// One call's geometry and medium, shared by the two kernels
struct SpectraRec {
    const NodeRec *node;          // nullptr on a uniform grid: base cell == leaf
    const double *value;          // [ncell] absorber density
    const double *tgas;           // [ncell]
    const double *vel;            // [ncell] the component along the depth axis, or nullptr: zero
    const int32_t *ibase, *jbase; // [nxmap], [nymap]: i0, j0, 1-based (ftte_map_axis)
    const double *ifrac, *jfrac;
    MapZone zone;
    int32_t n, nxmap, nymap;
    int32_t fast_is_j;            // the check pass: neighbouring lanes along the map's second axis
    int32_t kstart, kend;         // ftte_map_depth
    int32_t vel_negate;           // the depth axis is mirrored in storage
    double cell_cm;
    ftte_spectra_par par;
    ftte_consts K;
    // the check pass, all sightlines: per line its segments and N; flags[0] a leaf without a line width, flags[1] the most segments
    int32_t *nseg;                // [nxmap * nymap]
    double *column;               // [nxmap * nymap]
    int32_t *flags;               // [2], zero before the launch
    // the spectra of lines line0 .. line0 + nlines - 1 (line = i + nxmap j), one workgroup each
    int64_t line0;
    int32_t nlines, nvel;
    double *tau;                  // [nlines][nvel], line0's first
    double *summary;              // [nlines][3] or nullptr
    ftte_spectra_seg *spill;      // [nlines][spill_stride] for the lines with more than kSpectraChunk segments, or nullptr
    int64_t spill_stride;
};

// What the spectra keep on the device.  Owned by the context; dropped with the grid.
struct SpectraState {
    DeviceBuffer<double> vel[3];   // along storage i, j, k; all three or none
    bool velocity_set = false;
    DeviceBuffer<int32_t> base[2];
    DeviceBuffer<double> frac[2];
    DeviceBuffer<double> value;    // a host value array on its way to the kernel
    DeviceBuffer<int32_t> nseg, flags;
    DeviceBuffer<double> column;
    DeviceBuffer<double> tau, summary; // of a batch, where the caller's are on the host or absent
    DeviceBuffer<ftte_spectra_seg> spill;
    // the oblique rays (ftte_rays.cpp): a call's rays and their offsets, and a batch's records or segment list
    DeviceBuffer<double> ray_origin, ray_dir, ray_tmax, ray_tin, ray_tout;
    DeviceBuffer<int64_t> ray_offset, ray_leaf;
    DeviceBuffer<ftte_spectra_seg> ray_rec;

    void drop_velocity() { for (auto &v : vel) v.reset(); velocity_set = false; }
    void drop_grid()
    {
        drop_velocity();
        value.reset(); nseg.reset(); flags.reset(); column.reset(); tau.reset(); summary.reset(); spill.reset();
        for (int a = 0; a < 2; ++a) { base[a].reset(); frac[a].reset(); }
        ray_origin.reset(); ray_dir.reset(); ray_tmax.reset(); ray_tin.reset(); ray_tout.reset(); ray_offset.reset(); ray_leaf.reset(); ray_rec.reset();
    }
};

// Sightlines per launch so that what a batch stages stays under kSpectraWorkBytes: nvel doubles of tau per line where tau is
// staged, most_segments records per line where a line exceeds a chunk.  At least 1 (a single line may exceed the budget), at most nlines.
// (inline: tests/host/spectra_batch_check.cpp holds it without the context)
inline int64_t spectra_batch_lines(int64_t nlines, int64_t nvel, bool stage_tau, int64_t most_segments)
{
    if (nlines < 1) return 1;
    size_t per_line = 3 * sizeof(double);
    if (stage_tau) per_line += sizeof(double) * (size_t)(nvel > 0 ? nvel : 0);
    if (most_segments > kSpectraChunk) per_line += sizeof(ftte_spectra_seg) * (size_t)most_segments;
    const int64_t fit = (int64_t)(kSpectraWorkBytes / per_line);
    return fit < 1 ? 1 : fit < nlines ? fit : nlines;
}

// asynchronous on `stream`; 0, -1 bad argument, -2 launch failure
int launch_spectra_check(const SpectraRec &R, void *stream);
int launch_spectra(const SpectraRec &R, void *stream);

} // namespace ftte
