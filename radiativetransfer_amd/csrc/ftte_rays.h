// ftte_rays.h -- absorption spectra along oblique rays through the refined grid: a unit of the spectra family (ftte_spectra.h).  The
// ray walk is stated in ftte_ray_math.h, the line in ftte_spectra_math.h.  Here: the record the kernels of ftte_rays.hip read and the
// context-free batch rule.  The working memory is SpectraState's (ftte_spectra.h).
#pragma once

#include <cstddef>
#include <cstdint>

#include "ftte_node_rec.h"
#include "ftte_ray_math.h"
#include "ftte_spectra.h"

namespace ftte {

static_assert(sizeof(ftte_ray_node) == sizeof(NodeRec) && offsetof(ftte_ray_node, child0) == offsetof(NodeRec, child0) &&
                  offsetof(ftte_ray_node, leaf) == offsetof(NodeRec, leaf),
              "the walk reads NodeRec");

constexpr size_t kRaySegmentListBytes = sizeof(int64_t) + 2 * sizeof(double); // (leaf, t_in, t_out) of ftte_ray_segments

// One call's rays, tree and medium, shared by the two kernels
struct RayRec {
    const NodeRec *node;                // nullptr on a uniform grid
    const double *origin, *dir, *tmax;  // [nray][3], [nray][3], [nray] or nullptr
    int64_t nray;
    int32_t n;
    int64_t max_steps;                  // ray_step_bound, or ray_step_bound_periodic of the longest ray
    const double *value, *tgas;         // [ncell], or both nullptr (ftte_ray_segments: the geometry alone)
    const double *velx, *vely, *velz;   // [ncell] each, or nullptr: zero
    double cell_cm;
    ftte_spectra_par par;
    ftte_consts K;
    // count mode, all rays: per ray its segments and N; flags[0] a leaf without a line width, flags[1] the most segments,
    // flags[2] a walk beyond max_steps
    int32_t *nseg;                      // [nray]
    double *column;                     // [nray]
    int32_t *flags;                     // [3], zero before the launch
    // fill mode and the spectra: rays ray0 .. ray0 + nrays - 1; ray r's segments lie at offset[r] - offset[ray0]
    const int64_t *offset;              // [nray + 1]
    int64_t ray0;
    int32_t nrays, nvel;
    ftte_spectra_seg *rec;              // or nullptr
    int64_t *leaf;                      // the segment list, or three nullptr
    double *t_in, *t_out;
    double *tau;                        // [nrays][nvel], ray0's first
    double *summary;                    // [nrays][3] or nullptr
    int32_t periodic;                   // the walk wraps through the box's opposite face up to tmax (which is then required)
};

// Rays per launch from ray0 on so that what the batch keeps stays under kSpectraWorkBytes: per_segment bytes for every segment of
// its rays (offset[nray + 1]: the prefix sum of the counts), three doubles of summaries per ray, nvel doubles of tau per ray where
// tau is staged.  At least 1 (a single ray may exceed the budget), at most nray - ray0.
// (inline: tests/host/ray_batch_check.cpp holds it without the context)
inline int64_t ray_batch_rays(const int64_t *offset, int64_t nray, int64_t ray0, int64_t nvel, bool stage_tau, size_t per_segment)
{
    if (nray < 1 || ray0 < 0 || ray0 >= nray) return 1;
    const size_t per_ray = 3 * sizeof(double) + (stage_tau ? sizeof(double) * (size_t)(nvel > 0 ? nvel : 0) : 0);
    int64_t m = 0;
    while (ray0 + m < nray) {
        const size_t bytes = (size_t)(offset[ray0 + m + 1] - offset[ray0]) * per_segment + (size_t)(m + 1) * per_ray;
        if (bytes > kSpectraWorkBytes) break;
        ++m;
    }
    return m < 1 ? 1 : m;
}

// asynchronous on `stream`; 0, -1 bad argument, -2 launch failure
int launch_ray_walk(const RayRec &R, bool fill, void *stream);
int launch_ray_spectra(const RayRec &R, void *stream);

} // namespace ftte
