// ftte_point_rec.h -- records and launch wrappers of ftte_point.hip: the tracer's split queue and launch record, the packed medium
// and rates.  Plain structs; the launches are asynchronous on `stream` and return 0, -1 bad argument, -2 launch failure.  The host
// side is ftte_point.h, the table constants and FreqBin are ftte_tables.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "ftte_node_rec.h"
#include "ftte_tables.h"

namespace ftte {

// A ray waiting to be split into its four daughter pixels (startNewLongRay, equiSources.f90:3280-3383)
struct SplitRec {
    double pos[3];   // absolute position of the split point, box units (absoluteCoordinates)
    double radius;   // base-cell units
    double depth[4]; // tau1, tau2, tau3, tauDust accumulated so far
    double ndot;     // photons/s carried by the parent ray
    int32_t pixel;   // parent's NESTED index at its level
    int32_t src;     // which star of the batch the ray belongs to (its escape record)
};

// What the tracer touches per cell crossing is packed so that each kind of datum is one 64-byte line (or less):
// the rays of a wavefront are in 64 different places of the grid, and every separate array is another line from HBM.
constexpr int kCellRec = 8; // doubles per cell in the packed medium {HI, HeI, HeII, rho, abun2, 0, 0, 0} and in the packed
                            // rates {krate24, krate25, krate26, crate24, crate25, crate26, 0, 0}

struct TraceRec {
    const NodeRec *node;   // nullptr on a uniform grid: node == cell, level 0, no children
    int32_t n;
    int32_t dust;     // dustApproximation: 0 none, 1 ~HI, 2 ~total H
    int64_t ncell;
    double box;
    const double *medium;  // [ncell][kCellRec]
    const double *logtab;  // [3][11^4][2] natural logs of the rate tables, (number, heating) pairs; with slot_of: slot 0's
    const int32_t *slot_of; // [sources of this batch] population slot each star reads, or nullptr: all read `logtab`
    int64_t slot_stride;   // doubles between the slots' log tables
    const double *pixdir;  // [kPixelCount][3] unit vectors of all pixels of levels 1..6
    double rmax[kMaxPixelLevel + 1];
    double *rates;         // [ncell][kCellRec]
    // this launch: rays of `pixel_level`
    int32_t pixel_level;
    int32_t nrays;         // level 1: 12 * nsources; else 4 * number of split records
    const int32_t *src_node;  // level 1: host leaf node of each source
    const double *src_ndot;
    const SplitRec *in;    // level > 1
    SplitRec *out;         // rays of this level that split
    int32_t *out_count;
    int32_t out_capacity;
    int32_t *highest_level;    // [sources of this batch] highest pixel level each star's rays reached
    int32_t *error;
    unsigned long long *steps; // cell crossings, all rays (instrumentation)
    // escape bookkeeping
    double *escape;            // [sources of this batch][kEscapeRec], accumulated with atomics
    const double *sigma_ratio; // [4][300]: outputSigma24/6.30e-18, outputSigma25/1.58e-18, outputSigma26/7.42e-18, outputSigmaDust/5.41e-22,
                               // or nullptr (no cross-sections known: ndotSpectrum stays zero)
    double out_radius_kpc[kOutputRadii]; // outputRadius, equiSources.f90:10
    double kpc;
};

// point sources: table accumulation (P3), logs of user tables, one pixel level of the tracer (P1 + P2)
// npop populations side by side: bins[npop][nbins] -> tables[npop][6][11^4], logtab[npop][3][11^4][2], one launch
int launch_rate_table(const FreqBin *bins, int nbins, int npop, double *tables, double *logtab, hipStream_t stream);
int launch_rate_lookup(const double *logtab, int dust, int nsample, const double *tau, double *out, hipStream_t stream);
int launch_log_table(const double *tables, int npop, double *logtab, hipStream_t stream);
int launch_point_trace(const TraceRec &T, hipStream_t stream);
int launch_pack_medium(const double *const field[5], double *packed, long ncell, hipStream_t stream);
int launch_repack_rates(double *planes, double *packed, long ncell, bool to_packed, hipStream_t stream);

} // namespace ftte
