// ftte_analysis.h -- the reference's analysis modes on the device-resident medium: the slice map of its reader tool
// (readCellArray.f90:116-140, sliceCell :189-230), the mass-weighted projection of mode initialConfiguration (equiSources.f90:678-731,
// projectVariableToMap :4914-4954), the clumping factor (:661-676, computeClumping :4711-4735) and the gas PDF (:814-822,
// computeGasPDF :4682-4709).  Here: what the context keeps for them (AnalysisState), the records the kernels of ftte_analysis.hip
// read, and the context-free arithmetic of the map axes (ftte_analysis.cpp).
#pragma once

#include <cstdint>

#include "ftte_device.h"
#include "ftte_node_rec.h"

namespace ftte {

constexpr int kPdfBins = 50;            // npdf, definitionsModule.f90:64
constexpr int kPdfSlots = kPdfBins + 1; // the bins and `outside`
constexpr int kPdfLevels = 64;          // levels a census can tell apart (ftte_set_grid accepts trees 60 deep)
constexpr int kMapLevels = 64;          // and a projection
constexpr int kClumpBlocks = 1024;      // workgroups of the clumping census: [3][kClumpBlocks] partial sums, then the 3 totals
constexpr int kClumpParts = 3 * kClumpBlocks + 3;

// How the map's axes lie in storage for an izone (rotateIndices): storage index a = 0, 1, 2 (icell, jcell, kcell; kcell is
// contiguous) takes sweep index src[a] (0 = the map's first axis, 1 = its second, 2 = the depth), mirrored where mirror[a].
// child[4 (i-1) + 2 (j-1) + (k-1)] is the storage position 4 (a-1) + 2 (b-1) + (c-1) of the child a refined cell's sweep child
// (i, j, k) is: the is/js/ks arrays of the drivers (equiSources.f90:690-696, readCellArray.f90:116-122).
struct MapZone {
    int32_t src[3];
    int32_t mirror[3];
    int32_t child[8];
};

// One map.  Pixel (i, j), 0-based, is map[i + nxmap * j]: the reference's mapArray(nxmap, nymap).
struct MapRec {
    const NodeRec *node;   // nullptr on a uniform grid: base cell == leaf
    const double *value;   // [ncell]
    const double *rho;     // [ncell] (projection)
    const int32_t *ibase, *jbase; // [nxmap], [nymap]: i0, j0, 1-based
    const double *ifrac, *jfrac;  // xnew, ynew
    float *map;
    MapZone zone;
    int32_t n, nxmap, nymap;
    int32_t fast_is_j;     // neighbouring lanes are neighbours along the map's second axis (else along its first)
    int32_t kbase;         // slice: k0, 1-based
    double kfrac;          // slice: znew
    int32_t kstart, kend;  // projection: base cells along the depth, 1-based, inclusive
    int32_t mode;          // projection: 0 the reference's mass-weighted mean, 1 the path integral
    double cell_cm;        // physicalBoxSize / dfloat(nx)
    int32_t levels;        // levels of the tree: a leaf lies at most levels - 1 deep
    // projection: (cellSizeAbsoluteUnits/1.e21)**3 of a leaf `depth` refinements below a base cell, :4945 and :4948 -- the size
    // halved level by level, divided by the widened single-precision literal, multiplied out -- made once on the host
    double cube[kMapLevels];
};

struct ClumpRec {
    const int8_t *level;
    const double *rho;
    int64_t ncell;
    double *part; // [kClumpParts]
};

struct PdfRec {
    const int8_t *level;
    const double *rho;
    int64_t ncell;
    int32_t nlev;               // levels of the tree, at most kPdfLevels
    unsigned long long *counts; // [kPdfSlots][nlev], zero before the launch
};

// What the analysis keeps on the device.  Owned by the context; dropped with the grid.
struct AnalysisState {
    DeviceBuffer<float> map;
    DeviceBuffer<int32_t> base[2];
    DeviceBuffer<double> frac[2];
    DeviceBuffer<double> value;   // a host value array on its way to the kernel
    DeviceBuffer<double> sums;    // clumping: kClumpParts
    DeviceBuffer<unsigned long long> counts; // gas PDF: [kPdfSlots][levels]
    DeviceBuffer<int64_t> cells;  // star PDF: the stars' leaves
    DeviceBuffer<double> picked;  // star PDF: rho and HI of those leaves

    void drop_grid()
    {
        map.reset(); value.reset(); sums.reset(); counts.reset(); cells.reset(); picked.reset();
        for (int a = 0; a < 2; ++a) { base[a].reset(); frac[a].reset(); }
    }
};

// MapZone of an izone, and along which map axis neighbouring lanes should be neighbours: the one that feeds the contiguous storage
// index where a map axis does, else the one that feeds the next.  false: izone outside 1..24.
bool map_zone(int izone, MapZone *Z, int *fast_is_j);
// i0 and xnew of the map's columns (or rows), context-free.  quotient_first: the reader's form, the single-precision quotient
// (float(i)-0.5)/float(nmap) widened (readCellArray.f90:126), inside the window; else the driver's, left to right in double
// (equiSources.f90:703).  0, or -1 where an argument is bad or a base index leaves 1..n (the reference indexes out of bounds there).
int map_axis(int n, int nmap, double centre, double zoom, bool quotient_first, int32_t *base, double *frac);
// kstart and kend of the projection (equiSources.f90:687-700)
int map_depth(int n, double centre, double zoom, int32_t *kstart, int32_t *kend);
// the bin of computeGasPDF (:4700-4706) from tmp = log10(rho/msun*pc**3): 0..49, or kPdfBins for `outside` (rho = 0 and NaN too)
#if defined(__HIPCC__)
__host__ __device__ __forceinline__
#else
static inline
#endif
int pdf_bin(double tmp)
{
    const double apdf = -8.0, bpdf = 3.0; // definitionsModule.f90:65
    if (!(tmp > apdf && tmp < bpdf)) return kPdfBins;
    const int b = (int)((tmp - apdf) / (bpdf - apdf) * (double)(float)kPdfBins);
    return b < 0 ? 0 : b >= kPdfBins ? kPdfBins - 1 : b;
}

// asynchronous on `stream`; 0, -1 bad argument, -2 launch failure
int launch_slice_map(const MapRec &R, void *stream);
int launch_project_map(const MapRec &R, void *stream);
int launch_clumping(const ClumpRec &R, void *stream);
int launch_gas_pdf(const PdfRec &R, void *stream);

} // namespace ftte
