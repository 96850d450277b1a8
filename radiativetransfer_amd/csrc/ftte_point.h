// ftte_point.h -- host side of the point-source path (rows P1-P3 of the scope table): the stellar rate
// tables (stellarBetaTable.f90), the table look-up (getRatesHydrogenHelium, equiSources.f90:4157-4311) and
// the long-characteristics tracer with HEALPix ray splitting (startNewLongRay, equiSources.f90:3120-3385).
// What the path keeps has one owner each: RateTables, PointRates, TraceScratch, EscapeRecord; PointState is their composition.
// The tables' mathematics is ftte_tables.h, the tree on the device the context's DeviceTree (ftte_device_tree.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "ftte_amr.h"
#include "ftte_device.h"
#include "ftte_device_tree.h"
#include "ftte_gas.h"
#include "ftte_point_rec.h"
#include "ftte_tables.h"

namespace ftte {

constexpr int kSplitBatch = 1024;    // sources traced together; bounds the split queues
constexpr int kSplitsPerSource = 12 * 4 * 4 * 4 * 4; // split records one source can queue: its 12 * 4^4 rays that split into level 6
constexpr size_t kSetDoubles = (size_t)6 * kTableSize; // one set of rate tables, and as many logarithms

// `count` sets of rate tables side by side, [count][6][11^4], and their logarithms.  Used twice: the current tables (count 0 or 1)
// and the population slots, for stars that name the slot they read.
struct TableSets {
    DeviceBuffer<double> tables, logtab;
    int count = 0; // sets that hold what was put there last: 0 from the moment a buffer is replaced until the new ones are filled

    // Room for n sets.  Buffers that have it stay, and the sets in them; on failure nothing is held.
    hipError_t reserve(int n)
    {
        const size_t want = (size_t)n * kSetDoubles;
        if (tables.capacity() < want || logtab.capacity() < want) count = 0;
        hipError_t e = tables.reserve(want);
        if (e == hipSuccess) e = logtab.reserve(want);
        if (e != hipSuccess) { tables.reset(); logtab.reset(); count = 0; }
        return e;
    }
};

// The rate tables: the set every star of ftte_point_sources reads (`current`), the population slots, and the output cross-sections
// that belong to the current tables.  Each call returns 0 or an ftte_status and fills *err.
class RateTables {
public:
    // the set a trace reads: the slots where its stars name them, else the current tables
    const TableSets &by_slot(bool slots) const { return slots ? slots_ : current_; }
    int slot_count() const { return slots_.count; } // population slots held
    // 0, or FTTE_ERR_STATE and its text where that set holds nothing
    int missing(bool slots, std::string *err) const;
    // [4][300] outputSigma* / threshold cross-section (stellarBetaTable.f90:119-152) on the device, or null: none known
    const double *sigma() const { return sigma_ready_ ? sigma_ratio_.get() : nullptr; }

    // ftte_set_output_sigma: sigma[4][300], absolute cross-sections as the reference's module arrays hold them
    int set_sigma(hipStream_t stream, const double *sigma, std::string *err);
    // ftte_set_rate_tables: the cross-sections belonged to the population whose tables these replace, so none is known afterwards
    int set_current(hipStream_t stream, const double *tables, std::string *err);
    // ftte_stellar_beta_table: the population's bins [kFrequencies - 1] and its cross-sections come together
    int current_from_bins(hipStream_t stream, const std::vector<FreqBin> &bins, const double *sigma, std::string *err);
    // npop populations into slots 0..npop-1 (earlier slots are replaced), one launch for all tables
    int slots_from_bins(hipStream_t stream, const std::vector<FreqBin> &bins, int npop, const double *sigma, std::string *err);
    int set_slots(hipStream_t stream, int npop, const double *tables, std::string *err);
    // set k of by_slot(slots) (the caller has checked that there is one) to the host
    int get(hipStream_t stream, bool slots, int k, double *tables, std::string *err) const;

private:
    int reserve_slots(int npop, bool with_bins, std::string *err);
    int fill_from_bins(TableSets &S, hipStream_t stream, const std::vector<FreqBin> &bins, int n, std::string *err);
    int fill_from_host(TableSets &S, hipStream_t stream, const double *tables, int n, std::string *err);

    TableSets current_, slots_;
    DeviceBuffer<FreqBin> bins_; // [populations of the call][kFrequencies - 1]
    DeviceBuffer<double> sigma_ratio_;
    bool sigma_ready_ = false;
};

// What the tracer adds into, [ncell][kCellRec]: krate24, krate25, krate26, crate24, crate25, crate26, 0, 0; and the same in the
// layout of the interface, [6][ncell], made on request.
class PointRates {
public:
    bool ready(int64_t ncell) const { return rates_ && cells_ == ncell; }
    double *packed() const { return rates_; }
    // zeros for ncell cells (asynchronous); another cell count releases the planes too
    int zero(hipStream_t stream, int64_t ncell, std::string *err);
    // the planes in device memory (asynchronous; valid until the next trace)
    int planes(hipStream_t stream, double **planes, std::string *err);
    int set(hipStream_t stream, int64_t ncell, const double *planes_host, std::string *err);
    void drop()
    {
        rates_.reset(); planes_.reset();
        cells_ = 0;
    }

private:
    DeviceBuffer<double> rates_, planes_;
    int64_t cells_ = 0;
};

// The tracer's scratch on the device
struct TraceScratch {
    enum { kQueueLength = 0, kError = 2, kSteps = 4, kCounters = 8 }; // `counters`: [4..5] is the 64-bit count of cell crossings
    DeviceBuffer<SplitRec> queue[2];
    DeviceBuffer<int32_t> counters;
    DeviceBuffer<int32_t> src_node;
    DeviceBuffer<double> src_ndot;
    DeviceBuffer<int32_t> src_slot, src_highest; // [stars of the call]: the slot each reads, the highest pixel level each reached
    DeviceBuffer<double> escape;                 // [stars of the call][kEscapeRec]

    // Room for a trace of nsrc stars (by_slot: that name their slots).  Returns the stars of a batch, or 0 and the reason in *why.
    int reserve(int nsrc, bool by_slot, hipError_t *why)
    {
        const int batch = nsrc < kSplitBatch ? nsrc : kSplitBatch;
        hipError_t e = counters.reserve(kCounters);
        for (auto &q : queue)
            if (e == hipSuccess) e = q.reserve((size_t)batch * kSplitsPerSource);
        if (e == hipSuccess) e = src_node.reserve((size_t)batch);
        if (e == hipSuccess) e = src_ndot.reserve((size_t)batch);
        if (e == hipSuccess && by_slot) e = src_slot.reserve((size_t)nsrc);
        if (e == hipSuccess) e = src_highest.reserve((size_t)nsrc);
        if (e == hipSuccess) e = escape.reserve((size_t)nsrc * kEscapeRec);
        *why = e;
        return e == hipSuccess ? batch : 0;
    }
};

// The escape bookkeeping of the last trace on the host (startNewLongRay, equiSources.f90:3198-3233, 3336-3345): per star
// ndotRemaining[7], ndotBoundary[7], ndotDust, ndotSpectrum[300]; the stars' photon rates; the cell crossings
class EscapeRecord {
public:
    int stars() const { return (int)ndot_.size(); }
    long long ray_steps() const { return steps_; }
    // a trace of nsrc stars ends: where its records go; then the crossings it counted
    double *receive(int nsrc, const double *src_ndot)
    {
        rec_.resize((size_t)nsrc * kEscapeRec);
        ndot_.assign(src_ndot, src_ndot + nsrc);
        return rec_.data();
    }
    void counted(long long steps) { steps_ = steps; }
    // star s into element s of the outputs (remaining, boundary, fraction [stars][7]; dust [stars]; spectrum [stars][300]), each
    // of which may be null
    void unpack(int s, double *remaining, double *boundary, double *dust, double *spectrum, double *fraction) const
    {
        const double *E = rec_.data() + (size_t)s * kEscapeRec, *B = E + kOutputRadii;
        for (int ir = 0; ir < kOutputRadii; ++ir) {
            if (remaining) remaining[s * kOutputRadii + ir] = E[ir];
            if (boundary) boundary[s * kOutputRadii + ir] = B[ir];
            // equiSources.f90:1342-1348
            if (fraction) fraction[s * kOutputRadii + ir] = B[ir] < 1. ? E[ir] / (ndot_[(size_t)s] - B[ir]) : 0.;
        }
        if (dust) dust[s] = E[2 * kOutputRadii];
        if (spectrum) std::copy(E + 2 * kOutputRadii + 1, E + kEscapeRec, spectrum + (size_t)s * kOutputEnergies);
    }

private:
    std::vector<double> rec_, ndot_;
    long long steps_ = 0;
};

// What the point-source path keeps.  Owned by the context.  The medium it traces through is the context's GasState (ftte_gas.h),
// the tree its DeviceTree.
struct PointState {
    RateTables tables;
    PointRates rates;
    TraceScratch scratch;
    EscapeRecord escape;
    DeviceBuffer<double> pixdir; // [kPixelCount][3], made by the first trace, and rmax with it
    double rmax[30];
    DeviceBuffer<double> sample_in, sample_out; // the look-up's samples

    void drop_grid() { rates.drop(); } // after ftte_set_grid: the rates belong to the old grid
};

// Each returns 0 or an ftte_status and fills *err.
int point_stellar_beta_table(RateTables &R, hipStream_t stream, const double *a_smc, int nwave, const double *wavelength,
                             int nspectrum, int nmetal, const double *spec, int iSpectrum, double coefSpectrum, int iMetal,
                             double coefMetal, double *total_integral, std::string *err);
// npop populations into slots 0..npop-1: the host work of point_stellar_beta_table per population, grid and cross-sections once;
// total_integral[npop] may be null
int point_stellar_beta_tables(RateTables &R, hipStream_t stream, const double *a_smc, int nwave, const double *wavelength,
                              int nspectrum, int nmetal, const double *spec, int npop, const int *iSpectrum, const double *coefSpectrum,
                              const int *iMetal, const double *coefMetal, double *total_integral, std::string *err);
int point_lookup(PointState &P, hipStream_t stream, int dust, int nsample, const double *tau, double *rates, std::string *err);
// fills the gas: field[5] = HI, HeI, HeII, rho, abun2 on the host or the device; rho and abun2 may be null (zeros)
int point_set_medium(GasState &G, hipStream_t stream, int64_t ncell, const double *const field[5], bool on_device, int dust,
                     std::string *err);

// The tracer's steps that read no device (point_trace goes through them; tests/host/point_state_check.cpp drives them).
// The node of every star's cell into node[nsrc], or FTTE_ERR_ARG: a cell outside the cell array, or (slot not null) a star that
// names a slot outside 0..nslots-1.
int check_sources(const DeviceTree &D, int64_t ncell, int nsrc, const int64_t *cell, const int32_t *slot, int nslots, int32_t *node,
                  std::string *err);
// rays of a launch: level 1 starts 12 per star, every later level 4 per split record of the level before
inline int32_t rays_of_level(int level, int stars, int32_t records) { return level == 1 ? 12 * stars : 4 * records; }
const char *trace_error_text(int code); // what the kernel's error word says

// src_slot[nsrc]: the population slot each star reads, or null: all read the current tables.  highest_pixel_level: the maximum
// over the stars; highest_per_star[nsrc]: each star's own.  Either may be null.  Makes the rates, the device tree and the gas's
// packed copy where they are not current.
int point_trace(PointState &P, DeviceTree &D, GasState &G, hipStream_t stream, const AmrTree &tree, double box, int nsrc,
                const int64_t *src_cell, const double *src_ndot, const int32_t *src_slot, int *highest_pixel_level, int *highest_per_star,
                std::string *err);

} // namespace ftte
