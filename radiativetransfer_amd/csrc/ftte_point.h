// ftte_point.h -- host side of the point-source path (rows P1-P3 of the scope table): the stellar rate
// tables (stellarBetaTable.f90), the table look-up (getRatesHydrogenHelium, equiSources.f90:4157-4311) and
// the long-characteristics tracer with HEALPix ray splitting (startNewLongRay, equiSources.f90:3120-3385).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>
#include <vector>

#include "ftte_amr.h"
#include "ftte_device.h"
#include "ftte_gas.h"
#include "ftte_internal.h"

namespace ftte {

constexpr int kFrequencies = 400;    // nfreq, stellarBetaTable.f90:14
constexpr int kSplitBatch = 1024;    // sources traced together; bounds the split queues (3072 records each)
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

// What the point-source path keeps on the device: the tree, the rate tables, the rates it adds into, the tracer's scratch.  Owned
// by the context.  The medium it traces through is the context's GasState (ftte_gas.h).
struct PointState {
    // the tree, uploaded on first use after ftte_set_grid (nothing is uploaded for a uniform grid)
    DeviceBuffer<NodeRec> node;
    bool tree_ready = false;
    std::vector<int32_t> node_of_leaf; // cell-array index -> node
    TableSets current, slots; // the tables every star of ftte_point_sources reads; the population slots
    DeviceBuffer<FreqBin> bins; // [populations of the call][kFrequencies - 1]
    DeviceBuffer<double> pixdir; // [kPixelCount][3]
    double rmax[30];
    // [ncell][kCellRec] krate24, krate25, krate26, crate24, crate25, crate26, 0, 0: what the tracer adds into
    DeviceBuffer<double> rates;
    int64_t rates_cells = 0;
    DeviceBuffer<double> rate_planes; // [6][ncell]: the layout of the interface, filled on request
    // tracer scratch
    DeviceBuffer<SplitRec> queue[2];
    DeviceBuffer<int32_t> counters; // [0] queue length, [2] error, [4..5] 64-bit count of cell crossings
    long long ray_steps = 0;     // of the last trace
    DeviceBuffer<int32_t> src_node;
    DeviceBuffer<int32_t> src_slot, src_highest; // [stars of the call]: the slot each reads, the highest pixel level each reached
    DeviceBuffer<double> src_ndot;
    DeviceBuffer<double> sample_in, sample_out;
    // escape bookkeeping of the last trace (startNewLongRay, equiSources.f90:3198-3233, 3336-3345): per star ndotRemaining[7],
    // ndotBoundary[7], ndotDust, ndotSpectrum[300]
    DeviceBuffer<double> escape;         // device, [stars of the call][kEscapeRec]
    std::vector<double> escape_host, escape_ndot; // the same on the host after the trace; the stars' photon rates
    DeviceBuffer<double> sigma_ratio;    // device [4][300]: outputSigma* / threshold cross-section (stellarBetaTable.f90:119-152)
    bool sigma_ready = false;

    void drop_grid(); // after ftte_set_grid: tree and rates belong to the old grid
};

// dustCrossSection, dustModule.f90:30-73 (SMC branch); a_smc is the Fortran array a_smc(7,5), lambda in micron
double dust_cross_section(double lambda_um, const double *a_smc);
// stellarPopulation, stellarPopulationModule.f90:7-50.  spec is the Fortran array specificLuminosity(nmetal,nspectrum,nwave)
double stellar_population(const double *spec, int nmetal, int nspectrum, int nwave, const double *wavelength, int iSpectrum,
                          double coefSpectrum, int iMetal, double coefMetal, double freq_ev);
// uvbBetaTable(nfreq, freqdel, alpha), uvbBetaTable.f90:3-305: group-averaged cross-sections beta[species HI, HeI, HeII][group],
// photo-rate coefficients ksi[group][24, 25, 26] and heating coefficients gamma[group][HI, HeI, HeII] of the three frequency groups
void uvb_beta_table(int nfreq, double freqdel, const double *alpha, double *beta, double *ksi, double *gamma);
// uniformTable(nfreq, freqdel, alphaQuasar, alphaStellar), uniformTable.f90:1-200: ksi[component quasar, stellar][24, 25, 26] and
// gamma[component][HI, HeI, HeII] of the two power-law components of the uniform background
void uniform_table(int nfreq, double freqdel, double alpha_quasar, double alpha_stellar, double *ksi, double *gamma);
// coll_rates (coll_rates.f:42-150): k1..k6 at temperature T; recombination_type 1 = case A, 2 = case B (definitionsModule.f90:48)
void coll_rates(double T, int recombination_type, double *k);
// k1a..k6a(nratec) as calc_rates.f:324-337 fills them, with the table bounds of equiSources.f90:174-176; k[6][nratec]
void rate_coefficient_tables(int nratec, double temstart, double temend, int recombination_type, double *k, double *logtem0,
                             double *logtem9, double *dlogtem);
// rmax(1:30), equiSources.f90:296-309
void rmax_table(double *rmax30);

// Each returns 0 or an ftte_status and fills *err.
int point_stellar_beta_table(PointState &P, hipStream_t stream, const double *a_smc, int nwave, const double *wavelength,
                             int nspectrum, int nmetal, const double *spec, int iSpectrum, double coefSpectrum, int iMetal,
                             double coefMetal, double *total_integral, std::string *err);
// npop populations into slots 0..npop-1 (earlier slots are replaced): the host work of point_stellar_beta_table per population,
// grid and cross-sections once, one launch for all tables; total_integral[npop] may be null
int point_stellar_beta_tables(PointState &P, hipStream_t stream, const double *a_smc, int nwave, const double *wavelength,
                              int nspectrum, int nmetal, const double *spec, int npop, const int *iSpectrum, const double *coefSpectrum,
                              const int *iMetal, const double *coefMetal, double *total_integral, std::string *err);
int point_set_population_tables(PointState &P, hipStream_t stream, int npop, const double *tables, std::string *err);
int point_set_tables(PointState &P, hipStream_t stream, const double *tables, std::string *err);
// set k of S (the caller has checked that there is one) to the host
int point_get_tables(const TableSets &S, hipStream_t stream, int k, double *tables, std::string *err);
int point_lookup(PointState &P, hipStream_t stream, int dust, int nsample, const double *tau, double *rates, std::string *err);
// fills the gas: field[5] = HI, HeI, HeII, rho, abun2 on the host or the device; rho and abun2 may be null (zeros)
int point_set_medium(GasState &G, hipStream_t stream, int64_t ncell, const double *const field[5], bool on_device, int dust,
                     std::string *err);
int point_zero_rates(PointState &P, hipStream_t stream, int64_t ncell, std::string *err);
// rates in the interface's layout [6][ncell], in device memory (valid until the next trace)
int point_rate_planes(PointState &P, hipStream_t stream, double **planes, std::string *err);
int point_set_rates(PointState &P, hipStream_t stream, int64_t ncell, const double *planes_host, std::string *err);
// PointState::node holds the tree (the tracer and the maps of ftte_analysis.cpp descend through it); no-op once uploaded
int point_ensure_tree(PointState &P, hipStream_t stream, const AmrTree &tree, std::string *err);
// src_slot[nsrc]: the population slot each star reads, or null: all read the current tables.  highest_pixel_level: the maximum
// over the stars; highest_per_star[nsrc]: each star's own.  Either may be null.  Makes the gas's packed copy where it is not current.
int point_trace(PointState &P, GasState &G, hipStream_t stream, const AmrTree &tree, double box, int nsrc, const int64_t *src_cell,
                const double *src_ndot, const int32_t *src_slot, int *highest_pixel_level, int *highest_per_star, std::string *err);
// outputSigma24, 25, 26, Dust [4][300] (absolute cross-sections, as the reference's module arrays hold them)
int point_set_output_sigma(PointState &P, hipStream_t stream, const double *sigma, std::string *err);

} // namespace ftte
