// ftte_gas.h -- GasState: the species medium the point-source tracer, the chemistry, the opacities and the thin limit share (HI,
// HeI, HeII, rho, abun2 in cell-array order), with the packed copy the tracer reads.  The species have a version and the packed copy
// remembers the version it was made from, as a MediumField's copies do (ftte_medium.h): whoever writes the species says
// species_changed(), and the tracer asks packed_current().  Launches nothing and copies nothing: point_set_medium fills it.
// ChemState: what the per-leaf updates (ftte_leaf_pass.cpp) and the expansion of HII regions (ftte_chem.cpp) keep beside the gas.
#pragma once

#include <cstdint>

#include <vector>

#include "ftte_device.h"
#include "ftte_expansion.h"

namespace ftte {

class GasState {
public:
    enum { kHI, kHeI, kHeII, kRho, kAbun2, kFields };
    double *field(int f) const { return field_[f]; }
    int dust() const { return dust_; } // dustApproximation of the last fill
    bool ready(int64_t ncell) const { return cells_ > 0 && cells_ == ncell; }
    bool ready_with_density(int64_t ncell) const { return ready(ncell) && density_; } // (the chemistry and the census need rho)
    bool ready_with_abundance(int64_t ncell) const { return ready(ncell) && abundance_; } // (the star catalogue's abun2)

    // Room for a fill of ncell cells, which starts here: the packed copy is stale.  For another cell count everything is released
    // first and the gas is not ready until filled(); for the same one the buffers, the packed copy's among them, stay.  On failure
    // the gas is empty.
    hipError_t reserve(int64_t ncell)
    {
        species_changed();
        if (cells_ != ncell) drop();
        for (auto &f : field_) {
            const hipError_t e = f.reserve((size_t)ncell);
            if (e != hipSuccess) { drop(); return e; }
        }
        return hipSuccess;
    }
    void filled(int64_t ncell, int dust, bool density, bool abundance = false)
    {
        cells_ = ncell; dust_ = dust; density_ = density; abundance_ = abundance;
    }
    void species_changed() { ++version_; } // the packed copy is stale
    void drop()                            // another grid: nothing of the old one is kept
    {
        for (auto &f : field_) f.reset();
        packed_.reset();
        packed_from_ = kNever;
        cells_ = 0;
        density_ = abundance_ = false;
    }

    // the tracer's copy, [cells][cell_rec]: room (a new buffer holds nothing), then the launch, then packed_made()
    double *packed() const { return packed_; }
    hipError_t reserve_packed(int cell_rec)
    {
        bool fresh = false;
        const hipError_t e = packed_.reserve((size_t)cell_rec * (size_t)cells_, &fresh);
        if (fresh || e != hipSuccess) packed_from_ = kNever;
        return e;
    }
    bool packed_current() const { return packed_ && packed_from_ == version_; }
    void packed_made() { packed_from_ = version_; }

private:
    static constexpr long long kNever = -1;
    DeviceBuffer<double> field_[kFields], packed_;
    int64_t cells_ = 0; // of the last fill; 0: none
    int dust_ = 0;
    bool density_ = false; // that fill brought a density
    bool abundance_ = false; // ... and an abun2
    long long version_ = 0, packed_from_ = kNever;
};

// ionisation equilibrium (solveRateEquations, initialIonizationEquilibrium, computeMass) and thermal balance
struct ChemState {
    DeviceBuffer<int8_t> level;   // per leaf, uploaded on first use after ftte_set_grid
    DeviceBuffer<double> k;       // [6][nratec]
    int nratec = 0;
    double logtem0 = 0, logtem9 = 0, dlogtem = 0;
    DeviceBuffer<double> logtem;  // [ncell] log of the gas temperature
    bool temperature_set = false;
    DeviceBuffer<double> out, J;  // out: as many planes [ncell] as the update declares (leaf_pass); J: [3][ncell]
    DeviceBuffer<unsigned long long> counters; // first bad cell, bits of the largest change, bisection steps, then the update's own words
    long long steps = 0;          // of the last update
    DeviceBuffer<double> mass;    // computeMass: per-workgroup partial sums, then the two totals (kMassParts)
    // expansion of HII regions (ftte_expansion.h): where each leaf of a refined cell array lies, uploaded on first use after
    // ftte_set_grid like `level`, with each leaf's tree node on the host; the stars of the last call; its exact star-leaf tests
    DeviceBuffer<LeafPos> leaf_pos;
    std::vector<int32_t> leaf_node;
    DeviceBuffer<ExpStar> exp_star;
    DeviceBuffer<ExpStarTest> exp_test;
    DeviceBuffer<int64_t> exp_cells;
    long long expansion_tests = 0;
    // thermal balance (thermalEquilibrium and the temperature step, ftte_thermal_math.h): the temperature itself beside its
    // logarithm, the cooling coefficients on the rate coefficients' temperature grid ([13][nratec], or node-major [nratec][16]:
    // cool_node_major, for measurements), Compton's two numbers, and hydroHeating per leaf once a thermal-equilibrium pass has run on this grid
    DeviceBuffer<double> tgas, cool, hydro;
    bool cool_node_major = false, hydro_set = false;
    double comp1 = 0, comp2 = 0;
    // the coupled step (ftte_thermochem_math.h): the subcycles each leaf took in the last call that got through on this grid, and
    // the buffer the kernel writes them into (copied in, like `out`, once no leaf has failed)
    DeviceBuffer<int32_t> subcycles, subcycles_out;
    bool subcycles_set = false;
    // the diffuse recombination source (ftte_recombination.cpp): the ground-state recombination coefficients [3][nratec] on the rate
    // coefficients' temperature grid, the pass's two words (first bad leaf, lost (leaf, group) pairs), and S [3][ncell] on its way
    // into an emission field whose contents are in force
    DeviceBuffer<double> ground, ground_out;
    DeviceBuffer<unsigned long long> ground_words;

    void drop_grid() // after ftte_set_grid: what is sized by the old grid; the rate and cooling coefficients stay
    {
        level.reset(); logtem.reset(); out.reset(); J.reset(); leaf_pos.reset(); tgas.reset(); hydro.reset();
        subcycles.reset(); subcycles_out.reset(); ground_out.reset();
        leaf_node.clear();
        temperature_set = hydro_set = subcycles_set = false;
    }
};

} // namespace ftte
