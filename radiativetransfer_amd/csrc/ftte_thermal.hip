// ftte_thermal.hip -- the kernels behind the thermal per-leaf updates (ftte_leaf_pass.cpp): the thermal balance of every leaf
// (thermalEquilibrium, equiSources.f90:3870-4042) and its temperature advanced over a time step.  The thermal balance of a cell
// is ftte_thermal_math.h, compiled here for the device and by the tests' host library for the host; a kernel is the loop over the
// leaves, the leaf's loads, one call into that header, the leaf's stores into the `out` buffers (copied in by the host once no leaf
// has failed), and the fold of its statistics (all of ftte_leaf.h).
#include <hip/hip_runtime.h>

#include "ftte_leaf.h"
#include "ftte_thermal_math.h"

namespace ftte {

// thermalEquilibrium per leaf (thermal_equilibrium_cell), at ftte_log of the leaf's temperature.  A leaf whose temperature is not
// positive and finite, or whose results are not finite, fails.
__global__ void __launch_bounds__(256) thermal_equilibrium_kernel(const ThermalRec R)
{
    LeafWords<0, 1> w;
    const ChemTable T = {nullptr, R.nratec, R.logtem0, R.logtem9, R.dlogtem};
    const ThermalTable C = {R.cool, (long)R.coef_stride, (long)R.node_stride};
    FTTE_FOR_LEAVES(c, R.ncell) {
        double p24, p25, p26, heating = 0., cooling = 0., hydro = 0.;
        load_point_rates(R.crate, c, 3, p24, p25, p26);
        const double tgas = R.tgas[c];
        int ok = tgas > 0. && thermal_finite(tgas);
        if (ok) {
            hydro = thermal_equilibrium_cell(&T, &C, R.rho[c], tgas, ftte_log(&R.K, tgas), R.HI[c], R.HeI[c], R.HeII[c],
                                             chem_cell_volume(R.box, R.level[c], R.n), R.crate != nullptr, p24, p25, p26,
                                             R.run_uvb ? R.J + c : nullptr, R.ncell, R.gamma, R.uniform, R.threshold, R.comp1, R.comp2, &heating,
                                             &cooling);
            ok = thermal_finite(heating) && thermal_finite(cooling) && thermal_finite(hydro);
        }
        if (!ok) note_bad(w.bad, c);
        else { R.out0[c] = heating; R.out1[c] = cooling; R.out2[c] = hydro; }
    }
    fold_head_words(w, R.first_bad, R.max_change, R.steps);
}

// the temperature of every leaf advanced over R.dt in R.substeps implicit steps at the rates of the state on entry (thermal_advance_cell)
__global__ void __launch_bounds__(256) thermal_advance_kernel(const ThermalRec R)
{
    LeafWords<1, 1> w;
    const ChemTable T = {nullptr, R.nratec, R.logtem0, R.logtem9, R.dlogtem};
    const ThermalTable C = {R.cool, (long)R.coef_stride, (long)R.node_stride};
    FTTE_FOR_LEAVES(c, R.ncell) {
        double p24, p25, p26, T1, logtem1, change;
        load_point_rates(R.crate, c, 3, p24, p25, p26);
        unsigned long long steps;
        const int ok = thermal_advance_cell(&R.K, &T, &C, R.rho[c], R.tgas[c], R.HI[c], R.HeI[c], R.HeII[c], chem_cell_volume(R.box, R.level[c], R.n),
                                            R.crate != nullptr, p24, p25, p26, R.run_uvb ? R.J + c : nullptr, R.ncell, R.gamma, R.uniform,
                                            R.threshold, R.comp1, R.comp2, R.hydro ? R.hydro[c] : 0., R.dt, R.substeps, R.tmin, R.tmax, &T1,
                                            &logtem1, &steps, &change);
        w.sm[0] += steps;
        if (!ok) note_bad(w.bad, c);
        else {
            note_change(w.mx[0], change);
            R.out0[c] = T1; R.out1[c] = logtem1;
        }
    }
    fold_head_words(w, R.first_bad, R.max_change, R.steps);
}

static int launch_thermal(void (*kernel)(const ThermalRec), const ThermalRec &R, hipStream_t stream)
{
    const bool bad = R.nratec < 2 || !R.cool || !R.out0 || !R.out1;
    return R.ncell > 0 && bad ? -1 : launch_over_leaves(kernel, R, R.ncell, stream);
}

int launch_thermal_equilibrium(const ThermalRec &R, hipStream_t stream)
{
    return R.ncell > 0 && !R.out2 ? -1 : launch_thermal(thermal_equilibrium_kernel, R, stream);
}

int launch_thermal_advance(const ThermalRec &R, hipStream_t stream)
{
    const bool bad = R.substeps < 1 || !(R.dt > 0.) || !(R.tmin > 0.) || !(R.tmax > R.tmin);
    return R.ncell > 0 && bad ? -1 : launch_thermal(thermal_advance_kernel, R, stream);
}

} // namespace ftte
