// ftte_thermal.hip -- the kernels behind the thermal entry points of ftte_chem.cpp: the thermal balance of every leaf
// (thermalEquilibrium, equiSources.f90:3870-4042) and its temperature advanced over a time step.  The thermal balance of a cell
// is ftte_thermal_math.h, compiled here for the device and by the tests' host library for the host; a kernel is the grid-stride
// loop of the chemistry kernels, the cell's loads, one call into that header, the cell's stores into the `out` buffers (copied in
// by the host once no cell has failed), and the fold of its statistics (ftte_chem_fold.h).
#include <hip/hip_runtime.h>

#include "ftte_chem_fold.h"
#include "ftte_internal.h"
#include "ftte_thermal.h"
#include "ftte_thermal_math.h"

namespace ftte {

// thermalEquilibrium per leaf (thermal_equilibrium_cell), at ftte_log of the leaf's temperature.  A leaf whose temperature is not
// positive and finite, or whose results are not finite, fails.
__global__ void __launch_bounds__(256) thermal_equilibrium_kernel(const ThermalRec R)
{
    unsigned long long my_bad = ~0ull;
    const ChemTable T = {nullptr, R.nratec, R.logtem0, R.logtem9, R.dlogtem};
    const ThermalTable C = {R.cool, (long)R.coef_stride, (long)R.node_stride};
    for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < R.ncell; c += (long)gridDim.x * blockDim.x) {
        double p24 = 0., p25 = 0., p26 = 0., heating = 0., cooling = 0., hydro = 0.;
        if (R.crate) { p24 = R.crate[c * kCellRec + 3]; p25 = R.crate[c * kCellRec + 4]; p26 = R.crate[c * kCellRec + 5]; }
        const double tgas = R.tgas[c];
        int ok = tgas > 0. && thermal_finite(tgas);
        if (ok) {
            hydro = thermal_equilibrium_cell(&T, &C, R.rho[c], tgas, ftte_log(&R.K, tgas), R.HI[c], R.HeI[c], R.HeII[c],
                                             chem_cell_volume(R.box, R.level[c], R.n), R.crate != nullptr, p24, p25, p26,
                                             R.run_uvb ? R.J + c : nullptr, R.ncell, R.gamma, R.uniform, R.threshold, R.comp1, R.comp2, &heating,
                                             &cooling);
            ok = thermal_finite(heating) && thermal_finite(cooling) && thermal_finite(hydro);
        }
        if (!ok) my_bad = (unsigned long long)c < my_bad ? (unsigned long long)c : my_bad;
        else { R.out0[c] = heating; R.out1[c] = cooling; R.out2[c] = hydro; }
    }
    fold_statistics<false>(R.first_bad, R.max_change, R.steps, 0ull, 0ull, my_bad);
}

// the temperature of every leaf advanced over R.dt in R.substeps implicit steps at the rates of the state on entry (thermal_advance_cell)
__global__ void __launch_bounds__(256) thermal_advance_kernel(const ThermalRec R)
{
    unsigned long long my_change = 0ull, my_steps = 0ull, my_bad = ~0ull;
    const ChemTable T = {nullptr, R.nratec, R.logtem0, R.logtem9, R.dlogtem};
    const ThermalTable C = {R.cool, (long)R.coef_stride, (long)R.node_stride};
    for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < R.ncell; c += (long)gridDim.x * blockDim.x) {
        double p24 = 0., p25 = 0., p26 = 0., T1, logtem1, change;
        if (R.crate) { p24 = R.crate[c * kCellRec + 3]; p25 = R.crate[c * kCellRec + 4]; p26 = R.crate[c * kCellRec + 5]; }
        unsigned long long steps;
        const int ok = thermal_advance_cell(&R.K, &T, &C, R.rho[c], R.tgas[c], R.HI[c], R.HeI[c], R.HeII[c], chem_cell_volume(R.box, R.level[c], R.n),
                                            R.crate != nullptr, p24, p25, p26, R.run_uvb ? R.J + c : nullptr, R.ncell, R.gamma, R.uniform,
                                            R.threshold, R.comp1, R.comp2, R.hydro ? R.hydro[c] : 0., R.dt, R.substeps, R.tmin, R.tmax, &T1,
                                            &logtem1, &steps, &change);
        my_steps += steps;
        if (!ok) my_bad = (unsigned long long)c < my_bad ? (unsigned long long)c : my_bad;
        else {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(change); // non-negative doubles order like their bits
            my_change = bits > my_change ? bits : my_change;
            R.out0[c] = T1; R.out1[c] = logtem1;
        }
    }
    fold_statistics<true>(R.first_bad, R.max_change, R.steps, my_change, my_steps, my_bad);
}

// (the chemistry kernels' launch shape: enough workgroups to fill the GPU several times over, few enough that their atomics are nothing)
static int launch_leaves(void (*kernel)(const ThermalRec), const ThermalRec &R, hipStream_t stream)
{
    if (R.ncell <= 0) return 0;
    if (R.nratec < 2 || !R.cool || !R.out0 || !R.out1) return -1;
    const long blocks = (R.ncell + 255) / 256;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_thermal_equilibrium(const ThermalRec &R, hipStream_t stream)
{
    return R.ncell > 0 && !R.out2 ? -1 : launch_leaves(thermal_equilibrium_kernel, R, stream);
}

int launch_thermal_advance(const ThermalRec &R, hipStream_t stream)
{
    const bool bad = R.substeps < 1 || !(R.dt > 0.) || !(R.tmin > 0.) || !(R.tmax > R.tmin);
    return R.ncell > 0 && bad ? -1 : launch_leaves(thermal_advance_kernel, R, stream);
}

} // namespace ftte
