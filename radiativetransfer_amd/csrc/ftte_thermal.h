// ftte_thermal.h -- the launch record and the launch wrappers of ftte_thermal.hip: the thermal balance of every leaf
// (thermalEquilibrium, equiSources.f90:3870-4042) and its temperature advanced over a time step.  Asynchronous on `stream`; return 0,
// -1 bad argument, -2 launch failure.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "ftte_math.h"

namespace ftte {

constexpr int kCoolNode = 16; // doubles per temperature node in the device's node-major cooling table: thirteen used, 128 bytes

struct ThermalRec {
    // cell arrays, cell-array order
    const int8_t *level;       // per leaf
    const double *rho, *tgas;
    const double *HI, *HeI, *HeII;
    const double *crate;       // [ncell][kCellRec] packed point-source rates (crate24..26 at +3..+5) or nullptr
    const double *J;           // [3][ncell] or nullptr (uniform background)
    const double *hydro;       // advance: the stored hydroHeating to add, or nullptr
    double *out0, *out1, *out2; // equilibrium: heating, cooling, hydroHeating; advance: tgas, logtem (out2 unused)
    const double *cool;        // the cooling coefficients, coefficient r of node i at cool[r * coef_stride + i * node_stride]
    int64_t coef_stride, node_stride;
    int64_t ncell;
    int32_t n, nratec, run_uvb, substeps;
    double box, logtem0, logtem9, dlogtem;
    double gamma[9];           // [group][gammaHI, gammaHeI, gammaHeII]
    double uniform[3];         // uniformQuasar * quasar%gamma + uniformStellar * stellar%gamma of HI, HeII, HeI
    double threshold;          // selfShieldingThreshold
    double comp1, comp2;       // compa (1+z)^4, 2.73 (1+z)
    double dt, tmin, tmax;     // advance only
    unsigned long long *first_bad, *max_change, *steps; // the chemistry kernels' counters
    ftte_consts K;
};

int launch_thermal_equilibrium(const ThermalRec &R, hipStream_t stream);
int launch_thermal_advance(const ThermalRec &R, hipStream_t stream);

} // namespace ftte
