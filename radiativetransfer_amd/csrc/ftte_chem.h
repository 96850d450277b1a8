// ftte_chem.h -- launch wrappers of the kernels of ftte_chem.hip that are no per-leaf update (those are ftte_leaf.h): the opacities,
// the hydrogen census, the optically thin radiation field.  All asynchronous on `stream`; return 0, -1 bad argument, -2 launch failure.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace ftte {

int launch_opacity(const double *HI, const double *HeI, const double *HeII, const double *beta, double *kappa, long ncell,
                   int nnu, hipStream_t stream);

// computeMass over the leaves: part[kMassParts]; the neutral and the total hydrogen mass [msun] land in part[2 kMassBlocks], [+1]
constexpr int kMassBlocks = 1024;
constexpr int kMassParts = 2 * kMassBlocks + 2;
int launch_hydrogen_mass(const int8_t *level, const double *HI, const double *rho, long ncell, int n, double box, double *part,
                         hipStream_t stream);
int launch_thin_limit(const double *HI, const double *HeI, const double *HeII, const double *rho, const double *uvb, double threshold,
                      double *J, long ncell, int nnu, hipStream_t stream);

} // namespace ftte
