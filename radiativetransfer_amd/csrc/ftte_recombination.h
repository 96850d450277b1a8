// ftte_recombination.h -- the launch record of the diffuse recombination source (ftte_recombination.cpp; kernel:
// ftte_recombination.hip; the statement per leaf: ftte_recombination_math.h) and its launch wrapper: asynchronous on `stream`;
// returns 0, -1 bad argument, -2 launch failure.  A record of its own: the pass reads no rates, no J and no level, and writes no
// species, so it takes nothing of the per-leaf updates' records (ftte_leaf.h) but the loop, the fold and the launch shape.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace ftte {

struct RecombRec {
    // cell arrays, cell-array order
    const double *rho, *HI, *HeI, *HeII, *logtem;
    const double *g;                // [3][nratec] ground-state recombination coefficients of HI, HeI, HeII
    double *S;                      // [3][ncell] the source function
    unsigned long long *first_bad;  // lowest cell index whose leaf does not get through, or ~0
    unsigned long long *lost;       // (leaf, group) pairs that emit where nothing absorbs
    int64_t ncell;
    int32_t nratec;
    double logtem0, logtem9, dlogtem;
    double ksi[9];                  // [group][ksi24, ksi25, ksi26]
    double share[9];                // [ion][group]
};

int launch_recombination_source(const RecombRec &R, hipStream_t stream);

} // namespace ftte
