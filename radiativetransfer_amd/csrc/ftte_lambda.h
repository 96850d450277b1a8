// ftte_lambda.h -- records and launch wrappers of ftte_lambda.hip: the diagonal of the Lambda operator of the sweep with a source
// function, and the source-function update of an (accelerated) Lambda iteration.  Plain structs, all launches asynchronous on `stream`;
// the wrappers return 0, -1 bad argument, -2 launch failure.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "ftte_math.h"

namespace ftte {

// One (sub-)layer of one direction: all cells of a layer -- all leaves of a sub-layer of their level -- share the ray pattern, so
// they share the lengths of their segments.
struct LambdaRec {
    double dpath[3]; // cell size * segment length in the order the cell's mean adds them: xy, xz, yz; 0: the pattern has no such segment
    int32_t nseg;    // segments the mean is taken over (1..3)
    int32_t pad_;
};
static_assert(sizeof(LambdaRec) == 32, "LambdaRec must be 32 bytes");

// One direction: which storage axis (0 = ic, 1 = jc, 2 = kc, the contiguous one) its march runs along, and whether against it
struct LambdaDir {
    double w;        // quadrature weight
    int32_t axis, mirror;
};

// A leaf of a refined cell array: its level and its 0-based storage position on the grid of that level (n 2^level cells a side)
struct LambdaLeaf {
    int32_t level, pos[3];
};
static_assert(sizeof(LambdaLeaf) == 16, "LambdaLeaf must be 16 bytes");

struct LambdaLaunch {
    const double *kappa;     // [nnu][ncell], cell-array order
    double *diag;            // [nnu][ncell]
    const LambdaRec *table;  // [ndir][stride]: per direction the records of level 0 (n), then level 1 (2 n), ...
    const LambdaDir *dirs;   // [ndir]
    const LambdaLeaf *leaves; // [ncell], refined cell arrays only
    int64_t ncell;
    int32_t n, nnu, ndir, stride;
    ftte_consts K;
};
int launch_lambda_diagonal(const LambdaLaunch &L, bool refined, hipStream_t stream);

// stats[0]: smallest element index with a denominator <= 0 (~0: none), stats[1], stats[2]: bits of max |S_new - S_old|, max |S_new|
struct UpdateLaunch {
    const double *J, *B, *diag; // [nnu][ncell]; B [nnu] unless b_per_cell; diag may be null (the plain update)
    double *S;
    unsigned long long *stats;
    int64_t ncell;
    double eps;
    int32_t nnu, b_per_cell;
};
int launch_source_update(const UpdateLaunch &U, hipStream_t stream);

} // namespace ftte
