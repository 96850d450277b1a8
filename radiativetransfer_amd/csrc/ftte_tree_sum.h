// ftte_tree_sum.h -- the fold of the deterministic censuses (hydrogen_mass_kernel, clumping_kernel): a workgroup of 256 threads
// adds its 256 partial sums as a fixed tree, every array handed over in the same pass.  No floating-point atomics, so a census
// gives the same bits run after run.
#pragma once

#include <hip/hip_runtime.h>

namespace ftte {

template <typename... Arrays> __device__ __forceinline__ void tree_sum_256(Arrays *...a)
{
    for (int w = 128; w > 0; w >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < w) { ((a[threadIdx.x] += a[threadIdx.x + w]), ...); }
    }
    __syncthreads();
}

} // namespace ftte
