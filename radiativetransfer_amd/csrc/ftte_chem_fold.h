// ftte_chem_fold.h -- the counter protocol of the per-leaf update kernels (ftte_chem.hip, ftte_thermal.hip), device code.
// The statistics of an update -- the largest change (kChange), the bisection steps, the first cell the update stops at --
// are combined per wavefront, then per workgroup, before they go to their single words in memory with one atomic each: a
// quarter of a million atomics on ONE address each cost more than all the arithmetic of the kernel.  For workgroups of 256.
#pragma once
#include <hip/hip_runtime.h>

namespace ftte {

template <bool kChange>
__device__ __forceinline__ void fold_statistics(unsigned long long *first_bad, unsigned long long *max_change, unsigned long long *steps,
                                                unsigned long long my_change, unsigned long long my_steps, unsigned long long my_bad)
{
    __shared__ unsigned long long blk_change[4], blk_steps[4], blk_bad[4];
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long oc = kChange ? __shfl_xor(my_change, off) : 0ull, os = __shfl_xor(my_steps, off), ob = __shfl_xor(my_bad, off);
        my_change = oc > my_change ? oc : my_change;
        my_steps += os;
        my_bad = ob < my_bad ? ob : my_bad;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { if (kChange) blk_change[wave] = my_change; blk_steps[wave] = my_steps; blk_bad[wave] = my_bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            if (kChange) my_change = blk_change[k] > my_change ? blk_change[k] : my_change;
            my_steps += blk_steps[k];
            my_bad = blk_bad[k] < my_bad ? blk_bad[k] : my_bad;
        }
        if (my_bad != ~0ull) atomicMin(first_bad, my_bad);
        if (kChange && my_change) atomicMax(max_change, my_change);
        if (my_steps) atomicAdd(steps, my_steps);
    }
}

} // namespace ftte
