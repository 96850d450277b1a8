// ftte_expansion.hip -- the start-up expansion of HII regions on the device (equiSources.f90:1035-1069): findExpansion for every
// star and leaf, then applyExpansion, in one launch.
//
// One thread per leaf, a workgroup of 256 consecutive leaves of the cell array.  The reference visits every leaf for every star;
// here a workgroup first reduces the box around its leaf centres, then takes the stars through LDS in tiles of 256: every thread
// tests one star's sphere against the box (expansion_sphere_reaches_box: conservative), the survivors are compacted with wave
// ballots into the tile, and only they go through the exact test, which is the reference's arithmetic operation by operation
// (expansion_accepts).  rhoCoef is a minimum over the accepted stars of values that do not depend on each other -- the density in
// the test is the leaf's own before any expansion -- so neither the cull nor the order of the stars can change a bit of it.
#include <hip/hip_runtime.h>

#include "ftte_chem_math.h"
#include "ftte_expansion.h"

namespace ftte {

namespace {

constexpr int kWaves = kExpGroup / 64;

__device__ __forceinline__ double wave_min(double v)
{
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(v, off); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(v, off); v = o > v ? o : v; }
    return v;
}

__global__ void __launch_bounds__(kExpGroup) expansion_kernel(const ExpandRec R)
{
    __shared__ double s_box[6][kWaves];
    __shared__ ExpStar s_star[kExpGroup];
    __shared__ ExpStarTest s_test[kExpGroup];
    __shared__ int s_count[kWaves];

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c = (int64_t)blockIdx.x * kExpGroup + tid;
    const bool live = c < R.ncell;

    // the leaf's centre (findExpansion's xcell, ycell, zcell) and its hydrogen density before any expansion
    double x = 0., y = 0., z = 0., nh = 0.;
    if (live) {
        if (R.pos) {
            expansion_leaf_centre(R.pos[c], R.n, R.shift, &x, &y, &z);
        } else {
            const int64_t nn = (int64_t)R.n * R.n;
            const int i0 = (int)(c / nn), j0 = (int)((c / R.n) % R.n), k0 = (int)(c % R.n);
            x = expansion_base_centre(i0, R.n); y = expansion_base_centre(j0, R.n); z = expansion_base_centre(k0, R.n);
        }
        nh = chem_nh(R.rho[c]);
    }

    // the box around the workgroup's centres
    const double inf = __builtin_inf();
    const double v[6] = {wave_min(live ? x : inf), wave_min(live ? y : inf), wave_min(live ? z : inf),
                         wave_max(live ? x : -inf), wave_max(live ? y : -inf), wave_max(live ? z : -inf)};
    if (lane == 0)
        for (int q = 0; q < 6; ++q) s_box[q][wave] = v[q];
    __syncthreads();
    double lo[3], hi[3];
    for (int q = 0; q < 3; ++q) {
        double a = s_box[q][0], b = s_box[3 + q][0];
        for (int w = 1; w < kWaves; ++w) {
            a = s_box[q][w] < a ? s_box[q][w] : a;
            b = s_box[3 + q][w] > b ? s_box[3 + q][w] : b;
        }
        lo[q] = a; hi[q] = b;
    }

    double coef = 1.0; // rhoCoef, equiSources.f90:507, :1944
    unsigned long long survivors = 0;
    for (int t0 = 0; t0 < R.nsrc; t0 += kExpGroup) {
        const int s = t0 + tid;
        bool keep = false;
        ExpStar S = {0., 0., 0., 0.};
        if (s < R.nsrc) {
            S = R.star[s];
            keep = expansion_sphere_reaches_box(S, lo, hi);
        }
        const unsigned long long mask = __ballot(keep);
        const int rank = __popcll(mask & ((1ull << lane) - 1ull));
        __syncthreads(); // the last tile has been read by everyone
        if (lane == 0) s_count[wave] = __popcll(mask);
        __syncthreads();
        int first = 0, total = 0;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) first += s_count[w];
            total += s_count[w];
        }
        if (keep) {
            s_star[first + rank] = S;
            s_test[first + rank] = R.test[s];
        }
        __syncthreads();
        if (live)
            for (int k = 0; k < total; ++k)
                if (expansion_accepts(s_star[k], s_test[k], x, y, z, nh, R.box)) {
                    const double d = s_test[k].coef;
                    coef = d < coef ? d : coef; // min(rhoCoef, densityCoefficient)
                }
        survivors += (unsigned long long)total;
    }

    // applyExpansion (:4495-4500)
    const bool changed = live && coef < 1.0;
    if (changed) {
        R.rho[c] = R.rho[c] * coef;
        R.HI[c] = R.HI[c] * coef;
        R.HeI[c] = R.HeI[c] * coef;
        R.HeII[c] = R.HeII[c] * coef;
    }
    if (live && R.rho_coef) R.rho_coef[c] = coef;

    const unsigned long long cmask = __ballot(changed);
    __syncthreads();
    if (lane == 0) s_count[wave] = __popcll(cmask);
    __syncthreads();
    if (tid == 0) {
        const int64_t left = R.ncell - (int64_t)blockIdx.x * kExpGroup;
        const unsigned long long leaves = (unsigned long long)(left < kExpGroup ? left : kExpGroup);
        if (survivors) atomicAdd(&R.counters[0], survivors * leaves);
        int nchanged = 0;
        for (int w = 0; w < kWaves; ++w) nchanged += s_count[w];
        if (nchanged) atomicAdd(&R.counters[1], (unsigned long long)nchanged);
    }
}

// out[q] = field[cells[q]]: the densities of the stars' host leaves
__global__ void __launch_bounds__(256) gather_kernel(const double *__restrict__ field, const int64_t *__restrict__ cells, int count,
                                                     double *__restrict__ out)
{
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q < count) out[q] = field[cells[q]];
}

} // namespace

int launch_expansion(const ExpandRec &R, void *stream)
{
    if (R.ncell < 1 || R.n < 1 || R.nsrc < 1 || !R.star || !R.test || !R.rho || !R.HI || !R.HeI || !R.HeII || !R.counters) return -1;
    const int64_t groups = (R.ncell + kExpGroup - 1) / kExpGroup;
    if (groups > 0x7fffffff) return -1;
    hipLaunchKernelGGL(expansion_kernel, dim3((unsigned)groups), dim3(kExpGroup), 0, (hipStream_t)stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_gather(const double *field, const int64_t *cells, int count, double *out, void *stream)
{
    if (count < 1 || !field || !cells || !out) return -1;
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, field, cells, count, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
