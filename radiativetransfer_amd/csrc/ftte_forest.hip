// ftte_forest.hip -- kernels of the segment forests of refined cell arrays (amr_*) and the moves between leaf order, base cells and
// cell-major order around them.  Records and launch wrappers: ftte_forest_rec.h; the host side is ftte_forests.h.
#include <hip/hip_runtime.h>

#include "ftte_forest_rec.h"
#include "ftte_math.h"

namespace ftte {

// ------------------------------------------------------------------------------------------------
// Refined cell arrays.  The host planner (ftte_amr.cpp) has turned the reference's per-direction
// neighbour links into a forest over segments, ordered by depth; one launch processes one depth of
// up to kAmrBatch directions: a thread per (segment, frequency group) takes the intensity its upstream
// segment left (or the inflow, or the mean of two segments: transportRoutinesModule.f90:594-649),
// crosses its own segment (ftte_math.h), and stores the outgoing intensity and the segment's mean.
// ------------------------------------------------------------------------------------------------
// grid: x over the (segment, frequency group) pairs of the fullest direction, y = direction of the batch.
// NNU_SHIFT >= 0: nnu = 1 << NNU_SHIFT (no division); -1: any nnu.
// segment `e` of the level that starts at `begin` in direction D's list, frequency group nu
__device__ __forceinline__ void amr_segment(const AmrLevelRec &A, const AmrDirRec &D, int64_t begin, unsigned e, unsigned nu, unsigned nnu)
{
    const SegRec R = D.rec[begin + e];
    const int seg = R.seg, up = R.up, up2 = R.up2;
    const size_t at = (size_t)(unsigned)seg * nnu + nu;
    double I;
    if (up == -3) I = D.faces[(size_t)nu * A.face_stride + (size_t)R.at]; // a ray handed over by a brick (hybrid sweep)
    else if (up < 0) I = A.uvb[nu];
    else {
        I = D.Iout[(size_t)(unsigned)up * nnu + nu];
        if (up2 >= 0) I = 0.5 * (I + D.Iout[(size_t)(unsigned)up2 * nnu + nu]);
    }
    const unsigned cell = (unsigned)seg / 3u;
    const size_t kat = (size_t)nu * A.group_stride + (size_t)cell * A.cell_stride;
    const double kap = A.kappa[kat];
    double m;
    if (A.emit == 0) m = ftte_segment(&A.math, &I, kap * R.dpath);
    else {
        const double x = A.emis[kat];
        m = A.emit == 2 ? ftte_segment_source(&A.math, A.math.c[9], &I, kap * R.dpath, x) : ftte_segment_emit(&A.math, &I, kap * R.dpath, x, 0.0);
    }
    D.Iout[at] = I;                              // read again by the segments downstream
    __builtin_nontemporal_store(m, &D.mean[at]); // read once, by the combine kernel
}

template <int NNU_SHIFT>
__global__ void __launch_bounds__(256) amr_level_kernel(const AmrLevelRec A)
{
    const int d = blockIdx.y;
    const unsigned count = (unsigned)A.count[d];
    const unsigned nnu = (unsigned)A.nnu;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const unsigned e = NNU_SHIFT >= 0 ? t >> (NNU_SHIFT >= 0 ? NNU_SHIFT : 0) : t / nnu;
    const unsigned nu = NNU_SHIFT >= 0 ? t & (nnu - 1u) : t - e * nnu;
    if (e >= count) return;
    amr_segment(A, A.dir[d], A.begin[d], e, nu, nnu);
}

// A run of THIN levels in one launch: one workgroup per direction walks levels depth0 .. depth0 + ndepth - 1 of its forest, a
// barrier between two levels (what a level reads of the one before was written by this workgroup, on this CU: visible behind the
// barrier).  A level of a few hundred segments is a launch of a few microseconds that the next one has to wait for, and a forest
// around a refined patch is a hundred of them: here they cost a barrier each.  tables: [depth][count[ndir], begin[ndir]].
template <int NNU_SHIFT>
__global__ void __launch_bounds__(1024) amr_levels_kernel(const AmrLevelRec A, const int64_t *__restrict__ tables, int ndepth)
{
    const int d = blockIdx.x;
    const unsigned nnu = (unsigned)A.nnu;
    const AmrDirRec &D = A.dir[d];
    for (int k = 0; k < ndepth; ++k) {
        const int64_t *T = tables + (size_t)k * 2 * (size_t)A.ndir;
        const unsigned items = (unsigned)T[d] * nnu;
        const int64_t begin = T[A.ndir + d];
        for (unsigned t = threadIdx.x; t < items; t += 1024u) {
            const unsigned e = NNU_SHIFT >= 0 ? t >> (NNU_SHIFT >= 0 ? NNU_SHIFT : 0) : t / nnu;
            const unsigned nu = NNU_SHIFT >= 0 ? t & (nnu - 1u) : t - e * nnu;
            amr_segment(A, D, begin, e, nu, nnu);
        }
        __syncthreads();
    }
}

// J[g][leaf] += (w / nseg) * (mean_xy + mean_xz + mean_yz), one direction after the other in list order
// (transportRoutinesModule.f90:953-955)
__global__ void __launch_bounds__(256) amr_combine_kernel(const AmrLevelRec A, double *__restrict__ J, int zero_first)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int nnu = A.nnu;
    const bool pow2 = (nnu & (nnu - 1)) == 0; // wave-uniform: a shift instead of a 64-bit division
    const long slot = pow2 ? tid >> (31 - __builtin_clz(nnu)) : tid / nnu;
    const int nu = (int)(tid - slot * nnu);
    if (slot >= (A.cells ? A.ncells : A.ncell)) return;
    const long cell = A.cells ? A.cells[slot] : slot; // where the leaf sits in J; everything of the forest is numbered by `slot`
    double acc_J = zero_first ? 0.0 : J[(long)nu * A.ncell + cell];
    for (int d = 0; d < A.ndir; ++d) {
        const AmrDirRec &D = A.dir[d];
        const int active = D.active[slot];
        if (active & 4) continue; // outside this direction's region: a brick holds the cell's contribution
        double acc = __builtin_nontemporal_load(&D.mean[(3 * slot) * nnu + nu]);
        int nseg = 1;
        if (active & 1) { acc += __builtin_nontemporal_load(&D.mean[(3 * slot + 1) * nnu + nu]); ++nseg; }
        if (active & 2) { acc += __builtin_nontemporal_load(&D.mean[(3 * slot + 2) * nnu + nu]); ++nseg; }
        acc_J += ftte_cell_mean(acc, nseg, D.w);
    }
    J[(long)nu * A.ncell + cell] = acc_J;
}

// the rays that leave the forest's region: into the face buffers the bricks behind it read (hybrid sweep)
__global__ void __launch_bounds__(256) amr_export_kernel(const AmrLevelRec A)
{
    const AmrDirRec &D = A.dir[blockIdx.y];
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int nnu = A.nnu;
    const long e = t / nnu;
    const int nu = (int)(t - e * nnu);
    // this launch's share of the direction's rays (a pass of the hybrid sweep), or all of them
    const long count = A.count ? (long)A.count[blockIdx.y] : (long)D.nexports, first = A.begin ? (long)A.begin[blockIdx.y] : 0l;
    if (e >= count) return;
    const AmrExport X = D.exports[first + e];
    D.faces[(size_t)nu * A.face_stride + (size_t)X.at] = D.Iout[(size_t)(unsigned)X.seg * nnu + nu];
}

// the rays that enter a fine block's own brick sweep from the forest around it (AmrImport)
__global__ void __launch_bounds__(256) amr_fine_import_kernel(const AmrLevelRec A)
{
    const AmrDirRec &D = A.dir[blockIdx.y];
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int nnu = A.nnu;
    const long e = t / nnu;
    const int nu = (int)(t - e * nnu);
    if (e >= (long)D.nimports) return;
    const AmrImport X = D.imports[e];
    double I;
    if (X.up < 0) I = A.uvb[nu];
    else {
        I = D.Iout[(size_t)(unsigned)X.up * nnu + nu];
        if (X.up2 >= 0) I = 0.5 * (I + D.Iout[(size_t)(unsigned)X.up2 * nnu + nu]);
    }
    D.faces[(size_t)nu * A.face_stride + (size_t)X.at] = I;
}

int launch_amr_fine_import(const AmrLevelRec &A, int64_t most, hipStream_t stream)
{
    if (most <= 0) return 0;
    const dim3 grid((unsigned)((most * A.nnu + 255) / 256), (unsigned)A.ndir);
    hipLaunchKernelGGL(amr_fine_import_kernel, grid, dim3(256), 0, stream, A);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_amr_export(const AmrLevelRec &A, int64_t most, hipStream_t stream)
{
    if (most <= 0) return 0;
    const dim3 grid((unsigned)((most * A.nnu + 255) / 256), (unsigned)A.ndir);
    hipLaunchKernelGGL(amr_export_kernel, grid, dim3(256), 0, stream, A);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// kappa of the base cells of a refined cell array, storage order [ic][jc][kc], from the leaf-ordered array (a refined base cell,
// which no brick reads, gets 0): what the bricks of the hybrid sweep march through
__global__ void __launch_bounds__(256) base_cells_kernel(const double *__restrict__ leaf_values, const int32_t *__restrict__ leaf_of_base,
                                                         double *__restrict__ base_values, long nbase, long ncell)
{
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbase) return;
    const int32_t leaf = leaf_of_base[b];
    const long g = blockIdx.y;
    base_values[g * nbase + b] = leaf >= 0 ? leaf_values[g * ncell + leaf] : 0.0;
}

int launch_base_cells(const double *leaf_values, const int32_t *leaf_of_base, double *base_values, long nbase, long ncell, int nnu,
                      hipStream_t stream)
{
    hipLaunchKernelGGL(base_cells_kernel, dim3((unsigned)((nbase + 255) / 256), (unsigned)nnu), dim3(256), 0, stream, leaf_values,
                       leaf_of_base, base_values, nbase, ncell);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// dst[cell][g] = src[g][cell]: the forest path reads all groups of a cell together, one 8 * nnu byte run per segment.
// cells != nullptr: dst[position][g] = src[g][cells[position]] for the `count` leaves of the list (src has `ncell` per group)
__global__ void __launch_bounds__(256) cell_major_kernel(const double *__restrict__ src, double *__restrict__ dst, long ncell, int nnu,
                                                         const int32_t *__restrict__ cells, long count)
{
    extern __shared__ double tile[]; // [nnu][64 + 1]
    const long c0 = (long)blockIdx.x * 64;
    for (int i = threadIdx.x; i < nnu * 64; i += 256) {
        const int g = i >> 6, c = i & 63;
        if (c0 + c < count) tile[g * 65 + c] = src[(long)g * ncell + (cells ? (long)cells[c0 + c] : c0 + c)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nnu * 64; i += 256) {
        const int c = i / nnu, g = i - c * nnu;
        if (c0 + c < count) dst[(c0 + c) * nnu + g] = tile[g * 65 + c];
    }
}

int launch_cell_major(const double *src, double *dst, long ncell, int nnu, hipStream_t stream, const int32_t *cells, long count)
{
    if (!cells) count = ncell;
    if (count <= 0) return 0;
    hipLaunchKernelGGL(cell_major_kernel, dim3((unsigned)((count + 63) / 64)), dim3(256), (size_t)nnu * 65 * sizeof(double), stream, src, dst,
                       ncell, nnu, cells, count);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_amr_level(const AmrLevelRec &A, hipStream_t stream)
{
    if (A.most <= 0) return 0;
    const int64_t threads = A.most * A.nnu;
    if (threads >= ((int64_t)1 << 32)) return -1;
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)A.ndir);
    switch (A.nnu) {
    case 1: hipLaunchKernelGGL(amr_level_kernel<0>, grid, dim3(256), 0, stream, A); break;
    case 2: hipLaunchKernelGGL(amr_level_kernel<1>, grid, dim3(256), 0, stream, A); break;
    case 4: hipLaunchKernelGGL(amr_level_kernel<2>, grid, dim3(256), 0, stream, A); break;
    case 8: hipLaunchKernelGGL(amr_level_kernel<3>, grid, dim3(256), 0, stream, A); break;
    case 16: hipLaunchKernelGGL(amr_level_kernel<4>, grid, dim3(256), 0, stream, A); break;
    default: hipLaunchKernelGGL(amr_level_kernel<-1>, grid, dim3(256), 0, stream, A); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_amr_levels(const AmrLevelRec &A, const int64_t *tables, int ndepth, hipStream_t stream)
{
    if (ndepth <= 0 || A.ndir <= 0) return 0;
    const dim3 grid((unsigned)A.ndir);
    switch (A.nnu) {
    case 1: hipLaunchKernelGGL(amr_levels_kernel<0>, grid, dim3(1024), 0, stream, A, tables, ndepth); break;
    case 2: hipLaunchKernelGGL(amr_levels_kernel<1>, grid, dim3(1024), 0, stream, A, tables, ndepth); break;
    case 4: hipLaunchKernelGGL(amr_levels_kernel<2>, grid, dim3(1024), 0, stream, A, tables, ndepth); break;
    case 8: hipLaunchKernelGGL(amr_levels_kernel<3>, grid, dim3(1024), 0, stream, A, tables, ndepth); break;
    case 16: hipLaunchKernelGGL(amr_levels_kernel<4>, grid, dim3(1024), 0, stream, A, tables, ndepth); break;
    default: hipLaunchKernelGGL(amr_levels_kernel<-1>, grid, dim3(1024), 0, stream, A, tables, ndepth); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_amr_combine(const AmrLevelRec &A, double *J, bool zero_first, hipStream_t stream)
{
    const long threads = (A.cells ? A.ncells : A.ncell) * A.nnu;
    if (threads <= 0) return 0;
    hipLaunchKernelGGL(amr_combine_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, A, J,
                       zero_first ? 1 : 0);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
