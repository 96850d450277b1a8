// ftte_layout.hip -- J as a sum of pieces, and the layouts the pieces come in: the moves from cell-array order into the sweep layouts
// and the brick order, the merge of a sweep's accumulators into J, and the sum of the pieces of J that the devices of one context
// swept.  Constants and launch wrappers: ftte_layout.h.
#include <hip/hip_runtime.h>

#include "ftte_brick_rec.h"
#include "ftte_layout.h"

namespace ftte {

// ------------------------------------------------------------------------------------------------
// Layouts.  Cell-array order is [ic][jc][kc] (kc fastest).  A direction whose march axis is
// storage-j reads layout 1 = [jc][ic][kc]; storage-k reads layout 2 = [kc][ic][jc], so that the
// march axis is always the slowest and a sweep plane is always made of contiguous rows.
// ------------------------------------------------------------------------------------------------

// Brick order (BrickLaunch::tiled): element (a, b, c) of a frame [a][b][c] -- a the march axis, c contiguous -- when the eight rows
// b of a brick's layer are kept in one piece of 8 x 64 doubles, the pieces of a layer in the order of the bricks (along b, then
// along c).  n a multiple of 64 (and so of kBrickRows).
// chunk > 0: the `chunk` layers of a brick follow each other too (the brick in one piece; n a multiple of chunk).
__device__ __forceinline__ long tiled_index(int n, int a, int b, int c, int chunk = 0)
{
    const long piece = 64 * kBrickRows, in_piece = (b % kBrickRows) * 64 + c % 64;
    if (chunk > 0)
        return ((((long)(a / chunk) * (n / kBrickRows) + b / kBrickRows) * (n / 64) + c / 64) * chunk + a % chunk) * piece + in_piece;
    return (((long)a * (n / kBrickRows) + b / kBrickRows) * (n / 64) + c / 64) * piece + in_piece;
}

// dst[jc][ic][kc] = src[ic][jc][kc]   (rows of n doubles move as they are); layout 0: the rows stay where they are and only the
// brick order (tiled) moves them
template <bool tiled>
__global__ void __launch_bounds__(256) to_layout1_kernel(const double *__restrict__ src, double *__restrict__ dst, int n,
                                                         long group_stride, int layout, int tchunk)
{
    const long g = blockIdx.z;
    const int ic = blockIdx.y / n, jc = blockIdx.y % n;
    const double *s = src + g * group_stride + ((long)ic * n + jc) * n;
    const int a = layout == 1 ? jc : ic, b = layout == 1 ? ic : jc;
    double *d = dst + g * group_stride;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x)
        d[tiled ? tiled_index(n, a, b, k, tchunk) : ((long)a * n + b) * n + k] = s[k];
}

// dst[kc][ic][jc] = src[ic][jc][kc]   (per ic plane, a 32x32 tiled transpose through LDS)
template <bool tiled>
__global__ void __launch_bounds__(256) to_layout2_kernel(const double *__restrict__ src, double *__restrict__ dst, int n,
                                                         long group_stride, int tchunk)
{
    __shared__ double tile[32][33];
    const long g = blockIdx.z / n;
    const int ic = blockIdx.z % n;
    const int j0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32 x 8
    const double *s = src + g * group_stride + (long)ic * n * n;
    double *d = dst + g * group_stride;
    for (int r = ty; r < 32; r += 8)
        if (j0 + r < n && k0 + tx < n) tile[r][tx] = s[(long)(j0 + r) * n + k0 + tx];
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (k0 + r < n && j0 + tx < n) d[tiled ? tiled_index(n, k0 + r, ic, j0 + tx, tchunk) : ((long)(k0 + r) * n + ic) * n + j0 + tx] = tile[tx][r];
}

// The caller's opacities (cell-array order) into the library's three copies in ONE pass: dst0 as they come, dst1[jc][ic][kc] the
// same rows elsewhere (skipped when dst1 is null), dst2[kc][ic][jc] each ic plane transposed through LDS.  Read once, written three
// times (a copy and two transposes read them three times).
__global__ void __launch_bounds__(256) set_layouts_kernel(const double *__restrict__ src, double *__restrict__ dst0, double *__restrict__ dst1,
                                                          double *__restrict__ dst2, int n, long group_stride)
{
    __shared__ double tile[32][33];
    const long g = blockIdx.z / n;
    const int ic = blockIdx.z % n;
    const int j0 = blockIdx.y * 32, k0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32 x 8
    const long base = g * group_stride;
    for (int r = ty; r < 32; r += 8)
        if (j0 + r < n && k0 + tx < n) {
            const double v = src[base + ((long)ic * n + j0 + r) * n + k0 + tx];
            tile[r][tx] = v;
            dst0[base + ((long)ic * n + j0 + r) * n + k0 + tx] = v;
            if (dst1) dst1[base + ((long)(j0 + r) * n + ic) * n + k0 + tx] = v;
        }
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (k0 + r < n && j0 + tx < n) dst2[base + ((long)(k0 + r) * n + ic) * n + j0 + tx] = tile[tx][r];
}

int launch_set_layouts(const double *src, double *dst0, double *dst1, double *dst2, int n, int nnu, long group_stride, hipStream_t stream)
{
    const dim3 grid((n + 31) / 32, (n + 31) / 32, n * nnu);
    hipLaunchKernelGGL(set_layouts_kernel, grid, dim3(256), 0, stream, src, dst0, dst1, dst2, n, group_stride);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_to_layout(int layout, const double *src, double *dst, int n, int nnu, long group_stride, hipStream_t stream, bool tiled, int tchunk)
{
    if (tiled && (n % 64 != 0 || n % kBrickRows != 0 || (tchunk > 0 && n % tchunk != 0))) return -1;
    if (layout == 1 || (layout == 0 && tiled)) {
        const dim3 grid((n + 255) / 256, n * n, nnu);
        if (tiled) hipLaunchKernelGGL(to_layout1_kernel<true>, grid, dim3(256), 0, stream, src, dst, n, group_stride, layout, tchunk);
        else hipLaunchKernelGGL(to_layout1_kernel<false>, grid, dim3(256), 0, stream, src, dst, n, group_stride, layout, tchunk);
    } else if (layout == 2) {
        const dim3 grid((n + 31) / 32, (n + 31) / 32, n * nnu);
        if (tiled) hipLaunchKernelGGL(to_layout2_kernel<true>, grid, dim3(256), 0, stream, src, dst, n, group_stride, tchunk);
        else hipLaunchKernelGGL(to_layout2_kernel<false>, grid, dim3(256), 0, stream, src, dst, n, group_stride, tchunk);
    } else return -1;
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// J[ic][jc][kc] = sum over the accumulators in list order (layout 0 first, then 1, then 2; within
// a layout by slot).  One block per (32 jc x 32 kc) tile of one ic plane of one group.
struct MergeRec {
    const double *acc[3 * kMaxAcc];
    int layout[3 * kMaxAcc];
    int count;
};

// accumulate != 0: J += the accumulators (the additions continue the sequence of an earlier partial merge)
// leaf_of_base != nullptr (hybrid sweep of a refined cell array): the accumulators are arrays over the BASE cells (group stride
// n^3) and J is in cell-array order (group stride j_stride): element (ic, jc, kc) goes to its leaf, refined base cells are skipped.
// tiled: the accumulators are in brick order (tiled_index)
// blocks != nullptr: only the merge blocks listed there (kMergeBlock^3 cells, id (bi * nmb + bj) * nmb + bk): blockIdx.x the list entry,
// blockIdx.y the ic plane inside the block, blockIdx.z the group; the same sums per cell as the merge of the whole grid
template <bool tiled>
__global__ void __launch_bounds__(256) merge_kernel(const MergeRec M, double *__restrict__ J, int n, long group_stride, int accumulate,
                                                    const int32_t *__restrict__ leaf_of_base, long j_stride, int tchunk,
                                                    const int32_t *__restrict__ blocks, int nmb)
{
    static_assert(kMergeBlock == 32, "a merge block is one tile per ic plane");
    __shared__ double tile[32][33];
    long g;
    int ic, j0, k0;
    if (blocks) {
        const int b = blocks[blockIdx.x];
        const int bi = b / (nmb * nmb), bj = (b / nmb) % nmb, bk = b % nmb;
        g = blockIdx.z;
        ic = bi * kMergeBlock + (int)blockIdx.y;
        j0 = bj * kMergeBlock; k0 = bk * kMergeBlock;
        if (ic >= n) return; // (the whole workgroup: a ragged last block)
    } else {
        g = blockIdx.z / n;
        ic = blockIdx.z % n;
        j0 = blockIdx.y * 32; k0 = blockIdx.x * 32;
    }
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    bool have = false;
    if (accumulate && !leaf_of_base) {
        for (int q = 0; q < 4; ++q) {
            const int jc = j0 + ty + 8 * q, kc = k0 + tx;
            if (jc < n && kc < n) sum[q] = __builtin_nontemporal_load(&J[g * group_stride + ((long)ic * n + jc) * n + kc]);
        }
        have = true;
    }
    // the accumulators that need no transpose (layouts 0 and 1: they come first in the list), eight at a time: all their loads in
    // flight, then the sums in list order
    int a0 = 0;
    while (a0 < M.count && M.layout[a0] != 2) {
        int nb = 0;
        while (nb < 8 && a0 + nb < M.count && M.layout[a0 + nb] != 2) ++nb;
        double v[8][4];
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            if (b >= nb) continue;
            const double *s = M.acc[a0 + b] + g * group_stride;
            const bool one = M.layout[a0 + b] == 1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int jc = j0 + ty + 8 * q, kc = k0 + tx;
                v[b][q] = 0.0;
                if (jc >= n || kc >= n) continue;
                const int x = one ? jc : ic, y = one ? ic : jc;
                v[b][q] = __builtin_nontemporal_load(&s[tiled ? tiled_index(n, x, y, kc, tchunk) : ((long)x * n + y) * n + kc]);
            }
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            if (b >= nb) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) sum[q] = have ? sum[q] + v[b][q] : v[b][q];
            have = true;
        }
        a0 += nb;
    }
    for (int a = a0; a < M.count; ++a) {
        const double *s = M.acc[a] + g * group_stride;
        if (M.layout[a] == 2) {
            // element (ic, jc, kc) sits at [kc][ic][jc]: read rows along jc, transpose through LDS
            __syncthreads();
            for (int q = 0; q < 4; ++q) {
                const int r = ty + 8 * q; // kc offset
                if (k0 + r < n && j0 + tx < n)
                    tile[r][tx] = __builtin_nontemporal_load(&s[tiled ? tiled_index(n, k0 + r, ic, j0 + tx, tchunk) : ((long)(k0 + r) * n + ic) * n + j0 + tx]);
            }
            __syncthreads();
        }
        for (int q = 0; q < 4; ++q) {
            const int r = ty + 8 * q; // jc offset
            const int jc = j0 + r, kc = k0 + tx;
            if (jc >= n || kc >= n) continue;
            double v;
            if (M.layout[a] == 0) v = __builtin_nontemporal_load(&s[tiled ? tiled_index(n, ic, jc, kc, tchunk) : ((long)ic * n + jc) * n + kc]);
            else if (M.layout[a] == 1) v = __builtin_nontemporal_load(&s[tiled ? tiled_index(n, jc, ic, kc, tchunk) : ((long)jc * n + ic) * n + kc]);
            else v = tile[tx][r];
            sum[q] = have ? sum[q] + v : v;
        }
        have = true;
    }
    for (int q = 0; q < 4; ++q) {
        const int jc = j0 + ty + 8 * q, kc = k0 + tx;
        if (jc >= n || kc >= n) continue;
        const long b = ((long)ic * n + jc) * n + kc;
        if (!leaf_of_base) __builtin_nontemporal_store(sum[q], &J[g * group_stride + b]);
        else if (leaf_of_base[b] >= 0) { // += : the forest has already added the directions in whose box this cell lies
            double *dst = &J[g * j_stride + leaf_of_base[b]];
            *dst = accumulate ? *dst + sum[q] : sum[q];
        }
    }
}

int launch_merge(const double *const *acc, const int *layout, int count, double *J, int n, int nnu, long group_stride,
                 bool accumulate, hipStream_t stream, const int32_t *leaf_of_base, long j_stride, bool tiled, int tchunk)
{
    if (count > 3 * kMaxAcc) return -1;
    MergeRec M;
    M.count = count;
    for (int a = 0; a < count; ++a) { M.acc[a] = acc[a]; M.layout[a] = layout[a]; }
    const dim3 grid((n + 31) / 32, (n + 31) / 32, n * nnu);
    if (tiled) hipLaunchKernelGGL(merge_kernel<true>, grid, dim3(256), 0, stream, M, J, n, group_stride, accumulate ? 1 : 0, leaf_of_base, j_stride, tchunk, nullptr, 0);
    else hipLaunchKernelGGL(merge_kernel<false>, grid, dim3(256), 0, stream, M, J, n, group_stride, accumulate ? 1 : 0, leaf_of_base, j_stride, tchunk, nullptr, 0);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_merge_blocks(const double *const *acc, const int *layout, int count, double *J, int n, int nnu, long group_stride,
                        const int32_t *blocks, int nblocks, int nmb, hipStream_t stream, bool tiled, int tchunk)
{
    if (count > 3 * kMaxAcc || nmb != (n + kMergeBlock - 1) / kMergeBlock) return -1;
    if (nblocks == 0 || nnu == 0) return 0;
    MergeRec M;
    M.count = count;
    for (int a = 0; a < count; ++a) { M.acc[a] = acc[a]; M.layout[a] = layout[a]; }
    const dim3 grid(nblocks, kMergeBlock, nnu);
    if (tiled) hipLaunchKernelGGL(merge_kernel<true>, grid, dim3(256), 0, stream, M, J, n, group_stride, 0, nullptr, 0l, tchunk, blocks, nmb);
    else hipLaunchKernelGGL(merge_kernel<false>, grid, dim3(256), 0, stream, M, J, n, group_stride, 0, nullptr, 0l, tchunk, blocks, nmb);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- the pieces of J that the devices of one multi-device context swept for different directions, summed (ftte_multi.cpp)
struct SumParts { const double *part[64]; int nparts; };

__global__ void __launch_bounds__(256) sum_parts_kernel(const SumParts P, double *out, long count)
{
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= count) return;
    double sum = P.part[0][q];
    for (int k = 1; k < P.nparts; ++k) sum += P.part[k][q];
    out[q] = sum;
}

int launch_sum_parts(const double *const *parts, int nparts, double *out, long count, hipStream_t stream)
{
    if (nparts < 1 || nparts > 64 || count < 0) return -1;
    if (!count) return 0;
    SumParts P;
    for (int k = 0; k < nparts; ++k) P.part[k] = parts[k];
    P.nparts = nparts;
    hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, P, out, count);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
