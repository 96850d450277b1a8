// ftte_lambda.hip -- CDNA4 (gfx950) kernels of the accelerated source iteration.
//
// lambda_diagonal_kernel: the diagonal of the discrete Lambda operator of the sweep with a source function (ftte_math.h:
// ftte_segment_source).  A cell's share of a segment is S + (Iin - S) g(tau); its three segments belong to three different rays and
// each takes its Iin from another cell (or the inflow), so the cell's own S enters its own J through S (1 - g(tau_seg)) alone:
//
//     Lambda*(cell, nu) = sum over directions  w/nseg * sum over the cell's segments (1 - g(kappa_nu(cell) dpath_seg))
//
// No ray dependency: one thread owns a (cell, nu) for all directions, adds in the sweep's own order (segments xy, xz, yz, then
// ftte_cell_mean, directions in list order) and stores once.  Each term is literally what the sweep computes for that cell with
// Iin = 0 and S = 1, so the result equals J[cell] of a sweep with S = 1 in that cell alone, bit for bit.
// The segment lengths depend on the cell's layer along the direction's march axis only (refined cell arrays: on the leaf's
// sub-layer of its level), so the geometry is a table per direction.  Where the march axis is not the contiguous storage axis a
// wavefront's cells share the layer and the record sits in scalar registers; otherwise the lanes index the table.
// The work is the sweep's own g evaluations without its memory traffic: kappa read once, Lambda* written once; fp64-VALU-bound.
//
// source_update_kernel: S <- S + ((1 - eps) J + eps B - S) / (1 - (1 - eps) Lambda*) in one pass, with max |dS| and max |S|.
#include <hip/hip_runtime.h>

#include "ftte_lambda.h"

namespace ftte {

namespace {

__device__ __forceinline__ int uniform_int(int x) { return __builtin_amdgcn_readfirstlane(x); }

// One direction's term of one cell: the means of its segments with Iin = 0, S = 1, added as the sweep adds them.  A segment the
// pattern does not have has dpath = 0: tau = 0, g = 1, and its mean is an exact zero; a wavefront none of whose lanes has it skips it.
__device__ __forceinline__ double lambda_term(const ftte_consts &K, double kap, double d0, double d1, double d2, int nseg, double w)
{
    double I = 0.0;
    double acc = ftte_segment_source(&K, K.c[9], &I, kap * d0, 1.0);
    if (FTTE_ANY(d1 > 0.0)) { I = 0.0; acc += ftte_segment_source(&K, K.c[9], &I, kap * d1, 1.0); }
    if (FTTE_ANY(d2 > 0.0)) { I = 0.0; acc += ftte_segment_source(&K, K.c[9], &I, kap * d2, 1.0); }
    return ftte_cell_mean(acc, nseg, w);
}

// Uniform grids.  A wavefront owns up to 64 consecutive kc of one (ic, jc) row, blockIdx.y the frequency group.
__global__ void __launch_bounds__(256) lambda_diagonal_kernel(const LambdaLaunch L)
{
    const int n = L.n;
    const int kchunks = (n + 63) >> 6;
    const long nwave = (long)n * n * kchunks;
    const long wave = (long)blockIdx.x * 4 + uniform_int((int)(threadIdx.x >> 6));
    if (wave >= nwave) return; // (the whole wavefront)
    const int row = (int)(wave / kchunks);
    const int ic = row / n, jc = row - ic * n;
    const int kc = (int)(wave - (long)row * kchunks) * 64 + (int)(threadIdx.x & 63);
    const bool live = kc < n;
    const int kq = live ? kc : n - 1; // lanes beyond the row compute the row's last cell and store nothing
    const long at = (long)blockIdx.y * L.ncell + ((long)row * n + kq);
    const double kap = L.kappa[at];
    const LambdaRec *__restrict__ table = L.table;
    const LambdaDir *__restrict__ dirs = L.dirs;
    double sum = 0.0;
    for (int d = 0; d < L.ndir; ++d) {
        const LambdaDir D = dirs[d];
        const LambdaRec *__restrict__ T = table + (long)d * L.stride;
        if (D.axis != 2) {
            // the layer is the wavefront's: scalar loads, wave-uniform control flow
            const int p = D.axis == 0 ? ic : jc;
            const LambdaRec R = T[D.mirror ? n - 1 - p : p];
            sum += lambda_term(L.K, kap, R.dpath[0], R.dpath[1], R.dpath[2], R.nseg, D.w);
        } else {
            const LambdaRec *R = T + (D.mirror ? n - 1 - kq : kq);
            sum += lambda_term(L.K, kap, R->dpath[0], R->dpath[1], R->dpath[2], R->nseg, D.w);
        }
    }
    if (live) L.diag[at] = sum;
}

// Refined cell arrays: a thread per leaf; the record is that of the leaf's sub-layer on its level.
__global__ void __launch_bounds__(256) lambda_diagonal_leaves_kernel(const LambdaLaunch L)
{
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = c < L.ncell;
    const long cq = live ? c : L.ncell - 1;
    const LambdaLeaf leaf = L.leaves[cq];
    const long at = (long)blockIdx.y * L.ncell + cq;
    const double kap = L.kappa[at];
    const int side = L.n << leaf.level;            // cells a side on the leaf's level
    const int level_off = L.n * ((1 << leaf.level) - 1); // where that level's records start
    const LambdaRec *__restrict__ table = L.table;
    const LambdaDir *__restrict__ dirs = L.dirs;
    double sum = 0.0;
    for (int d = 0; d < L.ndir; ++d) {
        const LambdaDir D = dirs[d];
        const int p = D.axis == 0 ? leaf.pos[0] : (D.axis == 1 ? leaf.pos[1] : leaf.pos[2]);
        const LambdaRec *R = table + (long)d * L.stride + level_off + (D.mirror ? side - 1 - p : p);
        sum += lambda_term(L.K, kap, R->dpath[0], R->dpath[1], R->dpath[2], R->nseg, D.w);
    }
    if (live) L.diag[at] = sum;
}

// Which elements have a denominator 1 - (1 - eps) Lambda* <= 0 (or not a number): the smallest index into stats[0]
__global__ void __launch_bounds__(256) source_update_check_kernel(const UpdateLaunch U)
{
    const double om = 1.0 - U.eps;
    unsigned long long my_bad = ~0ull;
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < U.ncell; c += (long)gridDim.x * 256) {
        const long q = (long)blockIdx.y * U.ncell + c;
        const double den = 1.0 - om * U.diag[q];
        if (!(den > 0.0)) my_bad = (unsigned long long)q < my_bad ? (unsigned long long)q : my_bad;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ob = __shfl_xor(my_bad, off);
        my_bad = ob < my_bad ? ob : my_bad;
    }
    if ((threadIdx.x & 63) == 0 && my_bad != ~0ull) atomicMin(U.stats, my_bad);
}

// The update itself.  Writes nothing when the check found a bad denominator.  The maxima are combined per wavefront, then per
// workgroup, then by one atomic each (a maximum does not depend on the order).
template <bool ACCELERATED>
__global__ void __launch_bounds__(256) source_update_kernel(const UpdateLaunch U)
{
    __shared__ unsigned long long blk_change[4], blk_size[4];
    const double om = 1.0 - U.eps;
    unsigned long long my_change = 0ull, my_size = 0ull;
    if (!ACCELERATED || *U.stats == ~0ull) {
        for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < U.ncell; c += (long)gridDim.x * 256) {
            const long q = (long)blockIdx.y * U.ncell + c;
            const double B = U.B[U.b_per_cell ? q : (long)blockIdx.y];
            const double S = U.S[q];
            double Snew;
            if (ACCELERATED) {
                const double fs = om * U.J[q] + U.eps * B;
                Snew = S + (fs - S) / (1.0 - om * U.diag[q]);
            } else {
                Snew = __builtin_fma(U.eps, B, om * U.J[q]);
            }
            U.S[q] = Snew;
            // non-negative doubles order like their bits
            const unsigned long long dbits = (unsigned long long)__double_as_longlong(__builtin_fabs(Snew - S));
            const unsigned long long sbits = (unsigned long long)__double_as_longlong(__builtin_fabs(Snew));
            my_change = dbits > my_change ? dbits : my_change;
            my_size = sbits > my_size ? sbits : my_size;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long oc = __shfl_xor(my_change, off), os = __shfl_xor(my_size, off);
        my_change = oc > my_change ? oc : my_change;
        my_size = os > my_size ? os : my_size;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { blk_change[wave] = my_change; blk_size[wave] = my_size; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            my_change = blk_change[k] > my_change ? blk_change[k] : my_change;
            my_size = blk_size[k] > my_size ? blk_size[k] : my_size;
        }
        if (my_change) atomicMax(U.stats + 1, my_change);
        if (my_size) atomicMax(U.stats + 2, my_size);
    }
}

} // namespace

int launch_lambda_diagonal(const LambdaLaunch &L, bool refined, hipStream_t stream)
{
    if (!L.kappa || !L.diag || !L.table || !L.dirs || L.n < 1 || L.nnu < 1 || L.ncell < 1 || L.ndir < 0 || (refined && !L.leaves)) return -1;
    if (refined) {
        const long blocks = (L.ncell + 255) / 256;
        hipLaunchKernelGGL(lambda_diagonal_leaves_kernel, dim3((unsigned)blocks, (unsigned)L.nnu), dim3(256), 0, stream, L);
    } else {
        const long waves = (long)L.n * L.n * ((L.n + 63) / 64);
        hipLaunchKernelGGL(lambda_diagonal_kernel, dim3((unsigned)((waves + 3) / 4), (unsigned)L.nnu), dim3(256), 0, stream, L);
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_source_update(const UpdateLaunch &U, hipStream_t stream)
{
    if (!U.J || !U.B || !U.S || !U.stats || U.nnu < 1 || U.ncell < 1) return -1;
    // (enough workgroups to fill the GPU several times over, few enough that their atomics are nothing); blockIdx.y: the group
    const long blocks = (U.ncell + 255) / 256;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096), (unsigned)U.nnu);
    if (U.diag) {
        hipLaunchKernelGGL(source_update_check_kernel, grid, dim3(256), 0, stream, U);
        hipLaunchKernelGGL(source_update_kernel<true>, grid, dim3(256), 0, stream, U);
    } else {
        hipLaunchKernelGGL(source_update_kernel<false>, grid, dim3(256), 0, stream, U);
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
