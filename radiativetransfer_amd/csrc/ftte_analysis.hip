// ftte_analysis.hip -- the kernels behind ftte_analysis.cpp: the slice map, the projected map, the clumping census and the gas PDF
// of the device-resident medium.  A map is one lane per pixel and one descent (slice) or one column of descents (projection)
// through the NodeRec tree with the reference's child choice; the censuses are one pass over the leaves.
//
// Lanes and pixels.  A wavefront takes 64 consecutive pixels along the map axis R.fast_is_j names, which the host chooses as
// the axis that feeds the contiguous storage index where a map axis does, else the one that feeds the next (ftte_analysis.cpp:
// map_zone): neighbouring lanes then read the same or neighbouring leaves.  The map itself is float32 and small beside what is
// read; where the fast axis is the map's second, its stores are nxmap floats apart.
//
// Arithmetic.  The library is compiled with -ffp-contract=off, so products and sums stay apart as in the reference's compiled
// lines; the single-precision literals of :4948 are widened as the reference widens them.
#include <hip/hip_runtime.h>

#include "ftte_analysis.h"
#include "ftte_chem_math.h"
#include "ftte_tree_sum.h"

namespace ftte {

namespace {

// pixel (i, j) of this lane; i < 0 beyond the map
struct Pixel { int i, j; };
__device__ __forceinline__ Pixel lane_pixel(const MapRec &R)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)R.nxmap * R.nymap) return Pixel{-1, -1};
    const int fast = R.fast_is_j ? R.nymap : R.nxmap;
    const int lo = (int)(p % fast), hi = (int)(p / fast);
    return R.fast_is_j ? Pixel{hi, lo} : Pixel{lo, hi};
}

// rotateIndices(i0, j0, k0, n, n, n, izone, ...) -> the base cell's node (storage order, kcell fastest); 1-based in, 0-based out
__device__ __forceinline__ int64_t base_node(const MapZone &Z, int n, int i0, int j0, int k0)
{
    int64_t at = 0;
    for (int a = 0; a < 3; ++a) { // (selects, not an indexed array: nothing goes to scratch)
        const int v = Z.src[a] == 0 ? i0 : Z.src[a] == 1 ? j0 : k0;
        at = at * n + ((Z.mirror[a] ? n + 1 - v : v) - 1);
    }
    return at;
}

// x0 < 0.5 ? (1, 2 x0) : (2, 2 x0 - 1), sliceCell :203-209; returns i - 1
__device__ __forceinline__ int half_of(double *x)
{
    if (*x < 0.5) { *x = 2.0 * *x; return 0; }
    *x = 2.0 * *x - 1.0;
    return 1;
}

// readCellArray.f90:124-140 with sliceCell (:189-230): the pixel is the leaf's value, rounded to float32
__global__ void __launch_bounds__(256) slice_map_kernel(const MapRec R)
{
    const Pixel P = lane_pixel(R);
    if (P.i < 0) return;
    const int i = P.i, j = P.j;
    double x = R.ifrac[i], y = R.jfrac[j], z = R.kfrac;
    int64_t at = base_node(R.zone, R.n, R.ibase[i], R.jbase[j], R.kbase);
    if (R.node) {
        NodeRec N = R.node[at];
        while (N.child0 >= 0) {
            const int a = half_of(&x), b = half_of(&y), c = half_of(&z);
            at = (int64_t)N.child0 + R.zone.child[4 * a + 2 * b + c];
            N = R.node[at];
        }
        at = N.leaf;
    }
    R.map[(int64_t)i + (int64_t)R.nxmap * j] = (float)R.value[at];
}

// equiSources.f90:701-719 with projectVariableToMap (:4914-4954).  The descent below a base cell visits both depth children of
// every refined cell, k = 1 then 2, depth first; the choice along the map's axes depends on the level only, so the walk keeps one
// bit per level for k and descends from the base cell again for every leaf (trees are a few levels deep) instead of a stack.
// mode 1, the build's own: the path integral sum value * leaf size [cm] in double, rounded once at the end.
__global__ void __launch_bounds__(256) project_map_kernel(const MapRec R)
{
    const Pixel P = lane_pixel(R);
    if (P.i < 0) return;
    const int i = P.i, j = P.j;
    const double x0 = R.ifrac[i], y0 = R.jfrac[j];
    const int i0 = R.ibase[i], j0 = R.jbase[j];
    const double e25 = (double)1.e25f; // :4948
    float pixel = 0.f;
    double total = 0., path = 0.;
    for (int k0 = R.kstart; k0 <= R.kend; ++k0) {
        const int64_t base = base_node(R.zone, R.n, i0, j0, k0);
        unsigned long long kbits = 0ull;
        for (;;) {
            int64_t at = base;
            double x = x0, y = y0, size = R.cell_cm;
            int depth = 0;
            if (R.node) {
                NodeRec N = R.node[at];
                while (N.child0 >= 0) {
                    const int a = half_of(&x), b = half_of(&y), c = (int)((kbits >> depth) & 1ull);
                    at = (int64_t)N.child0 + R.zone.child[4 * a + 2 * b + c];
                    N = R.node[at];
                    size = size / 2.0;
                    ++depth;
                }
                at = N.leaf;
            }
            const double value = R.value[at];
            if (R.mode == 0) {
                const double tmp = (R.rho[at] * e25) * R.cube[depth];
                const double term = value * tmp;
                pixel = (float)((double)pixel + term);
                total = total + tmp;
            } else {
                const double term = value * size;
                path = path + term;
            }
            // the next leaf of this base cell: the deepest level still at k = 1 goes to k = 2, the levels below start over
            while (depth > 0 && ((kbits >> (depth - 1)) & 1ull)) { kbits &= ~(1ull << (depth - 1)); --depth; }
            if (depth == 0) break;
            kbits |= 1ull << (depth - 1);
        }
    }
    R.map[(int64_t)i + (int64_t)R.nxmap * j] = R.mode == 0 ? (float)((double)pixel / total) : (float)path;
}

// 2.**(3*level), a single-precision power (:4730): exact up to level 42, infinite from level 43 on as there
__device__ __forceinline__ double cube_of_two(int level)
{
    float p = 1.0f;
    for (int l = 0; l < 3 * level; ++l) p = p * 2.0f;
    return (double)p;
}

// computeClumping's leaf branch (:4729-4732) summed as hydrogen_mass_kernel sums: grid-stride per thread, a fixed tree per
// workgroup, the workgroups' sums in a fixed order by clumping_total_kernel
__global__ void __launch_bounds__(256) clumping_kernel(const ClumpRec R)
{
    __shared__ double sv[256], sd[256], sq[256];
    double av = 0., ad = 0., aq = 0.;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < R.ncell; c += (int64_t)gridDim.x * 256) {
        const double nh = chem_nh(R.rho[c]), p = cube_of_two(R.level[c]);
        av += 1.0 / p;
        ad += nh / p;
        aq += nh * nh / p;
    }
    sv[threadIdx.x] = av; sd[threadIdx.x] = ad; sq[threadIdx.x] = aq;
    tree_sum_256(sv, sd, sq);
    if (threadIdx.x == 0) { R.part[blockIdx.x] = sv[0]; R.part[kClumpBlocks + blockIdx.x] = sd[0]; R.part[2 * kClumpBlocks + blockIdx.x] = sq[0]; }
}

__global__ void __launch_bounds__(256) clumping_total_kernel(double *part, int nblocks)
{
    __shared__ double sv[256], sd[256], sq[256];
    double av = 0., ad = 0., aq = 0.;
    for (int b = threadIdx.x; b < nblocks; b += 256) { av += part[b]; ad += part[kClumpBlocks + b]; aq += part[2 * kClumpBlocks + b]; }
    sv[threadIdx.x] = av; sd[threadIdx.x] = ad; sq[threadIdx.x] = aq;
    tree_sum_256(sv, sd, sq);
    if (threadIdx.x == 0) { part[3 * kClumpBlocks] = sv[0]; part[3 * kClumpBlocks + 1] = sd[0]; part[3 * kClumpBlocks + 2] = sq[0]; }
}

// computeGasPDF's leaf branch (:4700-4706) as integer counts per (bin, level): LDS atomics in the workgroup, then one global
// atomic per slot that holds something.  Integers, so the order of the leaves does not matter; the host weighs them.
__global__ void __launch_bounds__(256) gas_pdf_kernel(const PdfRec R)
{
    extern __shared__ unsigned int s_count[]; // [kPdfSlots][nlev]
    const int slots = kPdfSlots * R.nlev;
    for (int q = threadIdx.x; q < slots; q += 256) s_count[q] = 0u;
    __syncthreads();
    const double pc = (double)3.08568025e18f; // definitionsModule.f90:21
    const double pc3 = pc * pc * pc;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < R.ncell; c += (int64_t)gridDim.x * 256) {
        const double tmp = log10(R.rho[c] / FTTE_MSUN * pc3);
        int level = R.level[c];
        level = level < 0 ? 0 : level >= R.nlev ? R.nlev - 1 : level;
        atomicAdd(&s_count[pdf_bin(tmp) * R.nlev + level], 1u);
    }
    __syncthreads();
    for (int q = threadIdx.x; q < slots; q += 256)
        if (s_count[q]) atomicAdd(&R.counts[q], (unsigned long long)s_count[q]);
}

} // namespace

int launch_slice_map(const MapRec &R, void *stream)
{
    if (R.n < 1 || R.nxmap < 1 || R.nymap < 1 || !R.value || !R.ibase || !R.jbase || !R.ifrac || !R.jfrac || !R.map || R.kbase < 1 || R.kbase > R.n)
        return -1;
    const int64_t groups = ((int64_t)R.nxmap * R.nymap + 255) / 256;
    if (groups > 0x7fffffff) return -1;
    hipLaunchKernelGGL(slice_map_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_project_map(const MapRec &R, void *stream)
{
    if (R.n < 1 || R.nxmap < 1 || R.nymap < 1 || !R.value || !R.ibase || !R.jbase || !R.ifrac || !R.jfrac || !R.map || R.kstart < 1 ||
        R.kend > R.n || R.levels < 1 || R.levels > kMapLevels || (R.mode != 0 && R.mode != 1) || (R.mode == 0 && !R.rho))
        return -1;
    const int64_t groups = ((int64_t)R.nxmap * R.nymap + 255) / 256;
    if (groups > 0x7fffffff) return -1;
    hipLaunchKernelGGL(project_map_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_clumping(const ClumpRec &R, void *stream)
{
    if (R.ncell < 1 || !R.level || !R.rho || !R.part) return -1;
    const int64_t want = (R.ncell + 255) / 256;
    const int blocks = (int)(want < kClumpBlocks ? want : kClumpBlocks);
    hipLaunchKernelGGL(clumping_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, R);
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(clumping_total_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, R.part, blocks);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_gas_pdf(const PdfRec &R, void *stream)
{
    if (R.ncell < 1 || !R.level || !R.rho || !R.counts || R.nlev < 1 || R.nlev > kPdfLevels) return -1;
    const int64_t want = (R.ncell + 255) / 256;
    const int blocks = (int)(want < 4096 ? want : 4096); // (a few leaves per thread: fewer flushes to memory)
    const size_t lds = sizeof(unsigned int) * (size_t)kPdfSlots * (size_t)R.nlev;
    hipLaunchKernelGGL(gas_pdf_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
