// ftte_spectra.hip -- the kernels behind ftte_spectra.cpp: absorption spectra along the pixel columns of the projected map.
//
// spectra_check_kernel, one lane per sightline, is project_map_kernel's walk (ftte_analysis.hip) once more: it counts the line's
// leaves, sums its column density in their order -- the same sum, the same bits as the map's mode 1 -- and says whether some
// leaf has no line width.  Nothing of the caller's is written before its verdict is in.
//
// sightline_spectra_kernel, one workgroup of 256 per sightline:
//   gather      the lanes take the line's base cells side by side, count their leaves, find their slots by an integer scan over
//               the workgroup and write the leaves' records (ftte_spectra_seg: everything per-leaf computed once) in sightline
//               order -- into LDS where the line has at most kSpectraChunk of them, else into the line's spill in memory;
//   accumulate  a lane owns pixels p = tid + 256 r, r < kSpectraPixelsPerLane, and keeps their tau in registers; all lanes read the
//               same record at the same time (an LDS broadcast) and pass through the chunk in order.  Pixels beyond one pass of
//               1024 take further passes, each over all chunks in order (a spilled line's chunks are read back): every pixel's
//               sum runs over the leaves in sightline order whatever the numbers of chunks and passes;
//   summaries   (1 - exp(-tau)) dv per pixel side by side into LDS, then one lane adds them, and tau, in pixel order: the host's
//               sequential loop, the same bits.
// No floating-point atomics (the check pass's are integer); no scratch: the per-lane arrays are unrolled into registers.
#include <hip/hip_runtime.h>

#include "ftte_spectra.h"

namespace ftte {

namespace {

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

__device__ __forceinline__ int half_of(double *x)
{
    if (*x < 0.5) { *x = 2.0 * *x; return 0; }
    *x = 2.0 * *x - 1.0;
    return 1;
}

// The leaves of a base cell's column in sightline order, as project_map_kernel visits them: both depth children of every refined
// cell, k = 1 then 2, depth first, from the base cell again for every leaf.  f(leaf, size [cm], centre): the leaf's centre along
// the depth as a fraction of the base cell, exact (a sum of powers of two).
template <class F> __device__ __forceinline__ void column_leaves(const SpectraRec &R, int64_t base, double x0, double y0, F &&f)
{
    if (!R.node) { f(base, R.cell_cm, 0.5); return; }
    unsigned long long kbits = 0ull;
    for (;;) {
        int64_t at = base;
        double x = x0, y = y0, size = R.cell_cm, lo = 0.0, half = 0.5;
        int depth = 0;
        NodeRec N = R.node[at];
        while (N.child0 >= 0) {
            const int a = half_of(&x), b = half_of(&y), c = (int)((kbits >> depth) & 1ull);
            at = (int64_t)N.child0 + R.zone.child[4 * a + 2 * b + c];
            N = R.node[at];
            size = size / 2.0;
            lo = c ? lo + half : lo;
            half = half * 0.5;
            ++depth;
        }
        f((int64_t)N.leaf, size, lo + half);
        while (depth > 0 && ((kbits >> (depth - 1)) & 1ull)) { kbits &= ~(1ull << (depth - 1)); --depth; }
        if (depth == 0) break;
        kbits |= 1ull << (depth - 1);
    }
}

__global__ void __launch_bounds__(256) spectra_check_kernel(const SpectraRec R)
{
    __shared__ int s_bad, s_most;
    if (threadIdx.x == 0) { s_bad = 0; s_most = 0; }
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < (int64_t)R.nxmap * R.nymap) {
        const int fast = R.fast_is_j ? R.nymap : R.nxmap;
        const int lo = (int)(p % fast), hi = (int)(p / fast);
        const int i = R.fast_is_j ? hi : lo, j = R.fast_is_j ? lo : hi;
        const double x0 = R.ifrac[i], y0 = R.jfrac[j];
        int count = 0, bad = 0;
        double path = 0.;
        for (int k0 = R.kstart; k0 <= R.kend; ++k0)
            column_leaves(R, base_node(R.zone, R.n, R.ibase[i], R.jbase[j], k0), x0, y0, [&](int64_t at, double size, double) {
                const double term = R.value[at] * size;
                path = path + term;
                bad |= !spectra_b2_ok(spectra_b2(&R.par, R.tgas[at]));
                ++count;
            });
        const int64_t line = (int64_t)i + (int64_t)R.nxmap * j;
        R.nseg[line] = count;
        R.column[line] = path;
        if (bad) atomicOr(&s_bad, 1);
        atomicMax(&s_most, count);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_bad) atomicOr(&R.flags[0], 1);
        atomicMax(&R.flags[1], s_most);
    }
}

// exclusive scan of one integer per lane over the workgroup; buf: [2 * 256]
__device__ __forceinline__ int scan_exclusive(int v, int32_t *buf, int *total)
{
    const int t = threadIdx.x;
    int32_t *in = buf, *out = buf + kSpectraLanes;
    in[t] = v;
    __syncthreads();
    for (int off = 1; off < kSpectraLanes; off <<= 1) {
        out[t] = in[t] + (t >= off ? in[t - off] : 0);
        __syncthreads();
        int32_t *swap = in; in = out; out = swap;
    }
    const int inclusive = in[t];
    *total = in[kSpectraLanes - 1];
    __syncthreads(); // (the next round writes the buffers again)
    return inclusive - v;
}

__global__ void __launch_bounds__(kSpectraLanes) sightline_spectra_kernel(const SpectraRec R)
{
    __shared__ ftte_spectra_seg s_seg[kSpectraChunk];
    __shared__ int32_t s_scan[2 * kSpectraLanes];
    const int tid = threadIdx.x;
    const int64_t slot = blockIdx.x, line = R.line0 + slot;
    const int i = (int)(line % R.nxmap), j = (int)(line / R.nxmap);
    const double x0 = R.ifrac[i], y0 = R.jfrac[j];
    const int i0 = R.ibase[i], j0 = R.jbase[j];
    const int nseg = R.nseg[line];
    const bool spilled = nseg > kSpectraChunk;
    if (spilled && (!R.spill || nseg > R.spill_stride)) return; // (the whole workgroup; the host sized the spill by the check pass's count)
    ftte_spectra_seg *const spill = R.spill + slot * R.spill_stride;

    // ---- gather
    int filled = 0;
    for (int kr = R.kstart; kr <= R.kend; kr += kSpectraLanes) {
        const int k0 = kr + tid;
        const bool active = k0 <= R.kend;
        const int64_t base = active ? base_node(R.zone, R.n, i0, j0, k0) : 0;
        int count = 0;
        if (active) column_leaves(R, base, x0, y0, [&](int64_t, double, double) { ++count; });
        int total;
        int at_slot = filled + scan_exclusive(count, s_scan, &total);
        if (active)
            column_leaves(R, base, x0, y0, [&](int64_t at, double size, double centre) {
                ftte_spectra_seg S;
                const double s = ((double)(k0 - R.kstart) + centre) * R.cell_cm;
                const double u = R.vel ? (R.vel_negate ? -R.vel[at] : R.vel[at]) : 0.0;
                (void)spectra_segment(&R.par, R.value[at], size, R.tgas[at], s, u, &S);
                if (at_slot < nseg) { // (the check pass counted the same leaves)
                    if (spilled) spill[at_slot] = S;
                    else s_seg[at_slot] = S;
                }
                ++at_slot;
            });
        filled += total;
    }
    __syncthreads();

    // ---- accumulate
    double *const tau_line = R.tau + slot * (int64_t)R.nvel;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int64_t p0 = 0; p0 < R.nvel; p0 += kSpectraPassPixels) {
        double vp[kSpectraPixelsPerLane], tau[kSpectraPixelsPerLane];
        bool live[kSpectraPixelsPerLane]; // the wavefront has a pixel of this row inside the spectrum
#pragma unroll
        for (int r = 0; r < kSpectraPixelsPerLane; ++r) {
            vp[r] = spectra_pixel_velocity(&R.par, p0 + tid + kSpectraLanes * r);
            tau[r] = 0.0;
            live[r] = p0 + 64 * wave + kSpectraLanes * r < R.nvel;
        }
        for (int c0 = 0; c0 < nseg; c0 += kSpectraChunk) {
            const int m = nseg - c0 < kSpectraChunk ? nseg - c0 : kSpectraChunk;
            if (spilled) {
                __syncthreads();
                const double *src = reinterpret_cast<const double *>(spill + c0);
                double *dst = reinterpret_cast<double *>(s_seg);
                for (int q = tid; q < 4 * m; q += kSpectraLanes) dst[q] = src[q];
                __syncthreads();
            }
            for (int q = 0; q < m; ++q) {
                const ftte_spectra_seg S = s_seg[q];
#pragma unroll
                for (int r = 0; r < kSpectraPixelsPerLane; ++r)
                    if (live[r]) tau[r] = spectra_accumulate(&R.K, &R.par, &S, vp[r], tau[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kSpectraPixelsPerLane; ++r) {
            const int64_t p = p0 + tid + kSpectraLanes * r;
            if (p < R.nvel) tau_line[p] = tau[r];
        }
    }
    if (!R.summary) return;

    // ---- summaries: the records' LDS now stages a pass of tau and of the width terms
    double *const s_term = reinterpret_cast<double *>(s_seg), *const s_tau = s_term + kSpectraPassPixels;
    double width = 0.0, total = 0.0;
    for (int64_t p0 = 0; p0 < R.nvel; p0 += kSpectraPassPixels) {
        __syncthreads();
        for (int q = tid; q < kSpectraPassPixels && p0 + q < R.nvel; q += kSpectraLanes) {
            const double t = tau_line[p0 + q];
            s_tau[q] = t;
            s_term[q] = spectra_width_term(&R.K, t, R.par.dv);
        }
        __syncthreads();
        if (tid == 0) {
            const int m = R.nvel - p0 < kSpectraPassPixels ? (int)(R.nvel - p0) : kSpectraPassPixels;
            for (int q = 0; q < m; ++q) { width = width + s_term[q]; total = total + s_tau[q]; }
        }
    }
    const double t_lo = 0.05 * total, t_hi = 0.95 * total;
    double run = 0.0;
    int64_t p_lo = -1, p_hi = -1;
    for (int64_t p0 = 0; p0 < R.nvel; p0 += kSpectraPassPixels) {
        __syncthreads();
        for (int q = tid; q < kSpectraPassPixels && p0 + q < R.nvel; q += kSpectraLanes) s_tau[q] = tau_line[p0 + q];
        __syncthreads();
        if (tid == 0) {
            const int m = R.nvel - p0 < kSpectraPassPixels ? (int)(R.nvel - p0) : kSpectraPassPixels;
            for (int q = 0; q < m; ++q) {
                run = run + s_tau[q];
                if (p_lo < 0 && run >= t_lo) p_lo = p0 + q;
                if (p_hi < 0 && run >= t_hi) p_hi = p0 + q;
            }
        }
    }
    if (tid == 0) {
        double *out = R.summary + slot * 3;
        out[0] = R.column[line];
        out[1] = width;
        out[2] = spectra_dv90(total, p_lo, p_hi, R.par.dv);
    }
}

bool geometry_ok(const SpectraRec &R)
{
    return R.n >= 1 && R.nxmap >= 1 && R.nymap >= 1 && R.value && R.tgas && R.ibase && R.jbase && R.ifrac && R.jfrac && R.kstart >= 1 &&
           R.kend <= R.n && R.nseg && R.column;
}

} // namespace

int launch_spectra_check(const SpectraRec &R, void *stream)
{
    if (!geometry_ok(R) || !R.flags) return -1;
    const int64_t groups = ((int64_t)R.nxmap * R.nymap + 255) / 256;
    if (groups > 0x7fffffff) return -1;
    hipLaunchKernelGGL(spectra_check_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// most_segments of the lines launched is what the caller read from the check pass: a line beyond a chunk needs its spill
int launch_spectra(const SpectraRec &R, void *stream)
{
    if (!geometry_ok(R) || !R.tau || R.nvel < 1 || R.nlines < 1 || R.line0 < 0 || R.line0 + R.nlines > (int64_t)R.nxmap * R.nymap) return -1;
    if (R.spill ? R.spill_stride < kSpectraChunk : R.spill_stride != 0) return -1;
    hipLaunchKernelGGL(sightline_spectra_kernel, dim3((unsigned)R.nlines), dim3(kSpectraLanes), 0, (hipStream_t)stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
