// ftte_rays.hip -- the kernels behind ftte_rays.cpp: absorption spectra along oblique rays through the refined grid.
//
// ray_walk_kernel, one lane per ray, is the walk of ftte_ray_math.h in two modes from one source, each of them also periodic (a
// template parameter, no run-time branch: the walk goes on through the box's opposite face up to the ray's tmax):
//   count  per ray its segments and its column density N = sum n size in ray order, whether a leaf has no line width, whether the
//          walk passed its step bound; across rays integer atomicOr / atomicMax only.  Nothing of the caller's is written before
//          the host has read these;
//   fill   the same walk again: at the ray's offset it writes the leaves' records (ftte_spectra_seg: everything per-leaf computed
//          once) and, where asked, the segment list (leaf, t_in, t_out').
// ray_spectra_kernel, one workgroup of 256 per ray, is the accumulate and the summary stage of sightline_spectra_kernel
// (ftte_spectra.hip) over the ray's records, read back chunk by chunk into LDS: a lane owns pixels p = tid + 256 r and keeps their
// tau in registers, all lanes read the same record at the same time, every pixel's sum runs over the leaves in ray order whatever
// the numbers of chunks and passes; then (1 - exp(-tau)) dv per pixel side by side and one lane adding in pixel order.
// No floating-point atomics; no scratch: the walk indexes nothing by a run-time axis.
#include <hip/hip_runtime.h>

#include "ftte_rays.h"

namespace ftte {

namespace {

template <bool Fill, bool Periodic> __global__ void __launch_bounds__(256) ray_walk_kernel(const RayRec Q)
{
    __shared__ int s_flags, s_most;
    if (!Fill) {
        if (threadIdx.x == 0) { s_flags = 0; s_most = 0; }
        __syncthreads();
    }
    const int64_t lane = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t ray = Fill ? Q.ray0 + lane : lane;
    if (Fill ? lane < Q.nrays : lane < Q.nray) {
        ftte_ray R;
        ftte_ray_walk W;
        ftte_ray_image I; // (the periodic modes alone: three image counters and the caller's origin)
        if (Periodic) ray_begin_periodic(&R, &W, &I, Q.n, Q.origin + 3 * ray, Q.dir + 3 * ray, Q.tmax[ray]);
        else ray_begin(&R, &W, Q.n, Q.origin + 3 * ray, Q.dir + 3 * ray, Q.tmax ? Q.tmax[ray] : 0.0);
        const ftte_ray_node *const node = reinterpret_cast<const ftte_ray_node *>(Q.node);
        const int32_t room = Fill ? Q.nseg[ray] : 0; // (the count pass walked the same ray)
        const int64_t at0 = Fill ? Q.offset[ray] - Q.offset[Q.ray0] : 0;
        int32_t count = 0;
        int flags = 0;
        int64_t steps = 0;
        double path = 0.0;
        while (!W.done) {
            if (++steps > Q.max_steps || !ray_locate(&R, &W, Q.n, node)) { flags |= 2; break; }
            double t_in, t_out;
            if (!(Periodic ? ray_cross_periodic(&R, &W, &I, Q.n, &t_in, &t_out) : ray_cross(&R, &W, Q.n, &t_in, &t_out))) continue;
            const int64_t cell = W.leaf;
            if (Q.value) {
                const double tgas = Q.tgas[cell];
                if (!Fill) {
                    path = path + Q.value[cell] * ((t_out - t_in) * Q.cell_cm);
                    flags |= !spectra_b2_ok(spectra_b2(&Q.par, tgas));
                } else if (Q.rec && count < room) {
                    ftte_spectra_seg S;
                    const double u = Q.velx ? ray_segment_u(&R, Q.velx[cell], Q.vely[cell], Q.velz[cell]) : 0.0;
                    (void)spectra_segment(&Q.par, Q.value[cell], (t_out - t_in) * Q.cell_cm, tgas, ray_segment_s(t_in, t_out) * Q.cell_cm, u, &S);
                    Q.rec[at0 + count] = S;
                }
            }
            if (Fill && Q.leaf && count < room) {
                Q.leaf[at0 + count] = cell;
                Q.t_in[at0 + count] = t_in;
                Q.t_out[at0 + count] = t_out;
            }
            if (count == 0x7fffffff) { flags |= 2; break; }
            ++count;
        }
        if (!Fill) {
            Q.nseg[ray] = count;
            Q.column[ray] = path;
            if (flags) atomicOr(&s_flags, flags);
            atomicMax(&s_most, count);
        }
    }
    if (!Fill) {
        __syncthreads();
        if (threadIdx.x == 0) {
            if (s_flags & 1) atomicOr(&Q.flags[0], 1);
            atomicMax(&Q.flags[1], s_most);
            if (s_flags & 2) atomicOr(&Q.flags[2], 1);
        }
    }
}

__global__ void __launch_bounds__(kSpectraLanes) ray_spectra_kernel(const RayRec Q)
{
    __shared__ ftte_spectra_seg s_seg[kSpectraChunk];
    const int tid = threadIdx.x;
    const int64_t slot = blockIdx.x, ray = Q.ray0 + slot;
    const int nseg = Q.nseg[ray];
    const ftte_spectra_seg *const rec = Q.rec + (Q.offset[ray] - Q.offset[Q.ray0]);

    // ---- accumulate
    double *const tau_line = Q.tau + slot * (int64_t)Q.nvel;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int64_t p0 = 0; p0 < Q.nvel; p0 += kSpectraPassPixels) {
        double vp[kSpectraPixelsPerLane], tau[kSpectraPixelsPerLane];
        bool live[kSpectraPixelsPerLane]; // the wavefront has a pixel of this row inside the spectrum
#pragma unroll
        for (int r = 0; r < kSpectraPixelsPerLane; ++r) {
            vp[r] = spectra_pixel_velocity(&Q.par, p0 + tid + kSpectraLanes * r);
            tau[r] = 0.0;
            live[r] = p0 + 64 * wave + kSpectraLanes * r < Q.nvel;
        }
        for (int c0 = 0; c0 < nseg; c0 += kSpectraChunk) {
            const int m = nseg - c0 < kSpectraChunk ? nseg - c0 : kSpectraChunk;
            __syncthreads();
            const double *src = reinterpret_cast<const double *>(rec + c0);
            double *dst = reinterpret_cast<double *>(s_seg);
            for (int q = tid; q < 4 * m; q += kSpectraLanes) dst[q] = src[q];
            __syncthreads();
            for (int q = 0; q < m; ++q) {
                const ftte_spectra_seg S = s_seg[q];
#pragma unroll
                for (int r = 0; r < kSpectraPixelsPerLane; ++r)
                    if (live[r]) tau[r] = spectra_accumulate(&Q.K, &Q.par, &S, vp[r], tau[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kSpectraPixelsPerLane; ++r) {
            const int64_t p = p0 + tid + kSpectraLanes * r;
            if (p < Q.nvel) tau_line[p] = tau[r];
        }
    }
    if (!Q.summary) return;

    // ---- summaries: the records' LDS now stages a pass of tau and of the width terms
    double *const s_term = reinterpret_cast<double *>(s_seg), *const s_tau = s_term + kSpectraPassPixels;
    double width = 0.0, total = 0.0;
    for (int64_t p0 = 0; p0 < Q.nvel; p0 += kSpectraPassPixels) {
        __syncthreads();
        for (int q = tid; q < kSpectraPassPixels && p0 + q < Q.nvel; q += kSpectraLanes) {
            const double t = tau_line[p0 + q];
            s_tau[q] = t;
            s_term[q] = spectra_width_term(&Q.K, t, Q.par.dv);
        }
        __syncthreads();
        if (tid == 0) {
            const int m = Q.nvel - p0 < kSpectraPassPixels ? (int)(Q.nvel - p0) : kSpectraPassPixels;
            for (int q = 0; q < m; ++q) { width = width + s_term[q]; total = total + s_tau[q]; }
        }
    }
    const double t_lo = 0.05 * total, t_hi = 0.95 * total;
    double run = 0.0;
    int64_t p_lo = -1, p_hi = -1;
    for (int64_t p0 = 0; p0 < Q.nvel; p0 += kSpectraPassPixels) {
        __syncthreads();
        for (int q = tid; q < kSpectraPassPixels && p0 + q < Q.nvel; q += kSpectraLanes) s_tau[q] = tau_line[p0 + q];
        __syncthreads();
        if (tid == 0) {
            const int m = Q.nvel - p0 < kSpectraPassPixels ? (int)(Q.nvel - p0) : kSpectraPassPixels;
            for (int q = 0; q < m; ++q) {
                run = run + s_tau[q];
                if (p_lo < 0 && run >= t_lo) p_lo = p0 + q;
                if (p_hi < 0 && run >= t_hi) p_hi = p0 + q;
            }
        }
    }
    if (tid == 0) {
        double *out = Q.summary + slot * 3;
        out[0] = Q.column[ray];
        out[1] = width;
        out[2] = spectra_dv90(total, p_lo, p_hi, Q.par.dv);
    }
}

bool rays_ok(const RayRec &Q)
{
    return Q.n >= 1 && Q.nray >= 1 && Q.origin && Q.dir && Q.max_steps >= 1 && Q.nseg && Q.column && (!Q.value == !Q.tgas) &&
           (!Q.velx == !Q.vely) && (!Q.velx == !Q.velz) && (!Q.periodic || Q.tmax);
}

bool batch_ok(const RayRec &Q) { return Q.offset && Q.ray0 >= 0 && Q.nrays >= 1 && Q.ray0 + Q.nrays <= Q.nray; }

} // namespace

int launch_ray_walk(const RayRec &Q, bool fill, void *stream)
{
    if (!rays_ok(Q)) return -1;
    if (fill) {
        if (!batch_ok(Q) || (!Q.rec && !Q.leaf) || (Q.rec && !Q.value) || (!Q.leaf != !Q.t_in) || (!Q.leaf != !Q.t_out)) return -1;
    } else if (!Q.flags) return -1;
    const int64_t groups = ((fill ? (int64_t)Q.nrays : Q.nray) + 255) / 256;
    if (groups > 0x7fffffff) return -1;
    const dim3 grid((unsigned)groups), block(256);
    if (fill && Q.periodic) hipLaunchKernelGGL((ray_walk_kernel<true, true>), grid, block, 0, (hipStream_t)stream, Q);
    else if (fill) hipLaunchKernelGGL((ray_walk_kernel<true, false>), grid, block, 0, (hipStream_t)stream, Q);
    else if (Q.periodic) hipLaunchKernelGGL((ray_walk_kernel<false, true>), grid, block, 0, (hipStream_t)stream, Q);
    else hipLaunchKernelGGL((ray_walk_kernel<false, false>), grid, block, 0, (hipStream_t)stream, Q);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_ray_spectra(const RayRec &Q, void *stream)
{
    if (!rays_ok(Q) || !batch_ok(Q) || !Q.rec || !Q.tau || Q.nvel < 1) return -1;
    hipLaunchKernelGGL(ray_spectra_kernel, dim3((unsigned)Q.nrays), dim3(kSpectraLanes), 0, (hipStream_t)stream, Q);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
