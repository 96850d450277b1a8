// ftte_tile.hip -- CDNA4 (gfx950) kernel of the ray-following tile sweep of round 1 (sweep_kernel, option "engine" = 1).  Its records
// and its launch wrapper are ftte_tile_rec.h; the brick sweep is ftte_brick.hip.
//
// The tile sweep.  What is computed (per direction, per frequency group): the reference's cell transfer,
//   transportRoutinesModule.f90:587-961  /  equiSources.f90:1580-1788,
// on a uniform grid.  How it is organised has nothing in common with the reference's serial
// pointer walk:
//
//  * After the izone rotation (rotateIndicesModule.f90) the march axis is sweep-i and every cell
//    of a layer shares one ray pattern, so a physical ray is a chain of 1-3 segments per layer
//    that drifts by at most one cell per layer along sweep-j and sweep-k, identically for all
//    rays of the direction.  Chains never interact: the only coupling is that a cell's mean
//    collects the segments of up to three different rays.
//  * One wavefront owns a tile of 64 x ROWS rays: 64 lanes along u, the storage-contiguous axis
//    of this direction's layout (every kappa/J access is a 512-byte coalesced row), ROWS rays
//    per lane along v.  The ray intensities never leave registers for the whole march.
//  * A cell's mean needs the 2nd/3rd segments of the rays one step lower in u and/or v: from
//    lane-1 through a DPP wave shift, from the previous row through registers.  Lane 0 and row
//    0 of every tile are therefore a read-only halo, recomputed by the neighbouring tile: no
//    LDS, no barrier, no atomics, no inter-wave communication of any kind, and every cell of
//    the grid is owned by exactly one lane of one wave per direction, which makes J a plain,
//    deterministic read-modify-write.
//  * The host turns each direction into a 32-byte-per-layer table (segment lengths, chain
//    class, cumulative drift) that the wave reads with scalar loads; per-layer control flow is
//    wave-uniform.
//
// Roofline: 24 algorithmic bytes per cell.direction.frequency update (kappa 8 B read, J 8 B
// read + 8 B write), ~2 segments of ~45 fp64 VALU instructions each: HBM-bound by design,
// with the fp64 pipe at 60-80 % when HBM saturates.
#include <hip/hip_runtime.h>

#include "ftte_layer_rec.h"
#include "ftte_math.h"
#include "ftte_tile_rec.h"

namespace ftte {

// Pointers that went through uniform() have lost their address space as far as the compiler can tell, and a generic pointer
// is read with flat_load, which also occupies the LDS path and counts on lgkmcnt: say that they are global memory.
using gcbyte = const __attribute__((address_space(1))) char;
using gbyte = __attribute__((address_space(1))) char;
using gcdouble = const __attribute__((address_space(1))) double;
using gdouble = __attribute__((address_space(1))) double;

// value held by lane-1 (lane 0 receives its own value back; it is a halo lane and never uses it)
__device__ __forceinline__ double from_lane_below(double x)
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    // DPP wave_shr:1 -- a full-rate VALU move, no LDS crossbar
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Values that are the same in every lane but reach the wave through vector loads (the compiler cannot prove the
// tables are not written by the kernel, so it will not use scalar loads for them): pin them into SGPRs, so that
// everything derived from them -- plane and row addresses, segment lengths, branch conditions -- is scalar.
__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ long uniform(long x)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x & 0xffffffffl));
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long)x >> 32));
    return (long)(((unsigned long)hi << 32) | lo);
}
__device__ __forceinline__ double uniform(double x) { return __longlong_as_double(uniform((long)__double_as_longlong(x))); }
template <typename T> __device__ __forceinline__ T *uniform(T *p) { return reinterpret_cast<T *>(uniform(reinterpret_cast<long>(p))); }

// One segment of one ray.  EDGE: the cell may lie outside the domain, where the ray is
// re-initialised with the inflow (transportRoutinesModule.f90:594-597) and adds nothing.
// EMIT: 0 no emission (the reference as shipped), 1 `x` is the reference's emissivity eta, 2 `x` is a source function S
// (ftte_math.h: ftte_segment_emit, ftte_segment_source).
template <bool EDGE, int EMIT>
__device__ __forceinline__ double segment(const ftte_consts &K, double &I, double kap, double x, double dpath, bool inside,
                                          double uvb)
{
    double It = I, m;
    if (EMIT == 0) m = ftte_segment(&K, &It, kap * dpath);
    else if (EMIT == 2) m = ftte_segment_source(&K, K.c[9], &It, kap * dpath, x);
    else m = ftte_segment_emit(&K, &It, kap * dpath, x, 0.0);
    if (EDGE) {
        I = inside ? It : uvb;
        return inside ? m : 0.0;
    }
    I = It;
    return m;
}

// One layer of one tile.  RC: chain class (ftte_layer_rec.h).  I[r]: intensity of ray r of this
// lane on entry to the layer / on exit.
//   kplane / jplane : byte pointers to the virtual element (row 0, column position 0) of this layer's
//                     kappa / J plane; rows are sv elements apart; a lane's column enters as a
//                     non-negative position (mirrored columns are folded into the position by the
//                     caller) so that every access is  uniform 64-bit base + 32-bit lane offset.
//   STACK           : wavefronts of the workgroup stacked along v.  The cell of row 0 needs the 2nd/3rd
//                     segments of the row below, which belongs to the wavefront below: with STACK = 1 row 0
//                     is a read-only halo (the tile below recomputes it); with STACK > 1 only the lowest
//                     wavefront has a halo row, the others receive the two numbers per lane they need
//                     through LDS (`xchg`, one s_barrier per layer that has such segments) and own row 0.
template <int ROWS, int RC, bool EDGE, int STACK, int EMIT>
__device__ __forceinline__ void layer_step(const ftte_consts &K, double (&I)[ROWS], gcbyte *__restrict__ kplane,
                                           gcbyte *__restrict__ xplane, gbyte *__restrict__ jplane, int cv0, int cu,
                                           int n, int sv, bool mirror_u,
                                           double d0, double d1, double d2, double w, double uvb, bool first,
                                           bool lane_owned, int lane, int wid, double *xchg)
{
    constexpr int SHAPE = (RC == RC_THREE_U_SWAP) ? RC_THREE_U : (RC == RC_THREE_V_SWAP) ? RC_THREE_V : RC;
    constexpr bool THIRD_FIRST = (RC == RC_THREE_U_SWAP || RC == RC_THREE_V_SWAP);
    constexpr bool HAS_U = (SHAPE == RC_TWO_U || SHAPE == RC_THREE_U || SHAPE == RC_THREE_V); // touches column u+1
    constexpr bool HAS_V = (SHAPE == RC_TWO_V || SHAPE == RC_THREE_U || SHAPE == RC_THREE_V); // touches row v+1
    constexpr int NSEG = (SHAPE == RC_ONE) ? 1 : (SHAPE <= RC_TWO_V ? 2 : 3);
    const bool row0_owned = STACK > 1 && wid > 0; // wave-uniform
    constexpr int R0 = (STACK > 1) ? 0 : 1;       // first row that may be owned

    // lane-varying column positions, clamped into the domain for EDGE tiles
    const int c0 = EDGE ? clampi(cu, 1, n) : cu;
    const int c1 = EDGE ? clampi(cu + 1, 1, n) : cu + 1;
    const unsigned off0 = 8u * (unsigned)(mirror_u ? n + 1 - c0 : c0);
    const unsigned off1 = 8u * (unsigned)(mirror_u ? n + 1 - c1 : c1);
    const bool in_u0 = !EDGE || (cu >= 1 && cu <= n);
    const bool in_u1 = !EDGE || (cu + 1 >= 1 && cu + 1 <= n);
    const long row_bytes = 8l * sv;

    // ---- issue every load of the layer up front ------------------------------------------------
    // kappa through the caches (halo rows and straddling lines are shared with neighbouring tiles); J is touched once
    // per direction, by this lane only: loaded and stored non-temporally, so that it streams past the L2 instead of
    // evicting kappa (measured: -6.5 % time; only the load or only the store non-temporal: none, or worse)
    double K0[ROWS + 1], K1[ROWS + 1], X0[EMIT ? ROWS + 1 : 1], X1[EMIT ? ROWS + 1 : 1], Jacc[ROWS];
#pragma unroll
    for (int r = 0; r <= ROWS; ++r) {
        const int row = EDGE ? clampi(cv0 + r, 1, n) : cv0 + r;
        gcbyte *rp = kplane + row * row_bytes;
        const bool need0 = (r < ROWS) || (SHAPE == RC_TWO_V || SHAPE == RC_THREE_V);
        const bool need1 = HAS_U && ((SHAPE == RC_TWO_U) ? (r < ROWS) : (SHAPE == RC_THREE_U) ? true : (r >= 1));
        if (need0) K0[r] = *(gcdouble *)(rp + off0);
        if (need1) K1[r] = *(gcdouble *)(rp + off1);
        if (EMIT) {
            gcbyte *xp = xplane + row * row_bytes;
            if (need0) X0[r] = *(gcdouble *)(xp + off0);
            if (need1) X1[r] = *(gcdouble *)(xp + off1);
        }
    }
    constexpr int XM = EMIT ? ~0 : 0; // index mask: without emission the X arrays have one (unused) element
    const bool own_lane = lane_owned && in_u0;
#pragma unroll
    for (int r = R0; r < ROWS; ++r) Jacc[r] = 0.0;
    if (!first && own_lane) {
#pragma unroll
        for (int r = R0; r < ROWS; ++r) {
            const int row = cv0 + r;
            if ((r > 0 || row0_owned) && (!EDGE || (row >= 1 && row <= n)))
                Jacc[r] = __builtin_nontemporal_load((gcdouble *)(jplane + row * row_bytes + off0));
        }
    }

    // ---- march the rays of this lane through the layer, row by row -----------------------------
    double prev1 = 0.0, prev2 = 0.0; // 2nd / 3rd segment means of the previous row (for HAS_V gathers)
    double own0 = 0.0, side0 = 0.0;  // row 0: its own xy mean, and what lane-1 of the same row gives it
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int row = cv0 + r;
        const bool in_v0 = !EDGE || (row >= 1 && row <= n);
        const bool in_v1 = !EDGE || (row + 1 >= 1 && row + 1 <= n);

        double m0, m1 = 0.0, m2 = 0.0;
        m0 = segment<EDGE, EMIT>(K, I[r], K0[r], X0[r & XM], d0, in_v0 && in_u0, uvb);
        if (SHAPE == RC_TWO_U) m1 = segment<EDGE, EMIT>(K, I[r], K1[r], X1[r & XM], d1, in_v0 && in_u1, uvb);
        if (SHAPE == RC_TWO_V) m1 = segment<EDGE, EMIT>(K, I[r], K0[r + 1], X0[(r + 1) & XM], d1, in_v1 && in_u0, uvb);
        if (SHAPE == RC_THREE_U) {
            m1 = segment<EDGE, EMIT>(K, I[r], K1[r], X1[r & XM], d1, in_v0 && in_u1, uvb);
            m2 = segment<EDGE, EMIT>(K, I[r], K1[r + 1], X1[(r + 1) & XM], d2, in_v1 && in_u1, uvb);
        }
        if (SHAPE == RC_THREE_V) {
            m1 = segment<EDGE, EMIT>(K, I[r], K0[r + 1], X0[(r + 1) & XM], d1, in_v1 && in_u0, uvb);
            m2 = segment<EDGE, EMIT>(K, I[r], K1[r + 1], X1[(r + 1) & XM], d2, in_v1 && in_u1, uvb);
        }

        // the cell (row, cu) collects: its own xy segment, and the 2nd / 3rd segments that end
        // up in it, which belong to the rays one step lower in u and/or v
        if (r >= 1) {
            double g1 = 0.0, g2 = 0.0;
            if (SHAPE == RC_TWO_U) g1 = from_lane_below(m1);
            if (SHAPE == RC_TWO_V) g1 = prev1;
            if (SHAPE == RC_THREE_U) { g1 = from_lane_below(m1); g2 = from_lane_below(prev2); }
            if (SHAPE == RC_THREE_V) { g1 = prev1; g2 = from_lane_below(prev2); }
            double acc = m0;
            if (NSEG == 2) acc += g1;
            if (NSEG == 3) {
                // reference order: xy + xz + yz (transportRoutinesModule.f90:695-941)
                acc += THIRD_FIRST ? g2 : g1;
                acc += THIRD_FIRST ? g1 : g2;
            }
            Jacc[r] += ftte_cell_mean(acc, NSEG, w);
            // computed here, for every lane: otherwise the whole mean (selects, products) is sunk into the
            // lane-predicated store block after the last row, with every row's operands kept alive until then
            asm volatile("" : "+v"(Jacc[r]));
        } else if (STACK > 1) {
            own0 = m0;
            if (SHAPE == RC_TWO_U || SHAPE == RC_THREE_U) side0 = from_lane_below(m1);
        }
        if (HAS_V) { prev1 = m1; prev2 = m2; }
        // keep the rows in program order: their arithmetic is independent, and left alone the scheduler
        // interleaves all of them, which multiplies the live registers by the row count
        __builtin_amdgcn_sched_barrier(0);
    }

    if (STACK > 1) {
        // row 0 of every wavefront but the lowest: the row below lives in the wavefront below
        double below1 = 0.0, below2 = 0.0;
        if (HAS_V) {
            double *mine = xchg + (wid * 2) * 64;
            mine[lane] = prev1;      // my top row's 2nd-segment mean
            mine[64 + lane] = prev2; // and 3rd
            __syncthreads();
            if (row0_owned) {
                const double *theirs = xchg + ((wid - 1) * 2) * 64;
                below1 = theirs[lane];
                below2 = theirs[64 + (lane > 0 ? lane - 1 : 0)]; // the 3rd segment comes from one lane lower as well
            }
        }
        double g1 = 0.0, g2 = 0.0;
        if (SHAPE == RC_TWO_U) g1 = side0;
        if (SHAPE == RC_TWO_V) g1 = below1;
        if (SHAPE == RC_THREE_U) { g1 = side0; g2 = below2; }
        if (SHAPE == RC_THREE_V) { g1 = below1; g2 = below2; }
        double acc = own0;
        if (NSEG == 2) acc += g1;
        if (NSEG == 3) {
            acc += THIRD_FIRST ? g2 : g1;
            acc += THIRD_FIRST ? g1 : g2;
        }
        Jacc[0] += ftte_cell_mean(acc, NSEG, w);
    }

    if (own_lane) {
#pragma unroll
        for (int r = R0; r < ROWS; ++r) {
            const int row = cv0 + r;
            if ((r > 0 || row0_owned) && (!EDGE || (row >= 1 && row <= n)))
                __builtin_nontemporal_store(Jacc[r], (gdouble *)(jplane + row * row_bytes + off0));
        }
    }
}

template <int ROWS, bool EDGE, int STACK, int EMIT>
__device__ __forceinline__ void layer_dispatch(const ftte_consts &K, double (&I)[ROWS], int rc, gcbyte *kplane,
                                               gcbyte *xplane, gbyte *jplane, int cv0, int cu, int n, int sv,
                                               bool mirror_u, double d0,
                                               double d1, double d2, double w, double uvb, bool first, bool lane_owned,
                                               int lane, int wid, double *xchg)
{
#define FTTE_CASE(C)                                                                                                     \
    case C:                                                                                                              \
        layer_step<ROWS, C, EDGE, STACK, EMIT>(K, I, kplane, xplane, jplane, cv0, cu, n, sv, mirror_u, d0, d1, d2, w,   \
                                               uvb, first, lane_owned, lane, wid, xchg);                                 \
        break;
    switch (rc) {
        FTTE_CASE(RC_ONE)
        FTTE_CASE(RC_TWO_U)
        FTTE_CASE(RC_TWO_V)
        FTTE_CASE(RC_THREE_U)
        FTTE_CASE(RC_THREE_V)
        FTTE_CASE(RC_THREE_U_SWAP)
    default:
        layer_step<ROWS, RC_THREE_V_SWAP, EDGE, STACK, EMIT>(K, I, kplane, xplane, jplane, cv0, cu, n, sv, mirror_u, d0, d1,
                                                             d2, w, uvb, first, lane_owned, lane, wid, xchg);
        break;
    }
#undef FTTE_CASE
}

// grid: nitems * nnu workgroups of STACK wavefronts; the frequency group is the fastest index, so that
// (for nnu = 8) all tiles of one group run on one XCD.
template <int ROWS, int WAVES, int STACK, int EMIT>
__global__ void __launch_bounds__(64 * STACK, WAVES) sweep_kernel(const LaunchRec L)
{
    __shared__ double xchg_lds[STACK > 1 ? 2 * STACK * 2 * 64 : 1]; // [parity][wavefront][2nd|3rd][lane]
    extern __shared__ double occupancy_pad[];                        // diagnostic: dynamic LDS only limits residency
    const int nnu = L.nnu;
    const int nu = blockIdx.x % nnu;
    const WorkItem *ip = L.items + blockIdx.x / nnu;
    const int slot = uniform((int)ip->slot), tu = uniform((int)ip->tu), tv = uniform((int)ip->tv);
    const int i_first = uniform((int)ip->i_first), i_last = uniform((int)ip->i_last);
    const DirRec &D = L.dir[slot];
    const int lane = threadIdx.x & 63;
    const int wid = STACK > 1 ? uniform((int)(threadIdx.x >> 6)) : 0;
    const int n = L.n;

    const double uvb = uniform(L.uvb[nu]);
    const double w = uniform(D.w);
    const int sv = uniform(D.sv), si = uniform(D.si);
    const bool mirror_u = uniform(D.su) < 0;
    const bool first = uniform(D.first) != 0;
    const long org = uniform((long)D.org);
    gcbyte *kbase = (gcbyte *)(uniform(D.kappa) + (long)nu * L.group_stride + org);
    gbyte *jbase = (gbyte *)(uniform(D.J) + (long)nu * L.group_stride + org);
    gcbyte *xbase = EMIT ? (gcbyte *)(uniform(D.emis) + (long)nu * L.group_stride + org) : nullptr;
    const int u_lo = uniform(D.u_lo), v_lo = uniform(D.v_lo);

    // labels of this lane's rays: u label of the lane (lane 0: halo), v label of this wavefront's row 0
    // (row 0 of wavefront 0: halo)
    const int ul = u_lo + 63 * tu + lane - 1;
    const int vl0 = v_lo + (STACK * ROWS - 1) * tv - 1 + wid * ROWS;
    const bool lane_owned = lane != 0;

    double I[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) I[r] = uvb;

    const __attribute__((address_space(1))) LayerRec *layers = (const __attribute__((address_space(1))) LayerRec *)uniform(D.layers);
    int parity = 0;
    for (int i = i_first; i <= i_last; ++i) {
        const __attribute__((address_space(1))) LayerRec *rp = layers + (i - 1);
        const double d0 = uniform(rp->dpath[0]), d1 = uniform(rp->dpath[1]), d2 = uniform(rp->dpath[2]);
        const int rc = uniform(rp->info) & 7;
        const int drift = uniform(rp->drift);
        const int du = (int)(short)(drift & 0xffff), dv = drift >> 16;
        const int cu = ul + du;
        const int cv0 = vl0 + dv;
        gcbyte *kplane = kbase + 8l * i * si;
        gbyte *jplane = jbase + 8l * i * si;
        gcbyte *xplane = EMIT ? xbase + 8l * i * si : nullptr;
        double *xchg = xchg_lds + parity * (STACK * 2 * 64);
        const bool has_v = rc != RC_ONE && rc != RC_TWO_U; // this layer passes segments from row to row

        // wave-uniform position tests on every cell any lane of this wavefront may touch (halo and +1 offsets included)
        const int u_min = u_lo + 63 * tu - 1 + du, v_min = cv0;
        const bool interior = u_min >= 1 && u_min + 64 <= n && v_min >= 1 && v_min + ROWS <= n;
        const bool outside = STACK > 1 && (u_min > n || u_min + 64 < 1 || v_min > n || v_min + ROWS < 1);
        if (outside) {
            // nothing of this wavefront is in the domain at this layer: its rays keep (or, having left, no longer need)
            // the inflow value; it only has to keep the workgroup's exchange protocol going
            if (has_v) {
                xchg[(wid * 2) * 64 + lane] = 0.0;
                xchg[(wid * 2 + 1) * 64 + lane] = 0.0;
                __syncthreads();
            }
        } else if (interior)
            layer_dispatch<ROWS, false, STACK, EMIT>(L.math, I, rc, kplane, xplane, jplane, cv0, cu, n, sv, mirror_u, d0, d1,
                                                     d2, w, uvb, first, lane_owned, lane, wid, xchg);
        else
            layer_dispatch<ROWS, true, STACK, EMIT>(L.math, I, rc, kplane, xplane, jplane, cv0, cu, n, sv, mirror_u, d0, d1,
                                                    d2, w, uvb, first, lane_owned, lane, wid, xchg);
        if (STACK > 1 && has_v) parity ^= 1;
    }
}

// WAVES = waves per SIMD the register allocation is held to (512 / WAVES VGPRs per lane)
template <int ROWS, int STACK>
static int launch_variant(const LaunchRec &L, int waves, int lds_pad, dim3 grid, hipStream_t stream)
{
    const dim3 block(64 * STACK);
    switch (waves) {
    case 2: hipLaunchKernelGGL((sweep_kernel<ROWS, 2, STACK, 0>), grid, block, lds_pad, stream, L); break;
    case 3: hipLaunchKernelGGL((sweep_kernel<ROWS, 3, STACK, 0>), grid, block, lds_pad, stream, L); break;
    case 4: hipLaunchKernelGGL((sweep_kernel<ROWS, 4, STACK, 0>), grid, block, lds_pad, stream, L); break;
    case 5: hipLaunchKernelGGL((sweep_kernel<ROWS, 5, STACK, 0>), grid, block, lds_pad, stream, L); break;
    case 6: hipLaunchKernelGGL((sweep_kernel<ROWS, 6, STACK, 0>), grid, block, lds_pad, stream, L); break;
    default: return -1;
    }
    return 0;
}

int launch_sweep(const LaunchRec &L, int rows, int waves, int stack, int nnu, int lds_pad, hipStream_t stream)
{
    if (L.nitems <= 0 || nnu != L.nnu) return L.nitems <= 0 ? 0 : -1;
    const dim3 grid((unsigned)L.nitems * (unsigned)nnu);
    int rc = -1;
    if (L.emit) { // emission: one built shape (8 rows, single wavefront, 3 waves per SIMD)
        if (rows != 8 || stack != 1) return -1;
        if (L.emit == 1) hipLaunchKernelGGL((sweep_kernel<8, 3, 1, 1>), grid, dim3(64), lds_pad, stream, L);
        else hipLaunchKernelGGL((sweep_kernel<8, 3, 1, 2>), grid, dim3(64), lds_pad, stream, L);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    if (rows == 4 && stack == 1) rc = launch_variant<4, 1>(L, waves, lds_pad, grid, stream);
    else if (rows == 4 && stack == 4) rc = launch_variant<4, 4>(L, waves, lds_pad, grid, stream);
    else if (rows == 4 && stack == 8) rc = launch_variant<4, 8>(L, waves, lds_pad, grid, stream);
    else if (rows == 8 && stack == 1) rc = launch_variant<8, 1>(L, waves, lds_pad, grid, stream);
    else if (rows == 8 && stack == 2) rc = launch_variant<8, 2>(L, waves, lds_pad, grid, stream);
    else if (rows == 8 && stack == 4) rc = launch_variant<8, 4>(L, waves, lds_pad, grid, stream);
    else if (rows == 16 && stack == 1) rc = launch_variant<16, 1>(L, waves, lds_pad, grid, stream);
    if (rc) return rc;
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
