// ftte_point.hip -- kernels of the point sources: the rate tables and their logarithms, the look-up, the splitting tracer, the packed
// medium and rates.  Records and launch wrappers: ftte_point_rec.h; the host side is ftte_point.h.
#include <hip/hip_runtime.h>

#include "ftte_chem_math.h"
#include "ftte_node_rec.h"
#include "ftte_point_rec.h"
#include "ftte_tables.h"

namespace ftte {

// ------------------------------------------------------------------------------------------------
// Point sources.  The reference follows each source's 12 base HEALPix rays depth-first, splitting a ray
// into its four daughter pixels when it has travelled rmax(level) cells (startNewLongRay,
// equiSources.f90:3120-3385).  Here the recursion is unrolled breadth-first by pixel level: one launch
// per level, a thread per ray; a ray that must split appends its state to a queue that seeds the next
// launch (four threads per record).  The tree walk (find/zoom??Neighbour, :2647-2960) uses node indices
// instead of the reference's call sequences: a node's position inside its parent is its index offset.
// Rates are deposited with hardware fp64 atomics (the only order-dependent step of the whole library:
// sums over rays differ in the last bits from run to run).
// ------------------------------------------------------------------------------------------------

// The look-up interpolates the logarithms of the tables.  They are kept as pairs (number rate, heating rate) of one
// reaction side by side, i1 fastest: the two i1 neighbours of both tables are 32 contiguous bytes.
//   logtab[reaction][idust][i3][i2][i1][2]
__device__ __forceinline__ size_t logtab_index(int reaction0, int flat) { return ((size_t)reaction0 * kTableSize + flat) * 2; }

// stellarBetaTable's accumulation over frequency bins, one thread per depth tuple (stellarBetaTable.f90:217-285), for every
// population of a batch: kTableBlocks workgroups per population, so a workgroup never straddles two and its population is
// a function of blockIdx alone.  bins[population][nbins], tables[population][6][11^4], logtab[population][3][11^4][2].  The bin
// index and the population are wave-uniform: the 64 bytes of a bin arrive through the scalar cache, once per wavefront.
constexpr int kTableBlocks = (kTableSize + 255) / 256, kLogTableBlocks = (3 * kTableSize + 255) / 256;

__global__ void __launch_bounds__(256) rate_table_kernel(const FreqBin *__restrict__ bins, int nbins, double *__restrict__ tables,
                                                         double *__restrict__ logtab)
{
    const int pop = blockIdx.x / kTableBlocks;
    const int t = (blockIdx.x - pop * kTableBlocks) * blockDim.x + threadIdx.x;
    if (t >= kTableSize) return;
    bins += (size_t)pop * nbins;
    tables += (size_t)pop * 6 * kTableSize;
    logtab += (size_t)pop * 6 * kTableSize;
    const int i1 = t % 11, i2 = (t / 11) % 11, i3 = (t / 121) % 11, id = t / 1331;
    // float(idepth)/float(ndepth)*maxOpticalDepth: a single-precision quotient widened, :236-242
    const double d1 = (double)((float)i1 / 10.f) * 10.0, d2 = (double)((float)i2 / 10.f) * 10.0;
    const double d3 = (double)((float)i3 / 10.f) * 10.0, dd = (double)((float)id / 10.f) * 10.0;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int b = 0; b < nbins; ++b) {
        const FreqBin B = bins[b];
        const double t1 = B.r24 * d1, t2 = B.r26 * d2, t3 = B.r25 * d3, td = B.rdust * dd;
        const double a = B.dtmp * exp(-(t1 + t2 + t3 + td));
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (B.excess[r] >= 0.0) { acc[r] = acc[r] + a; acc[3 + r] = acc[3 + r] + B.excess[r] * a; }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        tables[r * kTableSize + t] = acc[r];
        tables[(3 + r) * kTableSize + t] = acc[3 + r];
        logtab[logtab_index(r, t)] = log(acc[r]);
        logtab[logtab_index(r, t) + 1] = log(acc[3 + r]);
    }
}

// the logarithms of tables handed over, per population as above
__global__ void __launch_bounds__(256) log_table_kernel(const double *__restrict__ tables, double *__restrict__ logtab)
{
    const int pop = blockIdx.x / kLogTableBlocks;
    const int t = (blockIdx.x - pop * kLogTableBlocks) * blockDim.x + threadIdx.x;
    if (t >= 3 * kTableSize) return;
    tables += (size_t)pop * 6 * kTableSize;
    logtab += (size_t)pop * 6 * kTableSize;
    const int r = t / kTableSize, flat = t - r * kTableSize;
    logtab[logtab_index(r, flat)] = log(tables[r * kTableSize + flat]);
    logtab[logtab_index(r, flat) + 1] = log(tables[(3 + r) * kTableSize + flat]);
}

// getRatesHydrogenHelium, equiSources.f90:4157-4311, on the table of logarithms: number and heating rate of one reaction.
// The reference forms, for the lower dust slab q = idust and the upper one,
//   v_q = c1 ((1-c3)(1-c2) T(i1+1,i2,i3) + c3 (1-c2) T(i1+1,i2,i3+1) + c2 (1-c3) T(i1+1,i2+1,i3) + c3 c2 T(i1+1,i2+1,i3+1))
//       + (1-c1) (the same four with i1)
// and returns exp((1-cd) v_0 + cd v_1); the same operations in the same order here.  Without dust cd = 0 and the upper slab
// contributes 0 * v_1 = 0 exactly: it is not read.
__device__ __forceinline__ void lookup_rates(const double *__restrict__ logtab, int dust, int reaction, double tau1, double tau2,
                                             double tau3, double taud, double &number_rate, double &heating_rate)
{
    if (tau1 > 10.0 || tau2 > 10.0 || tau3 > 10.0 || taud > 10.0) { number_rate = 0.0; heating_rate = 0.0; return; }
    const int i1 = (int)(tau1 / 10.0 * 10.0), i2 = (int)(tau2 / 10.0 * 10.0), i3 = (int)(tau3 / 10.0 * 10.0);
    const double c1 = tau1 * 10.0 / 10.0 - (double)i1, c2 = tau2 * 10.0 / 10.0 - (double)i2, c3 = tau3 * 10.0 / 10.0 - (double)i3;
    int id = 0;
    double cd = 0.0;
    if (dust != 0) { id = (int)(taud / 10.0 * 10.0); cd = taud * 10.0 / 10.0 - (double)id; }
    // at tau == 10 exactly the reference reads one past the table with weight 0; stay inside
    const int s1 = i1 < 10 ? 2 : 0, s2 = i2 < 10 ? 11 : 0, s3 = i3 < 10 ? 121 : 0;
    const double w00 = (1. - c3) * (1. - c2), w01 = c3 * (1. - c2), w10 = c2 * (1. - c3), w11 = c3 * c2;
    const int nslab = (dust != 0 && id < 10) ? 2 : 1;
    double vn[2] = {0.0, 0.0}, ve[2] = {0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (q < nslab) {
            const double *P = logtab + logtab_index(reaction - 1, (((id + q) * 11 + i3) * 11 + i2) * 11 + i1);
            // corner (i2, i3): {n(i1), e(i1), n(i1+1), e(i1+1)} are contiguous
            const double *A = P, *B = P + 2 * s3, *Cc = P + 2 * s2, *D = P + 2 * (s2 + s3);
            const double a0n = A[0], a0e = A[1], a1n = A[s1], a1e = A[s1 + 1];
            const double b0n = B[0], b0e = B[1], b1n = B[s1], b1e = B[s1 + 1];
            const double c0n = Cc[0], c0e = Cc[1], c1n = Cc[s1], c1e = Cc[s1 + 1];
            const double d0n = D[0], d0e = D[1], d1n = D[s1], d1e = D[s1 + 1];
            vn[q] = c1 * (w00 * a1n + w01 * b1n + w10 * c1n + w11 * d1n) + (1. - c1) * (w00 * a0n + w01 * b0n + w10 * c0n + w11 * d0n);
            ve[q] = c1 * (w00 * a1e + w01 * b1e + w10 * c1e + w11 * d1e) + (1. - c1) * (w00 * a0e + w01 * b0e + w10 * c0e + w11 * d0e);
        }
    }
    if (dust == 0) { number_rate = exp(vn[0]); heating_rate = exp(ve[0]); return; }
    if (nslab == 1) { vn[1] = vn[0]; ve[1] = ve[0]; } // dust index 10: no slab above, weight 0
    number_rate = exp((1. - cd) * vn[0] + cd * vn[1]);
    heating_rate = exp((1. - cd) * ve[0] + cd * ve[1]);
}

struct Neighbour { int node; double a, b; bool boundary; };

__device__ __forceinline__ int node_child0(const TraceRec &T, int c) { return T.node ? T.node[c].child0 : -1; }
__device__ __forceinline__ int node_level(const TraceRec &T, int c) { return T.node ? T.node[c].level : 0; }
__device__ __forceinline__ int node_parent(const TraceRec &T, int c) { return T.node ? T.node[c].parent : -1; }
__device__ __forceinline__ int node_leaf(const TraceRec &T, int c) { return T.node ? T.node[c].leaf : c; }

// zoom??Neighbour, equiSources.f90:2827-2960: down into the leaf that holds (a,b) on the face the ray crosses.
// axis: 0 the ray crosses an x face (coordinates y,z), 1 a y face (x,z), 2 a z face (x,y).
__device__ __forceinline__ Neighbour zoom(const TraceRec &T, int c, double a, double b, int axis, int side)
{
    for (int first = node_child0(T, c); first >= 0; first = node_child0(T, c)) {
        const int ia = a < 0.5 ? 0 : 1, ib = b < 0.5 ? 0 : 1;
        a = ia ? 2. * a - 1. : 2. * a;
        b = ib ? 2. * b - 1. : 2. * b;
        const int ic = side == 0 ? 1 : 0; // coming down through the face (side 0): the child on the far side
        int i, j, k;
        if (axis == 2) { i = ia; j = ib; k = ic; }
        else if (axis == 0) { i = ic; j = ia; k = ib; }
        else { i = ia; j = ic; k = ib; }
        c = first + 4 * i + 2 * j + k;
    }
    Neighbour N;
    N.node = c; N.a = a; N.b = b; N.boundary = false;
    return N;
}

// find??Neighbour, equiSources.f90:2647-2825
__device__ __forceinline__ Neighbour find_neighbour(const TraceRec &T, int c, double a, double b, int axis, int side)
{
    const int pos = axis == 2 ? 2 : (axis == 0 ? 0 : 1);
    const int pa = axis == 2 ? 0 : (axis == 0 ? 1 : 0), pb = axis == 2 ? 1 : 2;
    int lvl = node_level(T, c);
    while (lvl > 0) {
        const int par = node_parent(T, c);
        const int first = node_child0(T, par);
        const int idx = c - first;
        int ijk[3] = {(idx >> 2) & 1, (idx >> 1) & 1, idx & 1};
        if ((side == 0 && ijk[pos] == 0) || (side == 1 && ijk[pos] == 1)) {
            a = ijk[pa] == 0 ? 0.5 * a : 0.5 * a + 0.5;
            b = ijk[pb] == 0 ? 0.5 * b : 0.5 * b + 0.5;
            c = par;
            --lvl;
        } else {
            ijk[pos] = side == 0 ? 0 : 1;
            return zoom(T, first + 4 * ijk[0] + 2 * ijk[1] + ijk[2], a, b, axis, side);
        }
    }
    const int n = T.n;
    int ijk[3] = {c / (n * n), (c / n) % n, c % n};
    if ((side == 0 && ijk[pos] == 0) || (side == 1 && ijk[pos] == n - 1)) {
        Neighbour N;
        N.node = -1; N.a = a; N.b = b; N.boundary = true;
        return N;
    }
    ijk[pos] += side == 0 ? -1 : 1;
    return zoom(T, (ijk[0] * n + ijk[1]) * n + ijk[2], a, b, axis, side);
}

__global__ void __launch_bounds__(64) point_trace_kernel(const TraceRec T)
{
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= T.nrays) return;
    const int L = T.pixel_level;
    const int n = T.n;
    const double fn = (double)(float)n;
    int pixel, cell, src;
    double pt[3], radius, d1, d2, d3, dd, ndot;
    const int level_off = 4 * ((1 << (2 * (L - 1))) - 1); // 12 (4^(L-1) - 1) / 3

    if (L == 1) {
        const int s = tid / 12;
        src = s;
        pixel = tid % 12;
        cell = T.src_node[s];
        pt[0] = pt[1] = pt[2] = 0.5;
        radius = 0.0; d1 = d2 = d3 = dd = 0.0;
        ndot = T.src_ndot[s] / 12.0;
    } else {
        const SplitRec R = T.in[tid >> 2];
        const int which = tid & 3;
        pixel = 4 * R.pixel + which;
        const double *pd = T.pixdir + 3 * (size_t)(4 * ((1 << (2 * (L - 2))) - 1) + R.pixel);
        double base[3] = {0, 0, 0};
        // the reference walks the four daughters in order and gives up on the rest once one starts outside the box
        // (strategy = boundary is never reset, equiSources.f90:3336-3345): daughter `which` exists only if it and all
        // its elder sisters start inside
        src = R.src;
        bool elder_outside = false;
        for (int sis = 0; sis <= which; ++sis) {
            const double *cd = T.pixdir + 3 * (size_t)(level_off + 4 * R.pixel + sis);
            base[0] = R.pos[0] + R.radius / fn * (cd[0] - pd[0]);
            base[1] = R.pos[1] + R.radius / fn * (cd[1] - pd[1]);
            base[2] = R.pos[2] + R.radius / fn * (cd[2] - pd[2]);
            const bool outside = base[0] < 0. || base[0] > 1. || base[1] < 0. || base[1] > 1. || base[2] < 0. || base[2] > 1.;
            if (outside && sis == which && T.escape) {
                // a daughter that starts outside the box counts as gone through the boundary, whatever her elder sisters did
                // (:3336-3343 is evaluated for every daughter)
                const double tmp = R.radius * T.box / (fn * T.kpc);
                double *E = T.escape + (size_t)src * kEscapeRec;
                for (int ir = 0; ir < kOutputRadii; ++ir)
                    if (T.out_radius_kpc[ir] > tmp) unsafeAtomicAdd(E + kOutputRadii + ir, R.ndot / 4.);
            }
            elder_outside = elder_outside || outside;
        }
        if (elder_outside) return;
        // localizeSplitContinuationCell, :3049-3118
        int ijk[3];
        for (int q = 0; q < 3; ++q) {
            ijk[q] = (int)(base[q] * n);
            if (ijk[q] < 0 || ijk[q] >= n) { atomicMax(T.error, 1); return; }
            pt[q] = base[q] * fn - (double)(float)ijk[q];
        }
        cell = (ijk[0] * n + ijk[1]) * n + ijk[2];
        for (int first = node_child0(T, cell); first >= 0; first = node_child0(T, cell)) {
            int h[3];
            for (int q = 0; q < 3; ++q) { h[q] = pt[q] < 0.5 ? 0 : 1; pt[q] = h[q] ? 2. * pt[q] - 1. : 2. * pt[q]; }
            cell = first + 4 * h[0] + 2 * h[1] + h[2];
        }
        radius = R.radius; d1 = R.depth[0]; d2 = R.depth[1]; d3 = R.depth[2]; dd = R.depth[3];
        ndot = R.ndot / 4.0;
    }
    if (pt[0] < 0. || pt[0] > 1. || pt[1] < 0. || pt[1] > 1. || pt[2] < 0. || pt[2] > 1.) { atomicMax(T.error, 2); return; }
    // the tables of this star's population.  `src` counts from the first star of the batch, like T.escape: T.slot_of and
    // T.highest_level start there too
    const double *logtab = T.slot_of ? T.logtab + (size_t)T.slot_of[src] * T.slot_stride : T.logtab;

    const double *dir = T.pixdir + 3 * (size_t)(level_off + pixel);
    const double prox = dir[0], proy = dir[1], proz = dir[2];
    const double rm = T.rmax[L];
    bool split = false;
    unsigned crossed = 0;
    for (int step = 0; step < 1000000; ++step) {
        ++crossed;
        // ---- drawSegment, :2412-2595
        const int lvl = node_level(T, cell);
        const double scale = (double)(1 << lvl);
        const double t1 = proz > 0. ? (1. - pt[2]) / proz : -pt[2] / proz;
        const double t2 = prox > 0. ? (1. - pt[0]) / prox : -pt[0] / prox;
        const double t3 = proy > 0. ? (1. - pt[1]) / proy : -pt[1] / proy;
        int axis;
        double len;
        if (t1 < fmin(t2, t3)) { axis = 2; len = t1; }
        else if (t2 < fmin(t1, t3)) { axis = 0; len = t2; }
        else { axis = 1; len = t3; }
        bool stop = false;
        Neighbour N;
        N.node = -1; N.a = N.b = 0.0; N.boundary = false;
        int side = 0;
        const double old_radius = radius;
        if (radius * scale + len < rm || L == kMaxPixelLevel) {
            radius = radius + len / scale;
            const double ex = pt[0] + len * prox, ey = pt[1] + len * proy, ez = pt[2] + len * proz;
            if (axis == 2) { side = proz < 0. ? 0 : 1; N = find_neighbour(T, cell, ex, ey, 2, side); }
            else if (axis == 0) { side = prox < 0. ? 0 : 1; N = find_neighbour(T, cell, ey, ez, 0, side); }
            else { side = proy < 0. ? 0 : 1; N = find_neighbour(T, cell, ex, ez, 1, side); }
            stop = N.boundary;
        } else if (radius * scale >= rm) {
            split = true; len = 0.0;
        } else {
            split = true;
            len = rm - radius * scale;
            radius = radius + len / scale;
            pt[0] = pt[0] + len * prox; pt[1] = pt[1] + len * proy; pt[2] = pt[2] + len * proz;
        }
        // ---- optical depths of the piece and what it absorbs, :3176-3269
        const double cell_size = T.box / ((double)((float)(1 << lvl) * (float)n));
        const double path = cell_size * len;
        const long c = node_leaf(T, cell);
        const double *M = T.medium + c * kCellRec; // HI, HeI, HeII, rho, abun2
        const double hi = M[0];
        const double tau1 = path * hi * FTTE_SIGMA_HI, tau2 = path * M[1] * FTTE_SIGMA_HEI, tau3 = path * M[2] * FTTE_SIGMA_HEII;
        double taud = 0.0;
        if (T.dust == 1) taud = path * hi * (double)5.4116737e-22f * M[4] / (double)0.2f;
        else if (T.dust == 2) taud = path * FTTE_PSI * M[3] / FTTE_MH * (double)5.4116737e-22f * M[4] / (double)0.2f;
        if (T.escape) { // :3198-3233: what is left of the ray where it crosses the output radii, what leaves through the box faces
            double *E = T.escape + (size_t)src * kEscapeRec;
            const double tmp1 = old_radius * T.box / fn, tmp2 = radius * T.box / fn;
            for (int ir = 0; ir < kOutputRadii; ++ir) {
                const double tmp = T.out_radius_kpc[ir] * T.kpc;
                if (tmp >= tmp1 && tmp <= tmp2) {
                    const double ratio = (tmp - tmp1) / (tmp2 - tmp1);
                    unsafeAtomicAdd(E + ir, ndot * exp(-(ratio * (tau1 + taud) + d1 + dd)));
                    if (ir == kOutputRadii - 1) {
                        const double o1 = ratio * tau1 + d1, o2 = ratio * tau2 + d2, o3 = ratio * tau3 + d3, od = ratio * taud + dd;
                        unsafeAtomicAdd(E + 2 * kOutputRadii, ndot * exp(-od));
                        if (T.sigma_ratio)
                            for (int ie = 0; ie < kOutputEnergies; ++ie) {
                                const double e1 = T.sigma_ratio[ie] * o1, e2 = T.sigma_ratio[2 * kOutputEnergies + ie] * o2,
                                             e3 = T.sigma_ratio[kOutputEnergies + ie] * o3, e4 = T.sigma_ratio[3 * kOutputEnergies + ie] * od;
                                unsafeAtomicAdd(E + 2 * kOutputRadii + 1 + ie, ndot * exp(-(e1 + e2 + e3 + e4)));
                            }
                    }
                }
            }
            if (stop) { // drawSegment ended on a box face (the depth test below is not a boundary in this sense)
                const double tmp = radius * T.box / (fn * T.kpc);
                for (int ir = 0; ir < kOutputRadii; ++ir)
                    if (T.out_radius_kpc[ir] > tmp) unsafeAtomicAdd(E + kOutputRadii + ir, ndot);
            }
        }
        if (fmin(fmin(d1 + tau1, d2 + tau2), fmin(d3 + tau3, dd + taud)) > 100.) { stop = true; split = false; }
        // a species without opacity in this cell takes nothing from the ray: R(d) - R(d) = 0 (and the reference adds that 0)
        double a, b, ea, eb;
        double *K = T.rates + c * kCellRec; // krate24, krate25, krate26, crate24, crate25, crate26
        if (tau1 != 0.0) {
            lookup_rates(logtab, T.dust, 1, d1, d2, d3, dd, a, ea);
            lookup_rates(logtab, T.dust, 1, d1 + tau1, d2, d3, dd, b, eb);
            unsafeAtomicAdd(K + 0, ndot * (a - b));
            unsafeAtomicAdd(K + 3, ndot * (ea - eb));
        }
        if (tau2 != 0.0) {
            lookup_rates(logtab, T.dust, 2, d1, d2, d3, dd, a, ea);
            lookup_rates(logtab, T.dust, 2, d1, d2 + tau2, d3, dd, b, eb);
            unsafeAtomicAdd(K + 2, ndot * (a - b));
            unsafeAtomicAdd(K + 5, ndot * (ea - eb));
        }
        if (tau3 != 0.0) {
            lookup_rates(logtab, T.dust, 3, d1, d2, d3, dd, a, ea);
            lookup_rates(logtab, T.dust, 3, d1, d2, d3 + tau3, dd, b, eb);
            unsafeAtomicAdd(K + 1, ndot * (a - b));
            unsafeAtomicAdd(K + 4, ndot * (ea - eb));
        }
        d1 = d1 + tau1; d2 = d2 + tau2; d3 = d3 + tau3; dd = dd + taud;
        if (stop || split) break;
        // ---- into the neighbour, :2512-2558
        const double face = side == 0 ? 1. : 0.;
        if (axis == 2) { pt[2] = face; pt[0] = N.a; pt[1] = N.b; }
        else if (axis == 0) { pt[0] = face; pt[1] = N.a; pt[2] = N.b; }
        else { pt[1] = face; pt[0] = N.a; pt[2] = N.b; }
        if (pt[0] < 0. || pt[0] > 1. || pt[1] < 0. || pt[1] > 1. || pt[2] < 0. || pt[2] > 1.) { atomicMax(T.error, 3); return; }
        cell = N.node;
        if (step == 999999) atomicMax(T.error, 4);
    }
    atomicAdd(T.steps, (unsigned long long)crossed);
    if (!split) return;

    // ---- hand the ray over to its four daughters: absoluteCoordinates, :3011-3047
    atomicMax(T.highest_level + src, L + 1);
    double p[3] = {pt[0], pt[1], pt[2]};
    int c = cell;
    for (int lvl = node_level(T, c); lvl > 0; --lvl) {
        const int par = node_parent(T, c);
        const int idx = c - node_child0(T, par);
        const int h[3] = {(idx >> 2) & 1, (idx >> 1) & 1, idx & 1};
        for (int q = 0; q < 3; ++q) p[q] = h[q] == 0 ? 0.5 * p[q] : 0.5 * p[q] + 0.5;
        c = par;
    }
    const int bi[3] = {c / (n * n), (c / n) % n, c % n};
    const int slot = atomicAdd(T.out_count, 1);
    if (slot >= T.out_capacity) { atomicMax(T.error, 5); return; }
    SplitRec R;
    for (int q = 0; q < 3; ++q) R.pos[q] = ((double)(float)bi[q] + p[q]) / fn;
    R.radius = radius;
    R.depth[0] = d1; R.depth[1] = d2; R.depth[2] = d3; R.depth[3] = dd;
    R.ndot = ndot;
    R.pixel = pixel;
    R.src = src;
    T.out[slot] = R;
}

// getRatesHydrogenHelium for a list of depth tuples: tau[nsample][4] -> out[nsample][3][2] (number rate, heating rate)
__global__ void __launch_bounds__(256) rate_lookup_kernel(const double *__restrict__ logtab, int dust, int nsample,
                                                          const double *__restrict__ tau, double *__restrict__ out)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsample) return;
    for (int r = 1; r <= 3; ++r) {
        double a, e;
        lookup_rates(logtab, dust, r, tau[4 * s], tau[4 * s + 1], tau[4 * s + 2], tau[4 * s + 3], a, e);
        out[6 * s + 2 * (r - 1)] = a;
        out[6 * s + 2 * (r - 1) + 1] = e;
    }
}

int launch_rate_lookup(const double *logtab, int dust, int nsample, const double *tau, double *out, hipStream_t stream)
{
    if (nsample <= 0) return 0;
    hipLaunchKernelGGL(rate_lookup_kernel, dim3((nsample + 255) / 256), dim3(256), 0, stream, logtab, dust, nsample, tau, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// packed[c][0..4] = HI, HeI, HeII, rho, abun2 (one 64-byte line per cell)
__global__ void __launch_bounds__(256) pack_medium_kernel(const double *__restrict__ HI, const double *__restrict__ HeI,
                                                          const double *__restrict__ HeII, const double *__restrict__ rho,
                                                          const double *__restrict__ abun2, double *__restrict__ packed, long ncell)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long c = t >> 3;
    const int f = (int)(t & 7);
    if (c >= ncell) return;
    const double *src = f == 0 ? HI : f == 1 ? HeI : f == 2 ? HeII : f == 3 ? rho : f == 4 ? abun2 : nullptr;
    packed[t] = src ? src[c] : 0.0;
}

// to_packed: packed[c][r] = planes[r][c] (r < 6), else planes[r][c] = packed[c][r]; tiles of 32 cells through LDS so that
// both sides move whole lines
__global__ void __launch_bounds__(256) repack_rates_kernel(double *__restrict__ planes, double *__restrict__ packed, long ncell,
                                                           int to_packed)
{
    __shared__ double tile[8][33];
    const long c0 = (long)blockIdx.x * 32;
    const int a = threadIdx.x & 31, b = threadIdx.x >> 5; // 32 x 8
    if (to_packed) {
        tile[b][a] = (b < 6 && c0 + a < ncell) ? planes[(long)b * ncell + c0 + a] : 0.0;
        __syncthreads();
        const int cc = threadIdx.x >> 3, r = threadIdx.x & 7;
        if (c0 + cc < ncell) packed[(c0 + cc) * kCellRec + r] = tile[r][cc];
    } else {
        const int cc = threadIdx.x >> 3, r = threadIdx.x & 7;
        tile[r][cc] = c0 + cc < ncell ? packed[(c0 + cc) * kCellRec + r] : 0.0;
        __syncthreads();
        if (b < 6 && c0 + a < ncell) planes[(long)b * ncell + c0 + a] = tile[b][a];
    }
}

int launch_pack_medium(const double *const field[5], double *packed, long ncell, hipStream_t stream)
{
    const long threads = ncell * kCellRec;
    hipLaunchKernelGGL(pack_medium_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, field[0], field[1], field[2],
                       field[3], field[4], packed, ncell);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_repack_rates(double *planes, double *packed, long ncell, bool to_packed, hipStream_t stream)
{
    hipLaunchKernelGGL(repack_rates_kernel, dim3((unsigned)((ncell + 31) / 32)), dim3(256), 0, stream, planes, packed, ncell,
                       to_packed ? 1 : 0);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_rate_table(const FreqBin *bins, int nbins, int npop, double *tables, double *logtab, hipStream_t stream)
{
    if (npop <= 0) return 0;
    hipLaunchKernelGGL(rate_table_kernel, dim3((unsigned)npop * kTableBlocks), dim3(256), 0, stream, bins, nbins, tables, logtab);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_log_table(const double *tables, int npop, double *logtab, hipStream_t stream)
{
    if (npop <= 0) return 0;
    hipLaunchKernelGGL(log_table_kernel, dim3((unsigned)npop * kLogTableBlocks), dim3(256), 0, stream, tables, logtab);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_point_trace(const TraceRec &T, hipStream_t stream)
{
    if (T.nrays <= 0) return 0;
    hipLaunchKernelGGL(point_trace_kernel, dim3((T.nrays + 63) / 64), dim3(64), 0, stream, T);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
