// ftte_leaf.h -- the per-leaf updates (ftte_leaf_pass.cpp; kernels: ftte_chem.hip, ftte_thermal.hip, ftte_thermochem.hip): the
// launch records, filled from one head, their launch wrappers (asynchronous on `stream`; return 0, -1 bad argument, -2 launch
// failure), and for device code what the six kernels share: the loop over the leaves, the load of a leaf's point-source rates, the
// two statistics a leaf contributes by comparison, the fold of a kernel's statistics and the launch shape.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "ftte_math.h"
#include "ftte_point_rec.h"

namespace ftte {

// What every per-leaf update reads, filled in one place (leaf_pass); the chemistry's records embed it, the thermal ones take it in
struct LeafRec {
    // cell arrays, cell-array order
    const int8_t *level;       // per leaf (not per node)
    const double *rho;
    const double *HI, *HeI, *HeII; // state on entry
    const double *rates;       // [ncell][kCellRec] packed point-source rates (krate24..26 at +0..+2, crate24..26 at +3..+5) or nullptr
    const double *J;           // [3][ncell] or nullptr (uniform background)
    unsigned long long *first_bad;  // lowest cell index at which the update stops, or ~0
    unsigned long long *max_change; // bits of the largest change
    unsigned long long *steps;      // bisection steps taken, all cells
    int64_t ncell;
    int32_t n, nratec, run_uvb;
    double box, logtem0, logtem9, dlogtem;
    double table[9];           // [group][3]: ksi24, ksi25, ksi26 for the chemistry, gammaHI, gammaHeI, gammaHeII for the heating
    double uniform[3];         // uniformQuasar * quasar% + uniformStellar * stellar% of the same integrals, per reaction
    double threshold;          // selfShieldingThreshold
};

// ---- ionisation equilibrium (solveRateEquations, equiSources.f90:3459-3677), the start-up equilibrium, the advance over dt
struct ChemRec {
    LeafRec L;
    const double *logtem;
    double *HI_out, *HeI_out, *HeII_out; // state on return
    const double *k;           // [6][nratec] rate coefficients k1a..k6a
    int32_t passes;            // initial_equilibrium_kernel only
    int32_t substeps;          // advance_equations_kernel only: the time to advance over [s], in `substeps` equal steps
    double dt;
};

// ---- thermal balance (thermalEquilibrium, equiSources.f90:3870-4042) and the temperature advanced over dt
constexpr int kCoolNode = 16; // doubles per temperature node in the device's node-major cooling table: thirteen used, 128 bytes

// The thermal kernels keep a record of their own form, the head's fields among their own in the order below, and the coupled kernel
// with them: with LeafRec embedded in front, whichever way its fields were ordered, the compiler kept more of the advance kernels'
// scalar registers in vector lanes and read them back inside the bisection, or laid the coupled kernel out 3.5 % slower
// (profiles/README.md).  put_head copies the head in.
struct ThermalRec {
    // cell arrays, cell-array order
    const int8_t *level;       // per leaf
    const double *rho, *tgas;
    const double *HI, *HeI, *HeII;
    const double *crate;       // the head's `rates` (crate24..26 at +3..+5)
    const double *J;
    const double *hydro;       // advance: the stored hydroHeating to add, or nullptr
    double *out0, *out1, *out2; // equilibrium: heating, cooling, hydroHeating; advance: tgas, logtem (out2 unused)
    const double *cool;        // the cooling coefficients, coefficient r of node i at cool[r * coef_stride + i * node_stride]
    int64_t coef_stride, node_stride;
    int64_t ncell;
    int32_t n, nratec, run_uvb, substeps;
    double box, logtem0, logtem9, dlogtem;
    double gamma[9];           // the head's `table`: [group][gammaHI, gammaHeI, gammaHeII]
    double uniform[3];
    double threshold;
    double comp1, comp2;       // compa (1+z)^4, 2.73 (1+z)
    double dt, tmin, tmax;     // advance only
    unsigned long long *first_bad, *max_change, *steps;
    ftte_consts K;
};

// ---- species and temperature advanced together over dt, each leaf in subcycles of its own (ftte_thermochem_math.h): the thermal
// advance's record (out0 = T, out1 = logtem; max_change = the species') and what the chemistry adds to it
struct ThermochemRec {
    ThermalRec T;
    const double *logtem;      // per leaf: the stored logarithm the first subcycle's chemistry reads
    const double *k;           // [6][nratec] rate coefficients k1a..k6a
    double *HI_out, *HeI_out, *HeII_out;
    int32_t *subcycles;        // per leaf: the subcycles it took
    double ksi[9];             // [group][ksi24, ksi25, ksi26]
    double uniform[3];         // the uniform background's ionisation rates, per reaction
    double eta;
    int32_t max_subcycles;
    // bits of the largest |T1 - T0| / T0, sum of the subcycles, largest subcycle count of a leaf, leaves the cap bounded
    unsigned long long *max_tchange, *sub_sum, *sub_max, *capped;
};

// the filled head into a record
inline void put_head(ChemRec &R, const LeafRec &L) { R.L = L; }
inline void put_head(ThermalRec &R, const LeafRec &L)
{
    R.level = L.level; R.rho = L.rho; R.HI = L.HI; R.HeI = L.HeI; R.HeII = L.HeII; R.crate = L.rates; R.J = L.J;
    R.ncell = L.ncell; R.n = L.n; R.nratec = L.nratec; R.run_uvb = L.run_uvb;
    R.box = L.box; R.logtem0 = L.logtem0; R.logtem9 = L.logtem9; R.dlogtem = L.dlogtem; R.threshold = L.threshold;
    for (int i = 0; i < 9; ++i) R.gamma[i] = L.table[i];
    for (int i = 0; i < 3; ++i) R.uniform[i] = L.uniform[i];
    R.first_bad = L.first_bad; R.max_change = L.max_change; R.steps = L.steps;
}
inline void put_head(ThermochemRec &R, const LeafRec &L) { put_head(R.T, L); }

// ionisation equilibrium of every leaf (solveRateEquations)
int launch_rate_equations(const ChemRec &R, hipStream_t stream);
// the start-up equilibrium (initialIonizationEquilibrium), R.passes times per leaf; L.rates, L.J, L.run_uvb, L.table unused
int launch_initial_equilibrium(const ChemRec &R, hipStream_t stream);
// HI, HeI, HeII of every leaf advanced over R.dt in R.substeps implicit steps; R.passes unused
int launch_advance_equations(const ChemRec &R, hipStream_t stream);
int launch_thermal_equilibrium(const ThermalRec &R, hipStream_t stream);
int launch_thermal_advance(const ThermalRec &R, hipStream_t stream);
int launch_thermochem_advance(const ThermochemRec &R, hipStream_t stream);

} // namespace ftte

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace ftte {

// every leaf once, a few leaves per thread (a macro and no function that takes the body: that one cost every kernel two registers,
// and rate_equations_kernel a wavefront per SIMD with them)
#define FTTE_FOR_LEAVES(c, ncell) for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < (ncell); c += (long)gridDim.x * blockDim.x)

// the three point-source rates of leaf c at `offset` of its packed record (0: krate24..26, 3: crate24..26); zeros without point rates
__device__ __forceinline__ void load_point_rates(const double *rates, long c, int offset, double &r24, double &r25, double &r26)
{
    r24 = r25 = r26 = 0.;
    if (rates) { r24 = rates[c * kCellRec + offset]; r25 = rates[c * kCellRec + offset + 1]; r26 = rates[c * kCellRec + offset + 2]; }
}

__device__ __forceinline__ void note_bad(unsigned long long &bad, long c) { bad = (unsigned long long)c < bad ? (unsigned long long)c : bad; }

// non-negative doubles order like their bits
__device__ __forceinline__ void note_change(unsigned long long &most, double change)
{
    const unsigned long long bits = (unsigned long long)__double_as_longlong(change);
    most = bits > most ? bits : most;
}

// The statistics of an update as one thread gathers them: kMax words that take the maximum, kSum words that add up, and the first
// leaf the update stops at
template <int kMax, int kSum> struct LeafWords {
    unsigned long long mx[kMax ? kMax : 1] = {}, sm[kSum ? kSum : 1] = {}, bad = ~0ull;
};

// The counter protocol: the words are combined per wavefront, then per workgroup, before thread 0 sends each that says anything to
// its single word in memory with one atomic: a quarter of a million atomics on ONE address each cost more than all the arithmetic
// of a kernel.  For workgroups of 256.
template <int kMax, int kSum>
__device__ __forceinline__ void fold_words(LeafWords<kMax, kSum> w, unsigned long long *first_bad, unsigned long long *const (&max_to)[kMax ? kMax : 1],
                                           unsigned long long *const (&sum_to)[kSum ? kSum : 1])
{
    __shared__ unsigned long long blk[4][kMax + kSum + 1];
    for (int off = 32; off > 0; off >>= 1) {
        for (int i = 0; i < kMax; ++i) { const unsigned long long o = __shfl_xor(w.mx[i], off); w.mx[i] = o > w.mx[i] ? o : w.mx[i]; }
        for (int i = 0; i < kSum; ++i) w.sm[i] += __shfl_xor(w.sm[i], off);
        const unsigned long long ob = __shfl_xor(w.bad, off);
        w.bad = ob < w.bad ? ob : w.bad;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int i = 0; i < kMax; ++i) blk[wave][i] = w.mx[i];
        for (int i = 0; i < kSum; ++i) blk[wave][kMax + i] = w.sm[i];
        blk[wave][kMax + kSum] = w.bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            for (int i = 0; i < kMax; ++i) w.mx[i] = blk[k][i] > w.mx[i] ? blk[k][i] : w.mx[i];
            for (int i = 0; i < kSum; ++i) w.sm[i] += blk[k][kMax + i];
            w.bad = blk[k][kMax + kSum] < w.bad ? blk[k][kMax + kSum] : w.bad;
        }
        if (w.bad != ~0ull) atomicMin(first_bad, w.bad);
        for (int i = 0; i < kMax; ++i) if (w.mx[i]) atomicMax(max_to[i], w.mx[i]);
        for (int i = 0; i < kSum; ++i) if (w.sm[i]) atomicAdd(sum_to[i], w.sm[i]);
    }
}

// the fold of a kernel with the head's three words alone: with the largest change (1, 1) or without it (0, 1)
template <int kMax>
__device__ __forceinline__ void fold_head_words(const LeafWords<kMax, 1> &w, unsigned long long *first_bad, unsigned long long *max_change,
                                                unsigned long long *steps)
{
    unsigned long long *const max_to[1] = {max_change}, *const sum_to[1] = {steps};
    fold_words<kMax, 1>(w, first_bad, max_to, sum_to);
}

// The launch shape: enough workgroups to fill the GPU several times over, few enough that their atomics are nothing
template <typename Rec> int launch_over_leaves(void (*kernel)(const Rec), const Rec &R, int64_t ncell, hipStream_t stream)
{
    if (ncell <= 0) return 0;
    const long blocks = (ncell + 255) / 256;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
#endif
