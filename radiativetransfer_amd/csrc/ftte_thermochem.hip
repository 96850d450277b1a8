// ftte_thermochem.hip -- the kernel behind ftte_advance_thermochemistry (ftte_chem.cpp): species and temperature of every leaf
// advanced together over a time step, each leaf in as many subcycles as its own time scales ask for.  The statement of a cell is
// ftte_thermochem_math.h, compiled here for the device and by the tests' host library for the host; the kernel is the grid-stride
// loop of the two advance kernels, the leaf's loads, one call into that header, the leaf's stores into the `out` buffers (copied
// in by the host once no leaf has failed), and the fold of its seven words.
#include <hip/hip_runtime.h>

#include "ftte_internal.h"
#include "ftte_thermochem.h"
#include "ftte_thermochem_math.h"

namespace ftte {

// The counter protocol of ftte_chem_fold.h for seven words: per wavefront, then per workgroup, then one atomic per workgroup
// and word.  mx[]: largest species change, largest T change (bits of non-negative doubles), largest subcycle count; sm[]:
// bisection steps, subcycles, leaves the cap bounded; bad: the first failing leaf.  For workgroups of 256.
struct ThermochemWords { unsigned long long mx[3], sm[3], bad; };

__device__ __forceinline__ void fold_thermochem(const ThermochemRec &R, ThermochemWords w)
{
    __shared__ unsigned long long blk[4][7];
    for (int off = 32; off > 0; off >>= 1) {
        for (int i = 0; i < 3; ++i) {
            const unsigned long long om = __shfl_xor(w.mx[i], off), os = __shfl_xor(w.sm[i], off);
            w.mx[i] = om > w.mx[i] ? om : w.mx[i];
            w.sm[i] += os;
        }
        const unsigned long long ob = __shfl_xor(w.bad, off);
        w.bad = ob < w.bad ? ob : w.bad;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int i = 0; i < 3; ++i) { blk[wave][i] = w.mx[i]; blk[wave][3 + i] = w.sm[i]; }
        blk[wave][6] = w.bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            for (int i = 0; i < 3; ++i) {
                w.mx[i] = blk[k][i] > w.mx[i] ? blk[k][i] : w.mx[i];
                w.sm[i] += blk[k][3 + i];
            }
            w.bad = blk[k][6] < w.bad ? blk[k][6] : w.bad;
        }
        if (w.bad != ~0ull) atomicMin(R.T.first_bad, w.bad);
        if (w.mx[0]) atomicMax(R.T.max_change, w.mx[0]);
        if (w.mx[1]) atomicMax(R.max_tchange, w.mx[1]);
        if (w.mx[2]) atomicMax(R.sub_max, w.mx[2]);
        if (w.sm[0]) atomicAdd(R.T.steps, w.sm[0]);
        if (w.sm[1]) atomicAdd(R.sub_sum, w.sm[1]);
        if (w.sm[2]) atomicAdd(R.capped, w.sm[2]);
    }
}

// HI, HeI, HeII and T of every leaf advanced over R.T.dt in at most R.max_subcycles subcycles (thermochem_advance_cell)
__global__ void __launch_bounds__(256) thermochem_advance_kernel(const ThermochemRec R)
{
    ThermochemWords w = {{0ull, 0ull, 0ull}, {0ull, 0ull, 0ull}, ~0ull};
    const ThermalRec &A = R.T;
    const ChemTable T = {R.k, A.nratec, A.logtem0, A.logtem9, A.dlogtem};
    const ThermalTable C = {A.cool, (long)A.coef_stride, (long)A.node_stride};
    for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < A.ncell; c += (long)gridDim.x * blockDim.x) {
        double p24 = 0., p25 = 0., p26 = 0., e24 = 0., e25 = 0., e26 = 0., HI, HeI, HeII, T1, logtem1, change, tchange;
        if (A.crate) {
            const double *rates = A.crate + c * kCellRec;
            p24 = rates[0]; p25 = rates[1]; p26 = rates[2]; e24 = rates[3]; e25 = rates[4]; e26 = rates[5];
        }
        unsigned long long steps;
        int subcycles, capped;
        const int ok = thermochem_advance_cell(&A.K, &T, &C, A.rho[c], A.tgas[c], R.logtem[c], A.HI[c], A.HeI[c], A.HeII[c],
                                               chem_cell_volume(A.box, A.level[c], A.n), A.crate != nullptr, p24, p25, p26, e24, e25, e26,
                                               A.run_uvb ? A.J + c : nullptr, A.ncell, R.ksi, R.uniform, A.gamma, A.uniform, A.threshold, A.comp1,
                                               A.comp2, A.hydro ? A.hydro[c] : 0., A.dt, R.eta, R.max_subcycles, A.tmin, A.tmax, &HI, &HeI, &HeII, &T1,
                                               &logtem1, &steps, &subcycles, &capped, &change, &tchange);
        w.sm[0] += steps;
        w.sm[1] += (unsigned long long)subcycles;
        w.sm[2] += (unsigned long long)capped;
        w.mx[2] = (unsigned long long)subcycles > w.mx[2] ? (unsigned long long)subcycles : w.mx[2];
        R.subcycles[c] = subcycles;
        if (!ok) w.bad = (unsigned long long)c < w.bad ? (unsigned long long)c : w.bad;
        else {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(change); // non-negative doubles order like their bits
            const unsigned long long tbits = (unsigned long long)__double_as_longlong(tchange);
            w.mx[0] = bits > w.mx[0] ? bits : w.mx[0];
            w.mx[1] = tbits > w.mx[1] ? tbits : w.mx[1];
            R.HI_out[c] = HI; R.HeI_out[c] = HeI; R.HeII_out[c] = HeII;
            A.out0[c] = T1; A.out1[c] = logtem1;
        }
    }
    fold_thermochem(R, w);
}

// (the chemistry kernels' launch shape)
int launch_thermochem_advance(const ThermochemRec &R, hipStream_t stream)
{
    const ThermalRec &A = R.T;
    if (A.ncell <= 0) return 0;
    const bool bad = A.nratec < 2 || !A.cool || !R.k || !R.logtem || !A.out0 || !A.out1 || !R.HI_out || !R.HeI_out || !R.HeII_out || !R.subcycles ||
                     !R.max_tchange || !R.sub_sum || !R.sub_max || !R.capped || R.max_subcycles < 1 || !(R.eta >= 0.) || !(A.dt > 0.) ||
                     !(A.tmin > 0.) || !(A.tmax > A.tmin);
    if (bad) return -1;
    const long blocks = (A.ncell + 255) / 256;
    hipLaunchKernelGGL(thermochem_advance_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
