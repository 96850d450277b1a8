// ftte_chem.hip -- the kernels behind the chemistry's per-leaf updates (ftte_leaf_pass.cpp) and ftte_chem.cpp: the ionisation equilibrium
// of every leaf (solveRateEquations, initialIonizationEquilibrium), its advance over a time step, the optically thin radiation field,
// the hydrogen census and the opacities.  The chemistry of a cell is ftte_chem_math.h, compiled here for the device and by the tests'
// host library for the host; a per-leaf kernel is the loop over the leaves, the leaf's loads, one call into that header and the
// leaf's stores, and then the fold of its statistics (all of ftte_leaf.h).
#include <hip/hip_runtime.h>

#include "ftte_chem.h"
#include "ftte_chem_math.h"
#include "ftte_leaf.h"
#include "ftte_tree_sum.h"

namespace ftte {

// solveRateEquations, equiSources.f90:3459-3677, per leaf (chem_solve_cell)
__global__ void __launch_bounds__(256) rate_equations_kernel(const ChemRec R)
{
    const LeafRec &L = R.L;
    LeafWords<1, 1> w;
    const ChemTable T = {R.k, L.nratec, L.logtem0, L.logtem9, L.dlogtem};
    FTTE_FOR_LEAVES(c, L.ncell) {
        double p24, p25, p26, HI, HeI, HeII, change;
        load_point_rates(L.rates, c, 0, p24, p25, p26);
        unsigned steps; int tame;
        const int ok = chem_solve_cell(&T, L.rho[c], R.logtem[c], L.HI[c], L.HeI[c], L.HeII[c], chem_cell_volume(L.box, L.level[c], L.n),
                                       L.rates != nullptr, p24, p25, p26, L.run_uvb ? L.J + c : nullptr, L.ncell, L.table, L.uniform, L.threshold,
                                       &HI, &HeI, &HeII, &steps, &change, &tame);
        if (!ok) note_bad(w.bad, c);
        else {
            note_change(w.mx[0], change);
            w.sm[0] += (unsigned long long)steps;
            R.HI_out[c] = HI; R.HeI_out[c] = HeI; R.HeII_out[c] = HeII;
        }
    }
    fold_head_words(w, L.first_bad, L.max_change, L.steps);
}

// The start-up ionisation equilibrium, initialIonizationEquilibrium (equiSources.f90:3679-3868), R.passes times per leaf
// (chem_initial_cell).  L.rates, L.J, L.run_uvb, L.table are not used.
__global__ void __launch_bounds__(256) initial_equilibrium_kernel(const ChemRec R)
{
    const LeafRec &L = R.L;
    LeafWords<0, 1> w;
    const ChemTable T = {R.k, L.nratec, L.logtem0, L.logtem9, L.dlogtem};
    FTTE_FOR_LEAVES(c, L.ncell) {
        double HI, HeI, HeII;
        unsigned long long steps;
        const int ok = chem_initial_cell(&T, L.rho[c], R.logtem[c], L.HI[c], L.HeI[c], L.HeII[c], L.uniform, L.threshold, R.passes, &HI, &HeI,
                                         &HeII, &steps);
        w.sm[0] += steps;
        if (!ok) note_bad(w.bad, c);
        else { R.HI_out[c] = HI; R.HeI_out[c] = HeI; R.HeII_out[c] = HeII; }
    }
    fold_head_words(w, L.first_bad, L.max_change, L.steps);
}

// HI, HeI, HeII of every leaf advanced over R.dt in R.substeps implicit steps at the rates of the state on entry (chem_advance_cell)
__global__ void __launch_bounds__(256) advance_equations_kernel(const ChemRec R)
{
    const LeafRec &L = R.L;
    LeafWords<1, 1> w;
    const ChemTable T = {R.k, L.nratec, L.logtem0, L.logtem9, L.dlogtem};
    FTTE_FOR_LEAVES(c, L.ncell) {
        double p24, p25, p26, HI, HeI, HeII, change;
        load_point_rates(L.rates, c, 0, p24, p25, p26);
        unsigned long long steps;
        const int ok = chem_advance_cell(&T, L.rho[c], R.logtem[c], L.HI[c], L.HeI[c], L.HeII[c], chem_cell_volume(L.box, L.level[c], L.n),
                                         L.rates != nullptr, p24, p25, p26, L.run_uvb ? L.J + c : nullptr, L.ncell, L.table, L.uniform, L.threshold,
                                         R.dt, R.substeps, &HI, &HeI, &HeII, &steps, &change);
        w.sm[0] += steps;
        if (!ok) note_bad(w.bad, c);
        else {
            note_change(w.mx[0], change);
            R.HI_out[c] = HI; R.HeI_out[c] = HeI; R.HeII_out[c] = HeII;
        }
    }
    fold_head_words(w, L.first_bad, L.max_change, L.steps);
}

int launch_rate_equations(const ChemRec &R, hipStream_t stream) { return launch_over_leaves(rate_equations_kernel, R, R.L.ncell, stream); }

int launch_initial_equilibrium(const ChemRec &R, hipStream_t stream)
{
    return R.L.ncell > 0 && R.passes < 1 ? -1 : launch_over_leaves(initial_equilibrium_kernel, R, R.L.ncell, stream);
}

int launch_advance_equations(const ChemRec &R, hipStream_t stream)
{
    return R.L.ncell > 0 && (R.substeps < 1 || !(R.dt > 0.)) ? -1 : launch_over_leaves(advance_equations_kernel, R, R.L.ncell, stream);
}

// assignUvbRadiation, transportRoutinesModule.f90:1056-1093: the optically thin alternative to the sweep.  J_g = uvb_g where the
// Lyman-limit mean free path of the cell is at least the self-shielding threshold, else 0.
__global__ void __launch_bounds__(256) thin_limit_kernel(const double *__restrict__ HI, const double *__restrict__ HeI,
                                                         const double *__restrict__ HeII, const double *__restrict__ rho,
                                                         const double *__restrict__ uvb, double threshold, double *__restrict__ J,
                                                         long ncell, int nnu)
{
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    const bool lit = chem_mean_free_path(fmin(HI[c], chem_nh(rho[c])), HeI[c], HeII[c]) >= threshold;
    for (int g = 0; g < nnu; ++g) J[(long)g * ncell + c] = lit ? uvb[g] : 0.0;
}

int launch_thin_limit(const double *HI, const double *HeI, const double *HeII, const double *rho, const double *uvb, double threshold,
                      double *J, long ncell, int nnu, hipStream_t stream)
{
    hipLaunchKernelGGL(thin_limit_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, stream, HI, HeI, HeII, rho, uvb, threshold, J,
                       ncell, nnu);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// computeMass (equiSources.f90:4369-4393) per leaf: HI mh cs3/msun and psi rho cs3/msun, cs3 the cube of the cell's size, each
// term with the reference's operations in its order.  The sums are the code's own and deterministic: every thread adds its
// cells in grid-stride order, the workgroup folds its 256 sums as a fixed tree, and mass_total_kernel adds the workgroups'
// partial sums in a fixed order too.  No floating-point atomics (tree_sum_256: ftte_tree_sum.h).
__global__ void __launch_bounds__(256) hydrogen_mass_kernel(const int8_t *__restrict__ level, const double *__restrict__ HI,
                                                            const double *__restrict__ rho, long ncell, int n, double box,
                                                            double *__restrict__ part)
{
    __shared__ double sn[256], st[256];
    double an = 0., at = 0.;
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < ncell; c += (long)gridDim.x * 256) {
        const double cs3 = chem_cell_volume(box, level[c], n);
        an += HI[c] * FTTE_MH * cs3 / FTTE_MSUN;
        at += FTTE_PSI * rho[c] * cs3 / FTTE_MSUN;
    }
    sn[threadIdx.x] = an; st[threadIdx.x] = at;
    tree_sum_256(sn, st);
    if (threadIdx.x == 0) { part[blockIdx.x] = sn[0]; part[kMassBlocks + blockIdx.x] = st[0]; }
}

__global__ void __launch_bounds__(256) mass_total_kernel(double *part, int nblocks)
{
    __shared__ double sn[256], st[256];
    double an = 0., at = 0.;
    for (int b = threadIdx.x; b < nblocks; b += 256) { an += part[b]; at += part[kMassBlocks + b]; }
    sn[threadIdx.x] = an; st[threadIdx.x] = at;
    tree_sum_256(sn, st);
    if (threadIdx.x == 0) { part[2 * kMassBlocks] = sn[0]; part[2 * kMassBlocks + 1] = st[0]; }
}

int launch_hydrogen_mass(const int8_t *level, const double *HI, const double *rho, long ncell, int n, double box, double *part,
                         hipStream_t stream)
{
    if (ncell < 1 || n < 1 || !part) return -1;
    const long want = (ncell + 255) / 256;
    const int blocks = (int)(want < kMassBlocks ? want : kMassBlocks);
    hipLaunchKernelGGL(hydrogen_mass_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, level, HI, rho, ncell, n, box, part);
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(mass_total_kernel, dim3(1), dim3(256), 0, stream, part, blocks);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// kappa[g][c] = HI[c]*beta[0][g] + HeI[c]*beta[1][g] + HeII[c]*beta[2][g]   (equiSources.f90:4977-4980)
__global__ void __launch_bounds__(256) opacity_kernel(const double *__restrict__ HI, const double *__restrict__ HeI,
                                                      const double *__restrict__ HeII, const double *__restrict__ beta,
                                                      double *__restrict__ kappa, long ncell, int nnu)
{
    for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += (long)gridDim.x * blockDim.x) {
        const double a = HI[c], b = HeI[c], d = HeII[c];
        for (int g = 0; g < nnu; ++g) kappa[(long)g * ncell + c] = a * beta[g] + b * beta[nnu + g] + d * beta[2 * nnu + g];
    }
}

int launch_opacity(const double *HI, const double *HeI, const double *HeII, const double *beta, double *kappa, long ncell,
                   int nnu, hipStream_t stream)
{
    const int blocks = (int)((ncell + 255) / 256 < 8192 ? (ncell + 255) / 256 : 8192);
    hipLaunchKernelGGL(opacity_kernel, dim3(blocks), dim3(256), 0, stream, HI, HeI, HeII, beta, kappa, ncell, nnu);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
