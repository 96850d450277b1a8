/* ftte_recombination_math.h -- the diffuse recombination radiation of one leaf, written once.
 *
 * Recombinations to the ground states of HI, HeI and HeII emit photons that can ionise again.  This header turns a leaf's gas
 * state into the source function the diffuse sweep carries: per frequency group j, the photons emitted per volume and second
 * over what the leaf's absorbers capture per unit 4 pi J,
 *   S[j] = E[j] / (4 pi D[j]),
 *   E[j] = share[0][j] R[0] + share[1][j] R[1] + share[2][j] R[2],     R = g(T) de (HII, HeII, HeIII),
 *   D[0] = HI ksi24[0],  D[1] = HI ksi24[1] + HeI ksi26[1],  D[2] = HI ksi24[2] + HeII ksi25[2] + HeI ksi26[2],
 * the ksi entries being the ones chem_radiation_rates reads and no others.  The chemistry consumes J only through 4 pi J ksi, so a
 * leaf bathed in J = S re-absorbs exactly E[j] photons per volume and second in group j, whatever the mix of its absorbers: photon
 * number is conserved against the chemistry as it is evaluated.  (Not so the energy: per unit intensity it follows ksi / beta, which
 * differs a little between the absorbers of one group, as in the reference's own group model.)  Nothing here is the reference's:
 * its emissivity is hard-wired to zero (transportRoutinesModule.f90:673-675).
 *
 * Conventions of ftte_math.h and ftte_chem_math.h: FTTE_HD functions, plain C11 plus HIP, every operation an IEEE add, multiply or
 * divide, no fused multiply-add.  The same source is compiled by hipcc into recombination_source_kernel (ftte_recombination.hip) and by
 * g++ into the tests' host library (tests/host/recombination_check.cpp), where CPU tests pin it and which the GPU is compared with
 * bit for bit.  Arguments are plain data and pointers to plain arrays: no launch record, nothing of the context.
 */
#ifndef FTTE_RECOMBINATION_MATH_H
#define FTTE_RECOMBINATION_MATH_H

#include "ftte_chem_math.h"

FTTE_HD int recomb_finite(double v) { return fabs(v) <= 0x1.fffffffffffffp+1023; } /* (false for a NaN) */

/* The three ground-state recombination coefficients at this temperature from T->k = g[3][nratec]: the statements of
 * chem_coefficients -- the same clamping, the same ix, the same expression -- over three rows instead of six */
FTTE_HD void recomb_coefficients(const ChemTable *T, double logtem, double *g)
{
    logtem = fmax(logtem, T->logtem0);
    logtem = fmin(logtem, T->logtem9);
    int ix = (int)((logtem - T->logtem0) / T->dlogtem) + 1;
    ix = ix < 1 ? 1 : ix;
    ix = ix > T->nratec - 1 ? T->nratec - 1 : ix;
    const double t1 = T->logtem0 + (double)(ix - 1) * T->dlogtem, t2 = T->logtem0 + (double)ix * T->dlogtem, tdef = t2 - t1;
    for (int r = 0; r < 3; ++r) {
        const double *ga = T->k + (size_t)r * T->nratec;
        g[r] = ga[ix - 1] + (logtem - t1) * (ga[ix] - ga[ix - 1]) / tdef;
    }
}

/* The source function of one leaf.  In: the leaf's density, the stored logarithm of its temperature and its species as they come
 * (clipped here to the elements' budgets as chem_advance_cell clips its incoming state); T->k = g[3][nratec], the coefficients of
 * recombination to the ground states of HI, HeI, HeII; ksi[group][ksi24, ksi25, ksi26]; share[ion][group], the part of an ion's
 * ground-state photons that group j receives.  Out: S[3]; E[3], the photons emitted per volume and second (what S was made
 * from: for the tests, the kernel drops it); *lost, the groups with E > 0 that nothing in the leaf absorbs (D == 0: the sweep's
 * S (1 - exp(-tau)) cannot emit them, and S is 0 there).  Returns whether the leaf got through: a density that is positive and
 * finite, a finite electron density, a finite S. */
FTTE_HD int recomb_source_cell(const ChemTable *T, double rho, double logtem, double HI, double HeI, double HeII, const double *ksi,
                               const double *share, double *S, double *E, int *lost)
{
    ChemEq q;
    q.nh = chem_nh(rho); q.nhe = chem_nhe(rho);
    chem_advance_clip(&q, &HI, &HeI, &HeII);
    const double HII = q.nh - HI, HeIII = q.nhe - HeI - HeII, de = HII + HeII + 2. * HeIII;
    double g[3];
    recomb_coefficients(T, logtem, g);
    const double R0 = g[0] * de * HII, R1 = g[1] * de * HeII, R2 = g[2] * de * HeIII;
    const double D[3] = {HI * ksi[0], HI * ksi[3] + HeI * ksi[5], HI * ksi[6] + HeII * ksi[7] + HeI * ksi[8]};
    int ok = rho > 0. && recomb_finite(rho) && recomb_finite(de), n = 0;
    for (int j = 0; j < 3; ++j) {
        E[j] = share[j] * R0 + share[3 + j] * R1 + share[6 + j] * R2;
        S[j] = D[j] == 0. ? 0. : E[j] / (4. * FTTE_PI * D[j]);
        n += E[j] > 0. && D[j] == 0.;
        ok = ok && recomb_finite(S[j]);
    }
    *lost = n;
    return ok;
}

#endif /* FTTE_RECOMBINATION_MATH_H */
