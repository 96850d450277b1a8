/* ftte_chem_math.h -- the ionisation chemistry of one cell, written once.
 *
 * solveRateEquations (equiSources.f90:3459-3677) and initialIonizationEquilibrium (:3679-3868) are one algorithm: densities
 * from rho, the six rate coefficients interpolated in log T, a bisection on the electron density whose residual is the
 * helium balance, and the closing statements for HII, HI, HeII with the reference's test of the fractions.  Every
 * statement keeps the reference's operation order (each operation an IEEE add, multiply or divide; the logarithm of the
 * temperature comes from the host) and its line reference.  What differs between the two routines is four parameters of
 * chem_bisect, literals at its two call sites.  Below them stands the build's own time-dependent step over dt
 * (chem_advance_cell), on the same densities, coefficients and rates.
 *
 * Conventions of ftte_math.h: FTTE_HD functions, plain C11 plus HIP, no templates, lambdas or references -- the same
 * source is compiled by hipcc into the kernels of ftte_chem.hip and by gcc into the tests' host library (fo_device_solve_rate_equations,
 * fo_device_initial_equilibrium, fo_device_chem_tame), where CPU tests pin it.  On the host FTTE_DIV is `/` and FTTE_ANY is
 * per element: control flow, operation order, constants and branch logic are what the host evaluation checks; the trimmed
 * division and the wavefront vote are the device's alone.  A compile-time choice is an int argument that is a literal at
 * every call site, under forced inlining.  Arguments are plain data and pointers to plain arrays (the coefficient tables,
 * J, ksi, the background): no launch record, nothing of the context.
 */
#ifndef FTTE_CHEM_MATH_H
#define FTTE_CHEM_MATH_H

#include <stddef.h>

#include "ftte_math.h"

/* The reference's constants: default-real literals assigned to double parameters, so each double holds the float32-rounded
 * value.  Everything in csrc/ that needs one takes it from here. */
#define FTTE_PI ((double)3.141592654f)      /* definitionsModule.f90:8 */
#define FTTE_MP ((double)1.6726231e-24f)    /* :25 */
#define FTTE_MN ((double)1.67492728e-24f)   /* :26 */
#define FTTE_MH FTTE_MP                     /* :27 */
#define FTTE_MHE (2. * (FTTE_MP + FTTE_MN)) /* :28 */
#define FTTE_MSUN ((double)1.98892e33f)     /* :29 */
#define FTTE_PSI ((double)0.76f)            /* :261, the hydrogen mass fraction */
/* the Lyman-limit cross sections of HI, HeI, HeII, literals where the reference uses them (equiSources.f90:3180-3182, :3556) */
#define FTTE_SIGMA_HI ((double)6.3e-18f)
#define FTTE_SIGMA_HEI ((double)7.42e-18f)
#define FTTE_SIGMA_HEII ((double)1.58e-18f)

#define CHEM_MAX_STEPS 4096u /* the reference loops forever on a NaN HeI: capped, and a failure */

typedef struct { double k1, k2, k3, k4, k5, k6, nh, nhe, kr24, kr25, kr26; } ChemEq;
/* the rate-coefficient tables k1a..k6a: k[6][nratec] over logtem0 + i dlogtem */
typedef struct { const double *k; int nratec; double logtem0, logtem9, dlogtem; } ChemTable;

/* number densities of hydrogen and helium nuclei, :3497-3498 */
FTTE_HD double chem_nh(double rho) { return FTTE_PSI * rho / FTTE_MH; }
FTTE_HD double chem_nhe(double rho) { return (1. - FTTE_PSI) * rho / FTTE_MHE; }

/* meanFreePathLymanLimit, :3556 (and :3734, transportRoutinesModule.f90:1081) */
FTTE_HD double chem_mean_free_path(double HI, double HeI, double HeII) { return 1. / (HI * FTTE_SIGMA_HI + HeI * FTTE_SIGMA_HEI + HeII * FTTE_SIGMA_HEII); }

/* a leaf's volume: the cube of box / (float(2**level) float(n)), :3520 (and computeMass, :4380) */
FTTE_HD double chem_cell_volume(double box, int level, int n)
{
    const double size = box / (double)((float)(1 << level) * (float)n);
    return size * size * size;
}

/* rate coefficients at this temperature, :3568-3587 (the same statements at :3747-3766) */
FTTE_HD void chem_coefficients(const ChemTable *T, double logtem, ChemEq *q)
{
    logtem = fmax(logtem, T->logtem0);
    logtem = fmin(logtem, T->logtem9);
    int ix = (int)((logtem - T->logtem0) / T->dlogtem) + 1;
    ix = ix < 1 ? 1 : ix;
    ix = ix > T->nratec - 1 ? T->nratec - 1 : ix;
    const double t1 = T->logtem0 + (double)(ix - 1) * T->dlogtem, t2 = T->logtem0 + (double)ix * T->dlogtem, tdef = t2 - t1;
    double kk[6];
    for (int r = 0; r < 6; ++r) {
        const double *ka = T->k + (size_t)r * T->nratec;
        kk[r] = ka[ix - 1] + (logtem - t1) * (ka[ix] - ka[ix - 1]) / tdef;
    }
    q->k1 = kk[0]; q->k2 = kk[1]; q->k3 = kk[2]; q->k4 = kk[3]; q->k5 = kk[4]; q->k6 = kk[5];
}

/* The residual of the helium balance at electron density de, and HeI there: :3592-3596 (repeated at :3600-3604 and
 * :3618-3622).  ieee: every division the compiler's own; else FTTE_DIV.  *HX is the last numerator, HeI X. */
FTTE_HD double chem_div(double a, double b, int ieee) { return ieee ? a / b : FTTE_DIV(a, b); }

FTTE_HD double chem_residual_as(const ChemEq *q, double de, int ieee, double *HeI, double *HX)
{
    const double X = q->k3 * de + q->kr26, Y = q->k4 * de;
    const double XY = chem_div(X, Y, ieee);
    const double HII = chem_div(q->nh, 1. + chem_div(q->k2 * de, q->k1 * de + q->kr24, ieee), ieee);
    *HeI = chem_div(de - HII - 2. * q->nhe, XY - 2. - chem_div(2. * X, Y, ieee), ieee);
    *HX = *HeI * X;
    const double HeII = chem_div(*HX, Y, ieee);
    return q->k3 * *HeI * de + q->k6 * (q->nhe - *HeI - HeII) * de + q->kr26 * *HeI - HeII * (q->k4 * de + q->k5 * de + q->kr25);
}

/* The residual's six divisions through FTTE_DIV, the trimmed sequence of ftte_math.h (a quarter fewer instructions, some forty
 * evaluations per cell), where that gives IEEE's quotient; the plain division where it might not.  `tame` (per cell,
 * chem_tame): every operand that depends on the rate coefficients lies in [2^-250, 2^250] for every de of the bracket -- then
 * every divisor, and every quotient but the last, is far from both ends of the range.  Left to check per evaluation: the last
 * numerator, HeI X (too small: HeII near the underflow), and NaN from an overflowing quotient.  Any lane outside takes the whole
 * wavefront through IEEE division, which gives the same bits in the lanes that did not need it. */
FTTE_HD double chem_residual(const ChemEq *q, double de, double *HeI, int tame)
{
    double HX;
    if (!FTTE_ANY(!tame)) {
        double h;
        const double r = chem_residual_as(q, de, 0, &h, &HX);
        if (!FTTE_ANY(!(r == r) || (HX != 0. && fabs(HX) < 0x1p-700))) { *HeI = h; return r; }
    }
    return chem_residual_as(q, de, 1, HeI, &HX);
}

/* Whether the divisors and numerators of chem_residual that depend on the rate coefficients stay in [2^-250, 2^250] over the
 * bracket [de1, de2] (each is a non-decreasing function of de when the coefficients are not negative, so its ends bound it), X
 * either there or 0 throughout, and nh, nhe there too.  False for a table whose coefficients vanish or come close to it where
 * nothing else ionises the cell: k1 de + kr24 or k4 de is then subnormal or 0 at de = 1e-30, where the trimmed division
 * returns NaN and IEEE's carries on with inf and 0. */
FTTE_HD int chem_in_range(double v) { return v >= 0x1p-250 && v <= 0x1p250; }

FTTE_HD int chem_tame(const ChemEq *q, double de1, double de2)
{
    const double X1 = q->k3 * de1 + q->kr26, X2 = q->k3 * de2 + q->kr26;
    return q->k1 >= 0. && q->k2 >= 0. && q->k3 >= 0. && q->k4 >= 0. && chem_in_range(q->nh) && chem_in_range(q->nhe) &&
           chem_in_range(q->k1 * de1 + q->kr24) && chem_in_range(q->k1 * de2 + q->kr24) && chem_in_range(q->k2 * de1) &&
           chem_in_range(q->k2 * de2) && chem_in_range(q->k4 * de1) && chem_in_range(q->k4 * de2) &&
           ((X1 == 0. && X2 == 0.) || (chem_in_range(X1) && chem_in_range(X2)));
}

/* The bisection on the electron density over [de_floor, nh + 2 nhe], :3589-3633 and :3771-3807, `opposite` at :5044-5058.
 * Returns the steps taken; *de, *HeI the last midpoint (the upper end if no step was taken) and HeI there, *HeIprev HeI
 * one step before (-1 if no step was taken); *tame what chem_tame said of the bracket (0 if not asked).  What the two
 * routines do differently, each named after what the reference does:
 *   de_floor        the lower end of the bracket: a default-real 1.e-30 (:3589) or 1.e-20 (:3771)
 *   res1_follows    the residual at the lower end follows the bracket when that end moves (:3624-3630), or is taken once
 *                   at de_floor and never updated (:3798-3805)
 *   stop_relative   run while HeI moves by more than 1e-10 of the helium density (:3610), or until it stops changing
 *                   at all (:3789)
 *   trimmed         the residual's divisions through chem_residual (the tame test of the cell decides), or IEEE throughout */
FTTE_HD unsigned chem_bisect(const ChemEq *q, double de_floor, int res1_follows, int stop_relative, int trimmed, double *de_out,
                             double *HeI_out, double *HeIprev_out, int *tame_out)
{
#define CHEM_RESIDUAL(de) (trimmed ? chem_residual(q, (de), &HeI, tame) : chem_residual_as(q, (de), 1, &HeI, &HX))
    double de1 = de_floor, de2 = q->nh + 2. * q->nhe, de = de2, HeI, HX, HeIprev = -1.;
    const int tame = trimmed ? chem_tame(q, de1, de2) : 0;
    double res1 = CHEM_RESIDUAL(de1);
    (void)CHEM_RESIDUAL(de2);
    unsigned steps = 0;
    while ((stop_relative ? fabs(HeI - HeIprev) / q->nhe > 1.e-10 : HeI != HeIprev) && steps < CHEM_MAX_STEPS) {
        HeIprev = HeI;
        de = 0.5 * (de1 + de2);
        const double res = CHEM_RESIDUAL(de);
        const int opposite = (res > 0. && res1 < 0.) || (res < 0. && res1 > 0.); /* :5044-5058 */
        if (opposite) de2 = de;
        else { de1 = de; res1 = res1_follows ? res : res1; }
        ++steps;
    }
    *de_out = de; *HeI_out = HeI; *HeIprev_out = HeIprev; *tame_out = tame;
    return steps;
#undef CHEM_RESIDUAL
}

/* The closing statements at the electron density the bisection ended on, :3634-3636 and :3820-3823 (IEEE divisions), and the
 * test behind which the reference prints the species and stops, :3637-3654 and :3832-3843.  Returns whether the fractions of HI
 * and HeI lie in [0, 1].  (The two routines spell these statements in different orders; none depends on another but HI on
 * HII.  Kept: solveRateEquations' order.) */
FTTE_HD int chem_close(const ChemEq *q, double de, double HeI, double *HI_out, double *HeII_out)
{
    const double X = q->k3 * de + q->kr26, Y = q->k4 * de;
    *HeII_out = HeI * X / Y;
    const double HII = q->nh / (1. + q->k2 * de / (q->k1 * de + q->kr24));
    const double HI = *HI_out = q->k2 * HII * de / (q->k1 * de + q->kr24);
    return (HI / q->nh >= 0. && HI / q->nh <= 1.) && (HeI / q->nhe >= 0. && HeI / q->nhe <= 1.);
}

/* The photo-ionisation rates per absorber, in two parts that each take the absorbers HI, HeI, HeII as their caller sees them.
 * First the point sources' rates per cell over the absorbers in the cell, :3520-3542; arguments as chem_solve_cell's. */
FTTE_HD void chem_point_rates(ChemEq *q, double HI, double HeI, double HeII, double vol, int point, double p24, double p25, double p26)
{
    q->kr24 = (point && HI > 0.) ? p24 / (vol * HI) : 0.;
    q->kr25 = (point && HeII > 0.) ? p25 / (vol * HeII) : 0.;
    q->kr26 = (point && HeI > 0.) ? p26 / (vol * HeI) : 0.;
    q->kr24 = fmax(q->kr24, 0.); q->kr25 = fmax(q->kr25, 0.); q->kr26 = fmax(q->kr26, 0.);
}

/* Then, added to them, either the transfer's J, :3545-3553, or the uniform background where the Lyman-limit mean free path
 * of HI, HeI, HeII is at least the self-shielding threshold, :3554-3562 */
FTTE_HD void chem_radiation_rates(ChemEq *q, double HI, double HeI, double HeII, const double *J, long J_stride, const double *ksi,
                                  const double *uniform, double threshold)
{
    if (J) { /* :3545-3553 */
        const double t1 = 4. * FTTE_PI * J[0], t2 = 4. * FTTE_PI * J[J_stride], t3 = 4. * FTTE_PI * J[2 * J_stride];
        q->kr24 = q->kr24 + t1 * ksi[0] + t2 * ksi[3] + t3 * ksi[6];
        q->kr25 = q->kr25 + t3 * ksi[7];
        q->kr26 = q->kr26 + t2 * ksi[5] + t3 * ksi[8];
    } else if (chem_mean_free_path(HI, HeI, HeII) >= threshold) { /* :3554-3562 */
        q->kr24 = q->kr24 + 4. * FTTE_PI * uniform[0];
        q->kr25 = q->kr25 + 4. * FTTE_PI * uniform[1];
        q->kr26 = q->kr26 + 4. * FTTE_PI * uniform[2];
    }
}

/* solveRateEquations for one cell.  In: the cell's state and its rates -- the point sources' rates per cell (point != 0: p24,
 * p25, p26 = krate24, krate25, krate26) plus either the transfer's J (J != NULL: the cell's three groups at J[0], J[J_stride],
 * J[2 J_stride]; ksi[group][ksi24, ksi25, ksi26]) or the uniform background behind the self-shielding test.  Out: whether the
 * reference carries on (else it prints the species and stops, :3637-3654, and what follows is of no use but *steps), the new
 * species, the bisection steps, the reference's (unused) convergence measure, :3671-3674, and chem_tame of the cell's bracket.
 * (J is read here, behind the branch that needs it, and not handed in as three values: on the device those would have to be
 * loaded ahead of the branch and stay live across the set-up, two registers over what keeps five wavefronts resident.  And
 * every output is written either way: written only behind the test they cost the device kernel eighteen registers.) */
FTTE_HD int chem_solve_cell(const ChemTable *T, double rho, double logtem, double HI0, double HeI0, double HeII0, double vol, int point,
                            double p24, double p25, double p26, const double *J, long J_stride, const double *ksi, const double *uniform,
                            double threshold, double *HI_out, double *HeI_out, double *HeII_out, unsigned *steps_out, double *change_out,
                            int *tame_out)
{
    ChemEq q;
    q.nh = chem_nh(rho); q.nhe = chem_nhe(rho);
    double HI = fmin(HI0, q.nh), HeI = HeI0, HeII = HeII0, de, HeIprev;
    if (q.nhe - HeI0 - HeII0 < 0. && HeII < 0.) HeII = 0.; /* :3504-3513: only this survives of the branch */
    chem_point_rates(&q, HI, HeI, HeII, vol, point, p24, p25, p26); /* :3520-3542 */
    chem_radiation_rates(&q, HI, HeI, HeII, J, J_stride, ksi, uniform, threshold);
    chem_coefficients(T, logtem, &q);
    const unsigned steps = *steps_out = chem_bisect(&q, (double)1.e-30f, 1, 1, 1, &de, &HeI, &HeIprev, tame_out);
    const int ok = chem_close(&q, de, HeI, &HI, &HeII) && steps < CHEM_MAX_STEPS;
    const double c1 = fabs(HI - HI0) * FTTE_MH / (FTTE_PSI * rho), c2 = fabs(HeI - HeI0) * FTTE_MHE / ((1. - FTTE_PSI) * rho),
                 c3 = fabs(HeII - HeII0) * FTTE_MHE / ((1. - FTTE_PSI) * rho);
    *change_out = fmax(c1, fmax(c2, c3));
    *HI_out = HI; *HeI_out = HeI; *HeII_out = HeII;
    return ok;
}

/* initialIonizationEquilibrium for one cell, `passes` times (the reference: twice, :1016), the next pass starting from the last
 * one's HI, HeI, HeII -- in registers, since the routine reads nothing outside its own cell.  The residual is
 * solveRateEquations'; the rates are the uniform background's behind the self-shielding test alone (:3731-3743).  Out: whether
 * every pass converged with fractions in [0, 1] (a pass that does not ends the cell: the reference stops, :3809-3818,
 * :3832-3843), the species after the last pass run (of use only if all converged), the steps of all passes run. */
FTTE_HD int chem_initial_cell(const ChemTable *T, double rho, double logtem, double HI0, double HeI0, double HeII0, const double *uniform,
                              double threshold, int passes, double *HI_out, double *HeI_out, double *HeII_out, unsigned long long *steps_out)
{
    ChemEq q;
    q.nh = chem_nh(rho); q.nhe = chem_nhe(rho);
    chem_coefficients(T, logtem, &q); /* :3747-3766: the same in every pass */
    double cHI = HI0, cHeI = HeI0, cHeII = HeII0; /* currentCell%HI, %HeI, %HeII on entry to the pass */
    int ok = 1, tame;
    *steps_out = 0ull;
    for (int pass = 0; pass < passes && ok; ++pass) {
        /* :3710-3726.  HII is dead (de is reassigned before use).  Of the HeIII clip only this survives: currentCell%HeI and
         * %HeII are overwritten at the end, so the local HeII = 0 of the inner branch is its one effect, and that branch tests
         * the REASSIGNED currentCell%HeII = nhe - HeI0 (unlike :3504-3513) */
        const double HI = fmin(cHI, q.nh);
        const double HeII = (q.nhe - cHeI - cHeII < 0. && q.nhe - cHeI < 0.) ? 0. : cHeII;
        /* uniform background only, behind the self-shielding test (:3731-3743); HI clipped, HeI unclipped */
        const int lit = chem_mean_free_path(HI, cHeI, HeII) >= threshold;
        q.kr24 = lit ? 4. * FTTE_PI * uniform[0] : 0.;
        q.kr25 = lit ? 4. * FTTE_PI * uniform[1] : 0.;
        q.kr26 = lit ? 4. * FTTE_PI * uniform[2] : 0.;
        double de, HeI, HeIprev;
        const unsigned steps = chem_bisect(&q, (double)1.e-20f, 0, 0, 0, &de, &HeI, &HeIprev, &tame);
        *steps_out += (unsigned long long)steps;
        /* :3808-3818: HIprev, HeIIprev are HI, HeII (unchanged inside the loop) once the loop has run, -1 if it has not */
        const double HIprev = steps ? HI : -1., HeIIprev = steps ? HeII : -1.;
        const int converged = HeI == HeIprev && !(HIprev != HI) && !(HeIIprev != HeII);
        ok = chem_close(&q, de, HeI, &cHI, &cHeII) && converged;
        cHeI = HeI;
    }
    *HI_out = cHI; *HeI_out = cHeI; *HeII_out = cHeII;
    return ok;
}

/* ---- time-dependent ionisation: one implicit step over dt ---------------------------------------------------------------
 *
 * The rate equations whose balance is the residual above (:3592-3602), at fixed temperature and fixed rates per absorber,
 *   dHI/dt   = k2 de HII - (k1 de + kr24) HI
 *   dHeI/dt  = Y HeII - X HeI                                   X = k3 de + kr26, Y = k4 de
 *   dHeII/dt = X HeI - (Y + W) HeII + Z HeIII                   W = k5 de + kr25, Z = k6 de
 * with HII = nh - HI and HeIII = nhe - HeI - HeII put in, stepped by backward Euler at a trial electron density de, and de
 * closed by bisection on charge neutrality.  Nothing here is the reference's (it has no time step); the stationary state of
 * the step is its equilibrium. */

/* by how much a species fraction may leave [0, 1] and count as rounding */
#define CHEM_ADVANCE_SLACK 0x1p-48

/* One backward-Euler step of length h at electron density de.  Hydrogen is linear in HI.  Helium is the 2x2 system
 *   (1 + hX) HeI' - hY HeII' = HeI,   -h(X - Z) HeI' + (1 + h(Y + W + Z)) HeII' = HeII + hZ nhe
 * by Cramer's rule, the determinant 1 + h(X + Y + W + Z) + h^2 (XW + XZ + YZ) and both numerators multiplied out into sums of
 * non-negative terms (HeI <= nhe on entry): no difference of products, nothing cancels, and HeI' + HeII' <= nhe to rounding.
 * The powers of h stay inside the products hX, hY, hW, hZ, so that a step of 1e40 s overflows nothing. */
FTTE_HD void chem_advance_step(const ChemEq *q, double h, double de, double HI, double HeI, double HeII, double *HI1, double *HeI1,
                               double *HeII1)
{
    const double a = q->k1 * de + q->kr24, b = q->k2 * de;
    *HI1 = (HI + h * b * q->nh) / (1. + h * (a + b));
    const double hX = h * (q->k3 * de + q->kr26), hY = h * (q->k4 * de), hW = h * (q->k5 * de + q->kr25), hZ = h * (q->k6 * de);
    const double det = 1. + (hX + hY + hW + hZ) + (hX * hW + hX * hZ + hY * hZ);
    *HeI1 = (HeI * (1. + (hY + hW + hZ)) + hY * (HeII + hZ * q->nhe)) / det;
    *HeII1 = (HeII + hZ * (q->nhe - HeI) + hX * (HeII + HeI) + hX * hZ * q->nhe) / det;
}

/* The step closed: bisection on de over [1e-30, nh + 2 nhe] of de - (HII' + HeII' + 2 HeIII'), until the midpoint is an end
 * of the bracket (or CHEM_MAX_STEPS moves of the bracket).  Returns the moves; the species are those at the last midpoint. */
FTTE_HD unsigned chem_advance_close(const ChemEq *q, double h, double *HI, double *HeI, double *HeII)
{
    double de1 = (double)1.e-30f, de2 = q->nh + 2. * q->nhe, HI1, HeI1, HeII1;
    unsigned steps = 0;
    for (;;) {
        const double de = 0.5 * (de1 + de2);
        chem_advance_step(q, h, de, *HI, *HeI, *HeII, &HI1, &HeI1, &HeII1);
        if (de == de1 || de == de2 || steps >= CHEM_MAX_STEPS) break;
        const double res = de - ((q->nh - HI1) + HeII1 + 2. * (q->nhe - HeI1 - HeII1));
        if (res > 0.) de2 = de;
        else de1 = de;
        ++steps;
    }
    *HI = HI1; *HeI = HeI1; *HeII = HeII1;
    return steps;
}

/* a state within the elements' budgets: HI <= nh, HeI <= nhe, HeII <= nhe - HeI, none negative */
FTTE_HD void chem_advance_clip(const ChemEq *q, double *HI, double *HeI, double *HeII)
{
    *HI = fmax(fmin(*HI, q->nh), 0.);
    *HeI = fmax(fmin(*HeI, q->nhe), 0.);
    *HeII = fmax(fmin(*HeII, q->nhe - *HeI), 0.);
}

/* What a call fixes for a cell before its first step: the densities, the incoming state clipped to the elements' budgets
 * (*HI, *HeI, *HeII on return), the rates per absorber and the coefficients.  The rates are formed by the statements that
 * form chem_solve_cell's: the point sources' over the absorbers of the clipped state (none where there are none); the
 * self-shielding test on the incoming state as the equilibrium routines take it -- HI no more than nh, HeI and HeII as they
 * come -- so that a cell over its helium budget is shielded or lit here as it is there. */
FTTE_HD void chem_advance_setup(const ChemTable *T, ChemEq *q, double rho, double logtem, double *HI, double *HeI, double *HeII, double vol,
                                int point, double p24, double p25, double p26, const double *J, long J_stride, const double *ksi,
                                const double *uniform, double threshold)
{
    q->nh = chem_nh(rho); q->nhe = chem_nhe(rho);
    const double HI0 = fmin(*HI, q->nh), HeI0 = *HeI, HeII0 = *HeII;
    chem_advance_clip(q, HI, HeI, HeII);
    chem_point_rates(q, *HI, *HeI, *HeII, vol, point, p24, p25, p26);
    chem_radiation_rates(q, HI0, HeI0, HeII0, J, J_stride, ksi, uniform, threshold);
    chem_coefficients(T, logtem, q);
}

/* HI, HeI, HeII of one cell advanced over dt in `substeps` equal steps.  In: as chem_solve_cell, and dt [s].  The rates per
 * absorber (chem_advance_setup) stay fixed for the whole call, substeps included.  Out: whether the cell got through (else: an
 * output that is not finite, HI'/nh or (HeI' + HeII')/nhe outside [0, 1] by more than rounding, or a bisection that hit the
 * cap), the new species, the bisection steps of all substeps, and chem_solve_cell's measure of the change. */
FTTE_HD int chem_advance_cell(const ChemTable *T, double rho, double logtem, double HI0, double HeI0, double HeII0, double vol, int point,
                              double p24, double p25, double p26, const double *J, long J_stride, const double *ksi, const double *uniform,
                              double threshold, double dt, int substeps, double *HI_out, double *HeI_out, double *HeII_out,
                              unsigned long long *steps_out, double *change_out)
{
    ChemEq q;
    double HI = HI0, HeI = HeI0, HeII = HeII0;
    chem_advance_setup(T, &q, rho, logtem, &HI, &HeI, &HeII, vol, point, p24, p25, p26, J, J_stride, ksi, uniform, threshold);
    const double h = dt / (double)substeps;
    unsigned long long steps = 0ull;
    int ok = 1;
    for (int s = 0; s < substeps && ok; ++s) {
        if (s) chem_advance_clip(&q, &HI, &HeI, &HeII); /* a substep takes its state as a call does: the sums' rounding does not add up */
        const unsigned n = chem_advance_close(&q, h, &HI, &HeI, &HeII);
        steps += (unsigned long long)n;
        ok = n < CHEM_MAX_STEPS;
    }
    const double fH = HI / q.nh, fHe = (HeI + HeII) / q.nhe;
    /* (a NaN fails every comparison; an infinity the range) */
    ok = ok && fH >= -CHEM_ADVANCE_SLACK && fH <= 1. + CHEM_ADVANCE_SLACK && fHe >= -CHEM_ADVANCE_SLACK && fHe <= 1. + CHEM_ADVANCE_SLACK &&
         HeI >= -CHEM_ADVANCE_SLACK * q.nhe && HeII >= -CHEM_ADVANCE_SLACK * q.nhe;
    const double c1 = fabs(HI - HI0) * FTTE_MH / (FTTE_PSI * rho), c2 = fabs(HeI - HeI0) * FTTE_MHE / ((1. - FTTE_PSI) * rho),
                 c3 = fabs(HeII - HeII0) * FTTE_MHE / ((1. - FTTE_PSI) * rho);
    *change_out = fmax(c1, fmax(c2, c3));
    *HI_out = HI; *HeI_out = HeI; *HeII_out = HeII;
    *steps_out = steps;
    return ok;
}

#endif /* FTTE_CHEM_MATH_H */
