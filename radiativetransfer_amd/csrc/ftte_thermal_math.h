/* ftte_thermal_math.h -- the thermal balance of one cell, written once, beside the ionisation chemistry of ftte_chem_math.h.
 *
 * What is the reference's: thermalEquilibrium (equiSources.f90:3870-4042), restated statement by statement in its order -- the
 * locals HI, HII, HeI, HeII, HeIII, de (:3907-3925), the heating of the uniform background behind the self-shielding test
 * (:3929-3940), the thirteen cooling coefficients interpolated in log T (:3946-3987), the cooling function edot (:3991-4029) and
 * hydroHeating = max(-edot, 0) (:4030-4038).  Three things of that routine are NOT restated: it writes the clipped helium back
 * into the cell (:3914-3918; no thermal call here changes a species), and its sum carries two terms multiplied by the literal
 * zeros comp_xraya and 0. (:4019, :4027; dropped).
 *
 * What is the build's own: the heating by the transfer's J and by the point sources (thermal_heating's first two parts, formed as
 * solveRateEquations forms the ionisation rates, :3520-3553, from crate24..26 of the tracer and the gamma of uvbBetaTable); the
 * logarithm ftte_log; and the temperature step thermal_advance_cell -- the reference has no time step.
 *
 * Conventions of ftte_chem_math.h: FTTE_HD functions, plain C11 plus HIP, the same source compiled by hipcc into the kernels of
 * ftte_thermal.hip and by g++ into the tests' host evaluation (tests/host/thermal_check.cpp), every operation an IEEE add,
 * multiply or divide or an explicit fused multiply-add: host and device give the same bits.
 */
#ifndef FTTE_THERMAL_MATH_H
#define FTTE_THERMAL_MATH_H

#include "ftte_chem_math.h"

#define FTTE_KB 1.3806503e-16                    /* calc_rates.f:543 */
#define FTTE_GAMMA_GAS ((double)1.6667f)         /* definitionsModule.f90:39 */
#define FTTE_T_CMB ((double)2.73f)               /* equiSources.f90:3971 */
#define THERMAL_NCOEF 13

/* The cooling coefficients, in the order of :3975-3987: ceHI, ceHeI, ceHeII, ciHI, ciHeI, ciHeIS, ciHeII, reHII, reHeII1, reHeII2,
 * reHeIII, brem, lineHI.  Coefficient r at temperature node i is c[r * coef_stride + i * node_stride]: the caller's [13][nratec]
 * has strides (nratec, 1); the node-major alternative [nratec][16] -- one node's thirteen side by side in 128 bytes -- has (1, 16).  The
 * temperature grid is the rate coefficients' (ChemTable). */
typedef struct { const double *c; long coef_stride, node_stride; } ThermalTable;

typedef struct { double HI, HII, HeI, HeII, HeIII, de; } ThermalSpecies;

/* What a call fixes for a cell: the species, the heating crate [erg/(s cm^3)] (:3940), Compton's two numbers, and for the step
 * the incoming temperature of the substep, h over the heat capacity, and the extra heating (the stored hydroHeating, or 0). */
typedef struct { ThermalSpecies s; double crate, comp1, comp2, T0, hc, extra; } ThermalCell;

/* log(x) for x > 0, finite and normal.  The scheme of ftte_log1p (ftte_math.h): x = 2^k m with m in [sqrt(1/2), sqrt(2)) from
 * frexp(x) itself, f = m - 1 (exact), log m = 2 atanh(s), s = f/(2 + f) by one IEEE division, the degree-6 polynomial lg[] in s^2,
 * k ln2 in two parts.  Same bits from g++ and on the device.  Against libm: tests/test_thermal_host.py. */
FTTE_HD double ftte_log(const ftte_consts *K, double x)
{
    int k;
    double m = FTTE_FREXP(x, &k); /* [1/2, 1) */
    if (m < K->sqrt_half) { m = m + m; k -= 1; }
    const double f = m - 1.0, kf = (double)k;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double p = K->lg[6];
    p = FTTE_FMA(p, z, K->lg[5]);
    p = FTTE_FMA(p, z, K->lg[4]);
    p = FTTE_FMA(p, z, K->lg[3]);
    p = FTTE_FMA(p, z, K->lg[2]);
    p = FTTE_FMA(p, z, K->lg[1]);
    p = FTTE_FMA(p, z, K->lg[0]);
    const double s2 = s + s;
    const double logm = FTTE_FMA(s2, z * p, s2);
    return FTTE_FMA(kf, K->ln2_hi, FTTE_FMA(kf, K->ln2_lo, logm));
}

/* the locals of :3907-3925.  HII is formed from the cell's HI as it comes, HI is clipped; where HeI + HeII exceed the helium
 * density HeIII is 0 and the local HeII stays as it was, unless nhe - HeI is negative too: then it is 0 (the reference's nested
 * branch; its writes into the cell are not made) */
FTTE_HD void thermal_species(double rho, double HI0, double HeI0, double HeII0, ThermalSpecies *s)
{
    const double nh = chem_nh(rho), nhe = chem_nhe(rho);
    s->HI = fmin(HI0, nh);
    s->HII = nh - HI0;
    s->HeI = HeI0;
    s->HeII = HeII0;
    s->HeIII = nhe - HeI0 - HeII0;
    if (s->HeIII < 0.) {
        s->HeIII = 0.;
        if (nhe - HeI0 < 0.) s->HeII = 0.;
    }
    s->de = s->HII + s->HeII + 2. * s->HeIII;
}

/* The heating per absorber [erg/s]: crate24 (HI), crate25 (HeII), crate26 (HeI).  Only the uniform branch is the reference's
 * (:3929-3938; uniform_gamma[x] = uniformQuasar*quasar%gamma + uniformStellar*stellar%gamma of HI, HeII, HeI).  The point
 * sources' part (point != 0: p24, p25, p26 = the tracer's crate24, crate25, crate26 of the cell) and the transfer's J
 * (gamma[group][gammaHI, gammaHeI, gammaHeII] of uvbBetaTable) are this build's own, the statements of chem_point_rates and
 * chem_radiation_rates with the energy integrals in place of the number integrals. */
FTTE_HD void thermal_heating(const ThermalSpecies *s, double vol, int point, double p24, double p25, double p26, const double *J, long J_stride,
                             const double *gamma, const double *uniform_gamma, double threshold, double *c24, double *c25, double *c26)
{
    double a = (point && s->HI > 0.) ? p24 / (vol * s->HI) : 0.;
    double b = (point && s->HeII > 0.) ? p25 / (vol * s->HeII) : 0.;
    double d = (point && s->HeI > 0.) ? p26 / (vol * s->HeI) : 0.;
    a = fmax(a, 0.); b = fmax(b, 0.); d = fmax(d, 0.);
    if (J) {
        const double t1 = 4. * FTTE_PI * J[0], t2 = 4. * FTTE_PI * J[J_stride], t3 = 4. * FTTE_PI * J[2 * J_stride];
        a = a + t1 * gamma[0] + t2 * gamma[3] + t3 * gamma[6];
        d = d + t2 * gamma[4] + t3 * gamma[7];
        b = b + t3 * gamma[8];
    } else if (chem_mean_free_path(s->HI, s->HeI, s->HeII) >= threshold) { /* :3929-3933 */
        a = a + 4. * FTTE_PI * uniform_gamma[0];
        b = b + 4. * FTTE_PI * uniform_gamma[1];
        d = d + 4. * FTTE_PI * uniform_gamma[2];
    }
    *c24 = a; *c25 = b; *c26 = d;
}

/* the thirteen coefficients at logtem, clamped to the table: index and statement of :3947-3987, as chem_coefficients */
FTTE_HD void thermal_coefficients(const ChemTable *T, const ThermalTable *C, double logtem, double *coef)
{
    logtem = fmax(logtem, T->logtem0);
    logtem = fmin(logtem, T->logtem9);
    int ix = (int)((logtem - T->logtem0) / T->dlogtem) + 1;
    ix = ix < 1 ? 1 : ix;
    ix = ix > T->nratec - 1 ? T->nratec - 1 : ix;
    const double t1 = T->logtem0 + (double)(ix - 1) * T->dlogtem, t2 = T->logtem0 + (double)ix * T->dlogtem, tdef = t2 - t1;
    const double *lo = C->c + (long)(ix - 1) * C->node_stride, *hi = lo + C->node_stride;
    for (int r = 0; r < THERMAL_NCOEF; ++r) {
        const double a0 = lo[r * C->coef_stride], a1 = hi[r * C->coef_stride];
        coef[r] = a0 + (logtem - t1) * (a1 - a0) / tdef;
    }
}

/* edot of :3991-4029 [erg/(s cm^3)]: the reference's terms in its order (de**2 where it has it), without the two it multiplies
 * by literal zeros.  *cooling is minus the parenthesised sum (positive where the gas cools), the return value that sum plus crate. */
FTTE_HD double thermal_edot(const double *coef, const ThermalSpecies *s, double tgas, double comp1, double comp2, double crate, double *cooling)
{
    const double HI = s->HI, HII = s->HII, HeI = s->HeI, HeII = s->HeII, HeIII = s->HeIII, de = s->de;
    const double sum = -coef[0] * HI * de      /* ceHI */
                       - coef[1] * HeI * (de * de)  /* ceHeI */
                       - coef[2] * HeII * de   /* ceHeII */
                       - coef[3] * HI * de     /* ciHI */
                       - coef[4] * HeI * de    /* ciHeI */
                       - coef[6] * HeII * de   /* ciHeII */
                       - coef[5] * HeII * (de * de) /* ciHeIS */
                       - coef[7] * HII * de    /* reHII */
                       - coef[8] * HeII * de   /* reHeII1 */
                       - coef[9] * HeII * de   /* reHeII2 */
                       - coef[10] * HeIII * de /* reHeIII */
                       - comp1 * (tgas - comp2) * de
                       - coef[11] * (HII + HeII + 4. * HeIII) * de; /* brem */
    *cooling = -sum;
    return sum + crate;
}

/* thermalEquilibrium for one cell at logtem = log(tgas).  In: the cell's state and the rates as thermal_heating takes them;
 * comp1 = compa (1+z)^4 and comp2 = 2.73 (1+z), formed once by the caller.  Out: crate (:3940), the cooling, and the return value
 * hydroHeating (:4030-4038). */
FTTE_HD double thermal_equilibrium_cell(const ChemTable *T, const ThermalTable *C, double rho, double tgas, double logtem, double HI0, double HeI0,
                                        double HeII0, double vol, int point, double p24, double p25, double p26, const double *J, long J_stride,
                                        const double *gamma, const double *uniform_gamma, double threshold, double comp1, double comp2,
                                        double *heating, double *cooling)
{
    ThermalSpecies s;
    double c24, c25, c26, coef[THERMAL_NCOEF];
    thermal_species(rho, HI0, HeI0, HeII0, &s);
    thermal_heating(&s, vol, point, p24, p25, p26, J, J_stride, gamma, uniform_gamma, threshold, &c24, &c25, &c26);
    const double crate = c24 * s.HI + c25 * s.HeII + c26 * s.HeI; /* :3940 */
    thermal_coefficients(T, C, logtem, coef);
    const double edot = thermal_edot(coef, &s, tgas, comp1, comp2, crate, cooling);
    *heating = crate;
    double hydro = -edot;
    if (hydro < 0.) hydro = 0.;
    return hydro;
}

/* ---- the temperature step: the build's own definition --------------------------------------------------------------------
 *
 * Isochoric, the species held fixed over the call (the chemistry is advanced by its own calls: the coupling is operator-split
 * and explicit, like evolve's).  Heat capacity per volume c = kB (nh + nhe + de) / (gamma - 1); net rate edot(T) above, plus the
 * cell's stored hydroHeating where the caller asks for it.  Each of `substeps` backward-Euler steps of h = dt/substeps solves
 *     F(T) = (T - T0) - hc (edot(T) + extra) = 0,      hc = h / c formed once per call,
 * one ftte_log and one set of table look-ups per evaluation.  The incoming T is clipped to [tmin, tmax].  Per substep:
 *   1. F(T0) == 0: T1 = T0 (a cell in balance with its stored hydroHeating stays exactly where it is);
 *   2. F(T0) < 0 (net heating): the bracket is [T0, tmax]; if F(tmax) <= 0, T1 = tmax;
 *   3. F(T0) > 0 (net cooling): the bracket is [tmin, T0]; if F(tmin) > 0, T1 = tmin;
 *   4. else bisection in T, mid = 0.5 (lo + hi), until mid is an end of the bracket (the stop rule of chem_advance_close),
 *      keeping F(lo) <= 0 < F(hi); T1 = lo.
 * So, unless clamped by 2 or 3 or stationary by 1, F(T1) <= 0 < F(nextafter(T1, +inf)).  The cooling curve is not monotonic: for a
 * long h, F can have several roots; the step returns the one its bracket -- on the gas's own side of T0 -- closes on.  A cell
 * fails if its incoming temperature or its heat capacity is not finite and positive, an F is not finite, or a bisection has not
 * settled in CHEM_MAX_STEPS steps. */
FTTE_HD double thermal_F(const ftte_consts *K, const ChemTable *T, const ThermalTable *C, const ThermalCell *q, double temp)
{
    double coef[THERMAL_NCOEF], cooling;
    thermal_coefficients(T, C, ftte_log(K, temp), coef);
    const double edot = thermal_edot(coef, &q->s, temp, q->comp1, q->comp2, q->crate, &cooling);
    return (temp - q->T0) - q->hc * (edot + q->extra);
}

FTTE_HD int thermal_finite(double v) { return fabs(v) <= 0x1.fffffffffffffp+1023; } /* (false for a NaN) */

/* one substep from q->T0: returns the bisection steps, *T1 the new temperature, *ok 0 on failure */
FTTE_HD unsigned thermal_advance_close(const ftte_consts *K, const ChemTable *T, const ThermalTable *C, const ThermalCell *q, double tmin,
                                       double tmax, double *T1, int *ok)
{
    const double F0 = thermal_F(K, T, C, q, q->T0);
    *T1 = q->T0;
    *ok = thermal_finite(F0);
    if (!*ok || F0 == 0.) return 0u;
    double lo = F0 < 0. ? q->T0 : tmin, hi = F0 < 0. ? tmax : q->T0;
    const double Fend = thermal_F(K, T, C, q, F0 < 0. ? tmax : tmin);
    *ok = thermal_finite(Fend);
    if (!*ok) return 0u;
    if (F0 < 0. && Fend <= 0.) { *T1 = tmax; return 0u; }
    if (F0 > 0. && Fend > 0.) { *T1 = tmin; return 0u; }
    unsigned steps = 0;
    for (;;) {
        const double mid = 0.5 * (lo + hi);
        if (mid == lo || mid == hi) break;
        if (steps >= CHEM_MAX_STEPS) { *ok = 0; break; }
        const double Fm = thermal_F(K, T, C, q, mid);
        if (!thermal_finite(Fm)) { *ok = 0; break; }
        if (Fm <= 0.) lo = mid;
        else hi = mid;
        ++steps;
    }
    *T1 = lo;
    return steps;
}

/* the heat capacity per volume at constant volume, kB (nh + nhe + de) / (gamma - 1) [erg/(K cm^3)] */
FTTE_HD double thermal_heat_capacity(double rho, double de) { return FTTE_KB * (chem_nh(rho) + chem_nhe(rho) + de) / (FTTE_GAMMA_GAS - 1.); }

/* what a call fixes for a cell before its first substep (all of ThermalCell but T0); returns whether the cell can be stepped */
FTTE_HD int thermal_advance_setup(ThermalCell *q, double rho, double tgas, double HI0, double HeI0, double HeII0, double vol, int point, double p24,
                                  double p25, double p26, const double *J, long J_stride, const double *gamma, const double *uniform_gamma,
                                  double threshold, double comp1, double comp2, double extra, double dt, int substeps)
{
    double c24, c25, c26;
    thermal_species(rho, HI0, HeI0, HeII0, &q->s);
    thermal_heating(&q->s, vol, point, p24, p25, p26, J, J_stride, gamma, uniform_gamma, threshold, &c24, &c25, &c26);
    q->crate = c24 * q->s.HI + c25 * q->s.HeII + c26 * q->s.HeI;
    q->comp1 = comp1; q->comp2 = comp2; q->extra = extra;
    const double heat_capacity = thermal_heat_capacity(rho, q->s.de);
    q->hc = (dt / (double)substeps) / heat_capacity;
    q->T0 = tgas;
    return thermal_finite(tgas) && heat_capacity > 0. && thermal_finite(heat_capacity) && thermal_finite(q->crate) && thermal_finite(extra);
}

/* The temperature of one cell advanced over dt in `substeps` equal steps.  In: as thermal_equilibrium_cell, the consts of
 * ftte_math.h, dt [s], the clip [tmin, tmax], and `extra`: the cell's stored hydroHeating, or 0.  The rates per absorber are
 * formed once per call.  Out: whether the cell got through, the new temperature and its ftte_log, the bisection steps of all
 * substeps, |T1 - T0| / T0 with T0 the clipped incoming temperature. */
FTTE_HD int thermal_advance_cell(const ftte_consts *K, const ChemTable *T, const ThermalTable *C, double rho, double tgas, double HI0, double HeI0,
                                 double HeII0, double vol, int point, double p24, double p25, double p26, const double *J, long J_stride,
                                 const double *gamma, const double *uniform_gamma, double threshold, double comp1, double comp2, double extra,
                                 double dt, int substeps, double tmin, double tmax, double *T_out, double *logtem_out,
                                 unsigned long long *steps_out, double *change_out)
{
    ThermalCell q;
    int ok = thermal_advance_setup(&q, rho, tgas, HI0, HeI0, HeII0, vol, point, p24, p25, p26, J, J_stride, gamma, uniform_gamma, threshold, comp1,
                                   comp2, extra, dt, substeps);
    const double Tin = fmin(fmax(tgas, tmin), tmax);
    double Tnow = Tin;
    unsigned long long steps = 0ull;
    for (int sub = 0; sub < substeps && ok; ++sub) {
        q.T0 = Tnow;
        steps += (unsigned long long)thermal_advance_close(K, T, C, &q, tmin, tmax, &Tnow, &ok);
    }
    *T_out = Tnow;
    *logtem_out = ok ? ftte_log(K, Tnow) : 0.;
    *steps_out = steps;
    *change_out = fabs(Tnow - Tin) / Tin;
    return ok;
}

#endif /* FTTE_THERMAL_MATH_H */
