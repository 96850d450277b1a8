/* ftte_thermochem_math.h -- species and temperature of one cell advanced together over dt, written once.
 *
 * Nothing here is the reference's: it has no time step, and its commented-out coupled solver is not restated.  The statement is
 * the build's own and is made of the two it already has -- the implicit chemistry step of ftte_chem_math.h (chem_advance_close)
 * and the implicit temperature step of ftte_thermal_math.h (thermal_advance_close) -- taken in turn over subcycles whose length
 * the cell's own time scales decide:
 *
 *   once per call   the densities; the incoming state clipped to the elements' budgets; the ionisation rates per absorber
 *                   kr24, kr25, kr26 by the statements of chem_advance_setup (the point sources' over the clipped state, the
 *                   self-shielding test on the state as the equilibrium routines take it); the heating rates per absorber c24,
 *                   c25, c26 by thermal_heating from the incoming state as thermal_species takes it; the incoming temperature
 *                   clipped to [tmin, tmax].  All six stay fixed for the call: the radiation is the step's, what changes inside
 *                   the call is the gas.
 *   subcycle s      while remaining > 0 (remaining = dt at the start):
 *     1. logtem is the cell's stored logarithm for s = 0 -- what chem_advance_cell would read -- and ftte_log(T) after;
 *        chem_coefficients and the thirteen cooling coefficients at it;
 *     2. the state at hand, clipped for s > 0 as the chemistry takes it (chem_advance_clip), gives de = (nh - HI) + HeII +
 *        2 (nhe - HeI - HeII), the three right-hand sides written above chem_advance_step, dT/dt = (edot(T) + extra) / c with
 *        c = kB (nh + nhe + de) / (gamma - 1), and
 *          tau = min( max(HI, f nh)/|dHI/dt|, max(HeI, f nhe)/|dHeI/dt|, max(HeII, f nhe)/|dHeII/dt|, T/|dT/dt| ),
 *        f = THERMOCHEM_FLOOR; a derivative of zero gives +infinity, and that is meant;
 *     3. h = min(remaining, max(eta > 0 ? eta tau : 0, remaining / (max_subcycles - s))): the second term ends the call within
 *        max_subcycles subcycles whatever eta is -- at worst the rest of the interval is split evenly; eta = 0 is the uniform
 *        schedule;
 *     4. the chemistry over h (chem_advance_close);
 *     5. the temperature over h with the new species: thermal_species, crate = c24 HI + c25 HeII + c26 HeI, hc = h / c with c
 *        of the new species, thermal_advance_close from the current T;
 *     6. remaining = h >= remaining ? 0 : remaining - h.
 *
 * First order in h, the radiation explicit.  With max_subcycles = 1 the species are chem_advance_cell(dt, 1)'s bit for bit, and
 * the temperature is thermal_advance_cell(dt, 1)'s on those species wherever the heating per absorber does not depend on the
 * state (the transfer's J without point sources); elsewhere the pair forms c24..c26 from the NEW species and this statement from
 * the incoming ones.  A cell fails for any reason either step fails, in any subcycle, and by chem_advance_cell's test of the
 * final fractions.
 *
 * Conventions of the two headers: FTTE_HD functions, IEEE add, multiply, divide, fmin, fmax, fabs, the one logarithm ftte_log;
 * compiled with -ffp-contract=off by hipcc (ftte_thermochem.hip) and by g++ (tests/host/thermochem_check.cpp): the same bits.
 */
#ifndef FTTE_THERMOCHEM_MATH_H
#define FTTE_THERMOCHEM_MATH_H

#include "ftte_thermal_math.h"

/* the floor under a species in its own time scale, as a fraction of its element: a trace species does not set the step until
 * it has grown to this (measured: DESIGN.md, the section on the coupled step) */
#define THERMOCHEM_FLOOR 0.2

/* a / |b|, +infinity for b = 0 (a > 0) */
FTTE_HD double thermochem_scale(double a, double b) { return a / fabs(b); }

/* The time scale tau of item 2 for the state (HI, HeI, HeII) -- within its budgets -- at temperature temp, with the
 * coefficients of q and coef at that temperature.  s: thermal_species of that state; crate: its heating. */
FTTE_HD double thermochem_time_scale(const ChemEq *q, const double *coef, const ThermalSpecies *s, double rho, double HI, double HeI,
                                     double HeII, double temp, double comp1, double comp2, double crate, double extra)
{
    const double de = s->de;
    const double a = q->k1 * de + q->kr24, b = q->k2 * de;
    const double X = q->k3 * de + q->kr26, Y = q->k4 * de, W = q->k5 * de + q->kr25, Z = q->k6 * de;
    const double dHI = b * (q->nh - HI) - a * HI;
    const double dHeI = Y * HeII - X * HeI;
    const double dHeII = X * HeI - (Y + W) * HeII + Z * (q->nhe - HeI - HeII);
    double cooling;
    const double dT = (thermal_edot(coef, s, temp, comp1, comp2, crate, &cooling) + extra) / thermal_heat_capacity(rho, de);
    const double t1 = thermochem_scale(fmax(HI, THERMOCHEM_FLOOR * q->nh), dHI), t2 = thermochem_scale(fmax(HeI, THERMOCHEM_FLOOR * q->nhe), dHeI),
                 t3 = thermochem_scale(fmax(HeII, THERMOCHEM_FLOOR * q->nhe), dHeII), t4 = thermochem_scale(temp, dT);
    return fmin(fmin(t1, t2), fmin(t3, t4));
}

/* the length of subcycle s (item 3); *even whether the even split of the rest decided it */
FTTE_HD double thermochem_subcycle(double remaining, double eta, double tau, int max_subcycles, int s, int *even)
{
    const double own = eta > 0. ? eta * tau : 0., split = remaining / (double)(max_subcycles - s);
    *even = own < split;
    return fmin(remaining, fmax(own, split));
}

/* Species and temperature of one cell advanced over dt.  In: as chem_advance_cell and thermal_advance_cell -- the point
 * sources' ionisation rates p24..p26 and heating rates e24..e26 of the cell (point != 0), the transfer's J with ksi and gamma or
 * the uniform background's two triples behind the self-shielding test, Compton's two numbers, `extra` (the stored hydroHeating,
 * or 0) -- and eta, max_subcycles (>= 1), the clip [tmin, tmax].  Out: whether the cell got through; HI, HeI, HeII, T and
 * ftte_log(T) (0 for a cell that failed); the bisection steps of both kinds; the subcycles taken; whether the even split ever
 * decided a subcycle; the change of the species as chem_advance_cell measures it; |T1 - T0| / T0, T0 the clipped incoming T. */
FTTE_HD int thermochem_advance_cell(const ftte_consts *K, const ChemTable *T, const ThermalTable *C, double rho, double tgas, double logtem,
                                    double HI0, double HeI0, double HeII0, double vol, int point, double p24, double p25, double p26, double e24,
                                    double e25, double e26, const double *J, long J_stride, const double *ksi, const double *uniform,
                                    const double *gamma, const double *uniform_gamma, double threshold, double comp1, double comp2, double extra,
                                    double dt, double eta, int max_subcycles, double tmin, double tmax, double *HI_out, double *HeI_out,
                                    double *HeII_out, double *T_out, double *logtem_out, unsigned long long *steps_out, int *subcycles_out,
                                    int *capped_out, double *change_out, double *tchange_out)
{
    ChemEq q;
    ThermalCell tc;
    double c24, c25, c26, HI = HI0, HeI = HeI0, HeII = HeII0, coef[THERMAL_NCOEF];
    q.nh = chem_nh(rho); q.nhe = chem_nhe(rho);
    {
        const double HIe = fmin(HI0, q.nh); /* the state as the equilibrium routines take it */
        chem_advance_clip(&q, &HI, &HeI, &HeII);
        chem_point_rates(&q, HI, HeI, HeII, vol, point, p24, p25, p26);
        chem_radiation_rates(&q, HIe, HeI0, HeII0, J, J_stride, ksi, uniform, threshold);
    }
    thermal_species(rho, HI0, HeI0, HeII0, &tc.s);
    thermal_heating(&tc.s, vol, point, e24, e25, e26, J, J_stride, gamma, uniform_gamma, threshold, &c24, &c25, &c26);
    tc.comp1 = comp1; tc.comp2 = comp2; tc.extra = extra;
    const double Tin = fmin(fmax(tgas, tmin), tmax);
    double Tnow = Tin, remaining = dt;
    unsigned long long steps = 0ull;
    int ok = thermal_finite(tgas) && thermal_finite(extra), s = 0, capped = 0;
    while (remaining > 0. && s < max_subcycles && ok) {
        const double lt = s ? ftte_log(K, Tnow) : logtem;
        chem_coefficients(T, lt, &q);
        thermal_coefficients(T, C, lt, coef);
        if (s) chem_advance_clip(&q, &HI, &HeI, &HeII);
        thermal_species(rho, HI, HeI, HeII, &tc.s);
        const double tau = thermochem_time_scale(&q, coef, &tc.s, rho, HI, HeI, HeII, Tnow, comp1, comp2, c24 * tc.s.HI + c25 * tc.s.HeII + c26 * tc.s.HeI,
                                                 extra);
        int even;
        const double h = thermochem_subcycle(remaining, eta, tau, max_subcycles, s, &even);
        capped |= even;
        const unsigned n = chem_advance_close(&q, h, &HI, &HeI, &HeII);
        steps += (unsigned long long)n;
        thermal_species(rho, HI, HeI, HeII, &tc.s);
        tc.crate = c24 * tc.s.HI + c25 * tc.s.HeII + c26 * tc.s.HeI;
        const double heat_capacity = thermal_heat_capacity(rho, tc.s.de);
        tc.hc = h / heat_capacity;
        tc.T0 = Tnow;
        ok = n < CHEM_MAX_STEPS && heat_capacity > 0. && thermal_finite(heat_capacity) && thermal_finite(tc.crate);
        if (ok) steps += (unsigned long long)thermal_advance_close(K, T, C, &tc, tmin, tmax, &Tnow, &ok);
        remaining = h >= remaining ? 0. : remaining - h;
        ++s;
    }
    const double fH = HI / q.nh, fHe = (HeI + HeII) / q.nhe;
    /* (a NaN fails every comparison; an infinity the range) */
    ok = ok && !(remaining > 0.) && fH >= -CHEM_ADVANCE_SLACK && fH <= 1. + CHEM_ADVANCE_SLACK && fHe >= -CHEM_ADVANCE_SLACK &&
         fHe <= 1. + CHEM_ADVANCE_SLACK && HeI >= -CHEM_ADVANCE_SLACK * q.nhe && HeII >= -CHEM_ADVANCE_SLACK * q.nhe;
    const double c1 = fabs(HI - HI0) * FTTE_MH / (FTTE_PSI * rho), c2 = fabs(HeI - HeI0) * FTTE_MHE / ((1. - FTTE_PSI) * rho),
                 c3 = fabs(HeII - HeII0) * FTTE_MHE / ((1. - FTTE_PSI) * rho);
    *change_out = fmax(c1, fmax(c2, c3));
    *tchange_out = fabs(Tnow - Tin) / Tin;
    *HI_out = HI; *HeI_out = HeI; *HeII_out = HeII;
    *T_out = Tnow;
    *logtem_out = ok ? ftte_log(K, Tnow) : 0.;
    *steps_out = steps;
    *subcycles_out = s;
    *capped_out = capped;
    return ok;
}

#endif /* FTTE_THERMOCHEM_MATH_H */
