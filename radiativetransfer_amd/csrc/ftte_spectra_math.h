/* ftte_spectra_math.h -- one absorption line along a sightline, written once.
 *
 * A sightline crosses leaves l = 0, 1, ... in order.  Leaf l has path D_l [cm] (its size), absorber density n_l, temperature T_l
 * and line-of-sight velocity u_l, and lies with its centre s_l [cm] behind the entry face of the first base cell.  With the line
 * line[4] = {sigma_line = (pi e^2 / m_e c) f lambda0 [cm^2 cm/s], damping = Gamma lambda0 / 4 pi [cm/s], mass [g], b_turb [cm/s]}:
 *   N_l = n_l D_l,   b_l = sqrt(2 k_B T_l / mass + b_turb^2),   a_l = damping / b_l,   v_l = hubble s_l + u_l,
 * and at pixel p, v_p = v0 + (p + 1/2) dv, with d = v_p - v_l (reduced by period rint(d / period) where period > 0) and x = d / b_l,
 *   tau_p = sum_l N_l sigma_line / (sqrt(pi) b_l) H(a_l, x),
 * the leaves in sightline order, one running sum per pixel.  H is Tepper-Garcia's (2006) form of the Voigt function,
 *   H = H0 - a / (sqrt(pi) x^2) [H0^2 (4 x^4 + 7 x^2 + 4 + Q) - Q - 1],   H0 = exp(-x^2),  Q = 1.5 / x^2,
 * with H0 exactly 0 for x^2 > 64 and, for x^2 < 1e-4, the bracket over x^2 replaced by its limit 2 (the raw form loses every
 * digit as x -> 0).  a = 0 is the Doppler profile H0 itself; a pair with a = 0 and x^2 > 64 adds nothing and is passed over.
 * Of a finished sightline: N = sum N_l (same order), W = sum_p (1 - exp(-tau_p)) dv with the bracket taken as tau g(tau) from
 * ftte_attenuation, and dv90 = (p_hi - p_lo) dv, p_lo and p_hi the first pixels whose running sum of tau reaches 0.05 and 0.95
 * of the total (p ascending; 0 where the total is not positive).
 *
 * Conventions of ftte_math.h: FTTE_HD functions, plain C plus HIP, every exponential ftte_attenuation, the root corrected to the
 * correctly rounded one whatever the library's last bit is, the per-pair division FTTE_DIV inside its range (x^2 is capped at
 * 2^200, far beyond any velocity a double holds in cm/s against a thermal width), everything else IEEE adds, multiplies and
 * divisions with nothing fused.  The same source is compiled by hipcc into the kernels of ftte_spectra.hip and by g++ into the
 * tests' host library (tests/host/spectra_check.cpp), which the GPU is compared with bit for bit.
 */
#ifndef FTTE_SPECTRA_MATH_H
#define FTTE_SPECTRA_MATH_H

#include <stdint.h>

#include "ftte_math.h"

#define FTTE_SPECTRA_KB 1.380649e-16                    /* erg / K */
#define FTTE_SPECTRA_INV_SQRTPI 0x1.20dd750429b6dp-1    /* 1 / sqrt(pi) */
#define FTTE_SPECTRA_CORE 64.0                          /* x^2 beyond which exp(-x^2) is taken as 0 */
#define FTTE_SPECTRA_SMALL 1.0e-4                       /* x^2 below which the bracket over x^2 is its limit */
#define FTTE_SPECTRA_X2_MAX 0x1p+200

/* what a call fixes for all of its sightlines */
typedef struct {
    double v0, dv, hubble;
    double period, inv_period; /* 0, 0: no period */
    double sigma, damping, mass, bturb;
} ftte_spectra_par;

/* a leaf on a sightline, everything per-leaf computed once */
typedef struct {
    double amp;   /* N_l sigma_line / (sqrt(pi) b_l) */
    double v;     /* v_l */
    double inv_b; /* 1 / b_l */
    double a;     /* a_l */
} ftte_spectra_seg;

/* The correctly rounded square root (Tuckerman's test: s is it if and only if s pred(s) < q <= s succ(s); the fused multiply-add
 * gives the sign of each difference exactly) */
FTTE_HD double spectra_sqrt(double q)
{
    double s = __builtin_sqrt(q);
    if (q > 0x1p-900 && q < 0x1p+900) {
        union { double d; uint64_t u; } lo, hi;
        lo.d = s; hi.d = s;
        lo.u -= 1; hi.u += 1;
        if (FTTE_FMA(s, lo.d, -q) >= 0.0) s = lo.d;
        else if (FTTE_FMA(s, hi.d, -q) < 0.0) s = hi.d;
    }
    return s;
}

/* b_l^2, and whether a line can be made of it: positive and finite */
FTTE_HD double spectra_b2(const ftte_spectra_par *P, double tgas) { return (2.0 * FTTE_SPECTRA_KB * tgas) / P->mass + P->bturb * P->bturb; }
FTTE_HD int spectra_b2_ok(double q) { return q > 0.0 && q <= 0x1.fffffffffffffp+1023; }

/* The record of a leaf: density n, size [cm], temperature, centre s [cm], line-of-sight velocity u.  Returns N_l. */
FTTE_HD double spectra_segment(const ftte_spectra_par *P, double n, double size, double tgas, double s, double u, ftte_spectra_seg *S)
{
    const double N = n * size;
    const double b = spectra_sqrt(spectra_b2(P, tgas));
    const double inv_b = 1.0 / b;
    S->amp = ((N * P->sigma) * FTTE_SPECTRA_INV_SQRTPI) * inv_b;
    S->v = P->hubble * s + u;
    S->inv_b = inv_b;
    S->a = P->damping / b;
    return N;
}

FTTE_HD double spectra_pixel_velocity(const ftte_spectra_par *P, int64_t p) { return P->v0 + ((double)p + 0.5) * P->dv; }

/* x^2 of a pixel against a leaf */
FTTE_HD double spectra_x2(const ftte_spectra_par *P, const ftte_spectra_seg *S, double vp)
{
    double d = vp - S->v;
    if (P->period > 0.0) d = d - P->period * FTTE_RINT(d * P->inv_period);
    const double x = d * S->inv_b;
    const double x2 = x * x;
    return x2 > FTTE_SPECTRA_X2_MAX ? FTTE_SPECTRA_X2_MAX : x2; /* (a NaN stays one) */
}

/* H(a, x) from x^2 and H0 = exp(-x^2) (0 beyond the core) */
FTTE_HD double spectra_voigt(double a, double x2, double H0)
{
    if (!(a > 0.0)) return H0;
    const double c = a * FTTE_SPECTRA_INV_SQRTPI;
    if (x2 < FTTE_SPECTRA_SMALL) return H0 - c * 2.0;
    const double r = FTTE_DIV(1.0, x2);
    const double Q = 1.5 * r;
    const double x4 = x2 * x2;
    const double poly = ((4.0 * x4 + 7.0 * x2) + 4.0) + Q;
    const double B = ((H0 * H0) * poly - Q) - 1.0;
    return H0 - c * (B * r);
}

/* spectra_voigt(a, x2, 0) for a > 0 and x^2 beyond the core, the same bits with less work: there H0^2 (...) is +0 whatever the
 * (finite, positive) polynomial, and 0 - Q is -Q */
FTTE_HD double spectra_wing(double a, double x2)
{
    const double c = a * FTTE_SPECTRA_INV_SQRTPI;
    const double r = FTTE_DIV(1.0, x2);
    const double Q = 1.5 * r;
    const double B = (0.0 - Q) - 1.0;
    return 0.0 - c * (B * r);
}

/* H0 of x^2: ftte_attenuation inside the core, exactly 0 beyond */
FTTE_HD double spectra_gauss(const ftte_consts *K, double x2)
{
    const int core = x2 <= FTTE_SPECTRA_CORE;
    double e, g;
    ftte_attenuation(K, core ? x2 : FTTE_SPECTRA_CORE, &e, &g);
    return core ? e : 0.0;
}

/* tau of a pixel after one more leaf.  On the device the test of the core is the wavefront's: a leaf whose core lies outside all of
 * a wavefront's pixels costs it that one branch when a = 0, and the wings alone (spectra_wing) when a > 0. */
FTTE_HD double spectra_accumulate(const ftte_consts *K, const ftte_spectra_par *P, const ftte_spectra_seg *S, double vp, double tau)
{
    const double x2 = spectra_x2(P, S, vp);
    const int core = x2 <= FTTE_SPECTRA_CORE, wings = S->a > 0.0;
    if (FTTE_ANY(core)) {
        const double H = spectra_voigt(S->a, x2, spectra_gauss(K, x2));
        const double sum = tau + S->amp * H;
        return (core || wings) ? sum : tau;
    }
    if (wings) return tau + S->amp * spectra_wing(S->a, x2);
    return tau;
}

/* (1 - exp(-tau)) dv of one pixel */
FTTE_HD double spectra_width_term(const ftte_consts *K, double tau, double dv)
{
    double e, g;
    ftte_attenuation(K, tau, &e, &g);
    return (tau * g) * dv;
}

/* dv90 from the total of tau and the two pixels found (-1: none) */
FTTE_HD double spectra_dv90(double total, int64_t p_lo, int64_t p_hi, double dv)
{
    return (total > 0.0 && p_lo >= 0 && p_hi >= 0) ? (double)(p_hi - p_lo) * dv : 0.0;
}

/* W and dv90 of a finished sightline, sequentially in p: what the kernel's one summing lane does */
FTTE_HD void spectra_summarise(const ftte_consts *K, const double *tau, int64_t nvel, double dv, double *W, double *dv90)
{
    double w = 0.0, total = 0.0;
    for (int64_t p = 0; p < nvel; ++p) {
        w = w + spectra_width_term(K, tau[p], dv);
        total = total + tau[p];
    }
    const double t_lo = 0.05 * total, t_hi = 0.95 * total;
    double run = 0.0;
    int64_t p_lo = -1, p_hi = -1;
    for (int64_t p = 0; p < nvel; ++p) {
        run = run + tau[p];
        if (p_lo < 0 && run >= t_lo) p_lo = p;
        if (p_hi < 0 && run >= t_hi) p_hi = p;
    }
    *W = w;
    *dv90 = spectra_dv90(total, p_lo, p_hi, dv);
}

#endif /* FTTE_SPECTRA_MATH_H */
