/* ftte_ray_math.h -- a straight ray through the refined grid, written once.
 *
 * Frame and units: the storage frame of the tracer and of ftte_set_velocity (x along storage-i, y along j, z along k), lengths in
 * base cells: the box is [0, n]^3 and every leaf face is an integer plus an exact dyadic fraction.  A ray is origin o, unit
 * direction d and an optional end tmax (<= 0: to the box's far side); inv_a = 1 / d_a, one IEEE division per axis with d_a != 0.
 * An axis with d_a == 0 (either sign) takes no part in any min or max; a ray whose origin on such an axis is outside [0, n) misses.
 *
 * A leaf occupies [lo_a, lo_a + h] per axis, h = 2^-level.  Its exit is t_out = min_a (far_a - o_a) inv_a with far_a = lo_a + h
 * for d_a > 0 and lo_a for d_a < 0; the exit axis is the argmin, ties to the lowest axis.  The ray starts at t_start = max(0, box
 * entry), the entry being the max over axes of (near face - o_a) inv_a, and ends at t_end = min(box exit, tmax); it misses unless
 * t_start < t_end.  A segment is [t_in, t_out'] with t_in the running t and t_out' = min(t_out, t_end); its chord is t_out' - t_in.
 * A chord <= 0 gives no segment and leaves the running t where it is (the last-bit disorder of two t's computed on different
 * axes; at a tie the tied axes' t's are the same expression, the chord between them is exactly 0 and a corner is crossed through
 * leaves that give nothing).  The running t starts at t_start, every segment starts where the last one ended and the walk ends
 * only with t_out >= t_end: the segments tile [t_start, t_end] by construction.
 *
 * The next leaf: across the exit face the coordinate on the exit axis is the face itself; the two transverse ones are
 * o_b + t_out d_b clamped into the current leaf's [lo_b, lo_b + h].  A coordinate on a face belongs to the cell on the side the ray
 * moves to; with d_b == 0 to the half-open cell [lo, lo + h).  From that point the walk descends from the base cell again
 * (ray_locate): every subtraction and doubling on the way is exact.  Along every axis the faces crossed are monotone: at most
 * 3 n 2^maxlevel + 3 steps (ray_step_bound); a walk that needs more has failed and says so.
 *
 * What a segment gives the line (spectra_segment of ftte_spectra_math.h): size = chord cell_cm, s = ((t_in + t_out') 0.5) cell_cm
 * from the ray's origin, u = (d_0 velx + d_1 vely) + d_2 velz of the leaf.  For d = +-e_a, an origin on a base cell's face and
 * dyadic transverse coordinates every t is exact, the chord is the leaf's size and s is that of the axis-aligned sightlines.
 *
 * Conventions of ftte_math.h: FTTE_HD functions, plain C plus HIP, IEEE adds, multiplies and divisions with nothing fused.  No
 * array is indexed by a run-time axis: selects, so that a lane keeps everything in registers.  The same source is compiled by hipcc
 * into the kernels of ftte_rays.hip and by g++ into the tests' host library (tests/host/ray_check.cpp), which the GPU equals bit
 * for bit.
 */
#ifndef FTTE_RAY_MATH_H
#define FTTE_RAY_MATH_H

#include <stdint.h>

#include "ftte_math.h"

#define FTTE_RAY_UNIT_TOL 1.0e-9 /* | |d|^2 - 1 | a caller's direction may have */
#define FTTE_RAY_MAX_LEVEL 40    /* n 2^level stays far inside 2^53 */

/* a tree node as the device holds it: the layout of ftte::NodeRec (ftte_node_rec.h; asserted in ftte_rays.h) */
typedef struct { int32_t child0, leaf, parent, level; } ftte_ray_node;

typedef struct {
    double ox, oy, oz, dx, dy, dz, ix, iy, iz; /* origin, direction, 1 / direction (0 where the direction is 0) */
    double t_start, t_end;
    int hit;
} ftte_ray;

/* the walk's state: the running t, the point the next leaf is found from, and the leaf found */
typedef struct {
    double t, px, py, pz;
    double lox, loy, loz, h;
    int64_t leaf; /* cell-array index */
    int done;
} ftte_ray_walk;

FTTE_HD int ray_finite(double v) { return v - v == 0.0; }

/* what a call refuses: a component that is not finite, a direction that is no unit vector */
FTTE_HD int ray_arguments_ok(const double *o, const double *d, const double *tmax)
{
    if (!ray_finite(o[0]) || !ray_finite(o[1]) || !ray_finite(o[2]) || !ray_finite(d[0]) || !ray_finite(d[1]) || !ray_finite(d[2])) return 0;
    if (tmax && !ray_finite(*tmax)) return 0;
    const double q = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) - 1.0;
    return q <= FTTE_RAY_UNIT_TOL && q >= -FTTE_RAY_UNIT_TOL;
}

/* 3 n 2^maxlevel + 3, or 0 where the tree is deeper than the walk goes */
FTTE_HD int64_t ray_step_bound(int n, int max_level)
{
    if (max_level < 0 || max_level > FTTE_RAY_MAX_LEVEL || n < 1) return 0;
    return 3 * ((int64_t)n << max_level) + 3;
}

/* entry and exit of one axis of the box into the running max and min */
FTTE_HD void ray_box_axis(double o, double d, double inv, double n, double *t_in, double *t_out, int *axis_in, int axis, int *miss)
{
    if (d == 0.0) {
        if (!(o >= 0.0 && o < n)) *miss = 1;
        return;
    }
    const double tn = ((d > 0.0 ? 0.0 : n) - o) * inv, tf = ((d > 0.0 ? n : 0.0) - o) * inv;
    if (*axis_in < 0 || tn > *t_in) { *t_in = tn; *axis_in = axis; }
    if (tf < *t_out) *t_out = tf;
}

FTTE_HD double ray_clamp(double v, double lo, double hi) { return !(v >= lo) ? lo : v > hi ? hi : v; } /* (a NaN becomes lo) */

/* The ray and the point its walk starts from.  tmax <= 0: to the far side of the box. */
FTTE_HD void ray_begin(ftte_ray *R, ftte_ray_walk *W, int n, const double *o, const double *d, double tmax)
{
    const double dn = (double)n;
    R->ox = o[0]; R->oy = o[1]; R->oz = o[2];
    R->dx = d[0]; R->dy = d[1]; R->dz = d[2];
    R->ix = d[0] != 0.0 ? 1.0 / d[0] : 0.0;
    R->iy = d[1] != 0.0 ? 1.0 / d[1] : 0.0;
    R->iz = d[2] != 0.0 ? 1.0 / d[2] : 0.0;
    double t_in = 0.0, t_out = 0x1.fffffffffffffp+1023;
    int axis_in = -1, miss = 0;
    ray_box_axis(R->ox, R->dx, R->ix, dn, &t_in, &t_out, &axis_in, 0, &miss);
    ray_box_axis(R->oy, R->dy, R->iy, dn, &t_in, &t_out, &axis_in, 1, &miss);
    ray_box_axis(R->oz, R->dz, R->iz, dn, &t_in, &t_out, &axis_in, 2, &miss);
    if (axis_in < 0) miss = 1; /* (no direction at all) */
    const int inside = !(t_in > 0.0);
    R->t_start = inside ? 0.0 : t_in;
    R->t_end = (tmax > 0.0 && tmax < t_out) ? tmax : t_out;
    R->hit = !miss && !(t_in > t_out) && R->t_start < R->t_end;
    /* the first point: the origin itself, or the entry face exactly on its axis and the ray's point at t_start inside the box on the others */
    const double t = R->t_start;
    double px = inside ? R->ox : ray_clamp(R->ox + t * R->dx, 0.0, dn);
    double py = inside ? R->oy : ray_clamp(R->oy + t * R->dy, 0.0, dn);
    double pz = inside ? R->oz : ray_clamp(R->oz + t * R->dz, 0.0, dn);
    if (!inside) {
        if (axis_in == 0) px = R->dx > 0.0 ? 0.0 : dn;
        else if (axis_in == 1) py = R->dy > 0.0 ? 0.0 : dn;
        else pz = R->dz > 0.0 ? 0.0 : dn;
    }
    W->t = t; W->px = px; W->py = py; W->pz = pz;
    W->lox = W->loy = W->loz = 0.0; W->h = 1.0;
    W->leaf = -1;
    W->done = !R->hit;
}

/* the base cell of a coordinate and the coordinate's fraction of it in [0, 1]: a coordinate on a face goes where the ray moves to */
FTTE_HD int ray_base_cell(double p, double d, int n, double *frac)
{
    double fl = __builtin_floor(p);
    if (d < 0.0 && p == fl) fl = fl - 1.0;
    fl = ray_clamp(fl, 0.0, (double)(n - 1));
    *frac = ray_clamp(p - fl, 0.0, 1.0);
    return (int)fl;
}

/* the half of a cell a fraction lies in, and the fraction of that half */
FTTE_HD int ray_half(double *f, double d)
{
    const int up = d < 0.0 ? *f > 0.5 : *f >= 0.5;
    *f = up ? 2.0 * *f - 1.0 : 2.0 * *f;
    return up;
}

/* The leaf of the walk's point, from the base cell down: W->leaf, lo and h.  node == NULL: a uniform grid, base cell == leaf.
 * Returns 0 where the tree has no leaf within FTTE_RAY_MAX_LEVEL + 1 levels. */
FTTE_HD int ray_locate(const ftte_ray *R, ftte_ray_walk *W, int n, const ftte_ray_node *node)
{
    double fx, fy, fz;
    const int bx = ray_base_cell(W->px, R->dx, n, &fx), by = ray_base_cell(W->py, R->dy, n, &fy), bz = ray_base_cell(W->pz, R->dz, n, &fz);
    int64_t at = ((int64_t)bx * n + by) * n + bz;
    double lox = (double)bx, loy = (double)by, loz = (double)bz, h = 1.0;
    if (!node) {
        W->leaf = at; W->lox = lox; W->loy = loy; W->loz = loz; W->h = h;
        return 1;
    }
    ftte_ray_node N = node[at];
    int level = 0;
    while (N.child0 >= 0) {
        if (++level > FTTE_RAY_MAX_LEVEL + 1) return 0;
        h = h * 0.5;
        const int a = ray_half(&fx, R->dx), b = ray_half(&fy, R->dy), c = ray_half(&fz, R->dz);
        lox = a ? lox + h : lox;
        loy = b ? loy + h : loy;
        loz = c ? loz + h : loz;
        at = (int64_t)N.child0 + (4 * a + 2 * b + c);
        N = node[at];
    }
    W->leaf = (int64_t)N.leaf; W->lox = lox; W->loy = loy; W->loz = loz; W->h = h;
    return 1;
}

/* the face a ray leaves a cell [lo, lo + h] through, on one axis */
FTTE_HD double ray_far(double lo, double h, double d) { return d > 0.0 ? lo + h : lo; }

/* t_out of the leaf found and its exit axis: the argmin over the axes with a direction, ties to the lowest axis */
FTTE_HD double ray_exit(const ftte_ray *R, const ftte_ray_walk *W, int *exit_axis)
{
    double t = 0x1.fffffffffffffp+1023;
    int axis = -1;
    if (R->dx != 0.0) { t = (ray_far(W->lox, W->h, R->dx) - R->ox) * R->ix; axis = 0; }
    if (R->dy != 0.0) { const double ty = (ray_far(W->loy, W->h, R->dy) - R->oy) * R->iy; if (axis < 0 || ty < t) { t = ty; axis = 1; } }
    if (R->dz != 0.0) { const double tz = (ray_far(W->loz, W->h, R->dz) - R->oz) * R->iz; if (axis < 0 || tz < t) { t = tz; axis = 2; } }
    *exit_axis = axis;
    return t;
}

/* Through the leaf found: its segment [*t_in, *t_out] where the return is 1 (a chord > 0), and on to the point the next leaf is
 * found from, or W->done. */
FTTE_HD int ray_cross(const ftte_ray *R, ftte_ray_walk *W, int n, double *t_in, double *t_out)
{
    const double h = W->h, dn = (double)n;
    int axis;
    const double t = ray_exit(R, W, &axis);
    const double cut = t < R->t_end ? t : R->t_end;
    const int some = cut - W->t > 0.0;
    if (some) { *t_in = W->t; *t_out = cut; W->t = cut; }
    if (!(t < R->t_end)) { W->done = 1; return some; }
    /* (values first, then the select: a select among the fields' addresses would put the walk's state into memory) */
    const double farx = ray_far(W->lox, h, R->dx), fary = ray_far(W->loy, h, R->dy), farz = ray_far(W->loz, h, R->dz);
    const double far = axis == 0 ? farx : axis == 1 ? fary : farz, d = axis == 0 ? R->dx : axis == 1 ? R->dy : R->dz;
    if (d > 0.0 ? far >= dn : far <= 0.0) { W->done = 1; return some; } /* (out of the box: t_end is no later) */
    W->px = axis == 0 ? far : ray_clamp(R->ox + t * R->dx, W->lox, W->lox + h);
    W->py = axis == 1 ? far : ray_clamp(R->oy + t * R->dy, W->loy, W->loy + h);
    W->pz = axis == 2 ? far : ray_clamp(R->oz + t * R->dz, W->loz, W->loz + h);
    return some;
}

/* s [base cells] and u of a segment for spectra_segment; vx, vy, vz the leaf's velocity */
FTTE_HD double ray_segment_s(double t_in, double t_out) { return (t_in + t_out) * 0.5; }
FTTE_HD double ray_segment_u(const ftte_ray *R, double vx, double vy, double vz) { return (R->dx * vx + R->dy * vy) + R->dz * vz; }

/* ---- The periodic ray: the box tiles space with period n on every axis and the ray goes on through the opposite face.
 *
 * A periodic ray is an origin o (any finite point), the caller's unit vector d and a length tmax, finite and > 0: it always hits,
 * t_start = 0 at the origin, t_end = tmax, and t is measured from the caller's origin along the whole ray, across images.
 *
 * Image and local origin: per axis an integer image w_a = floor(o_a / n), one lower where d_a < 0 and o_a == w_a n exactly (a
 * coordinate on a face belongs to the side the ray moves to; with d_a == 0 the half-open cell holds), and the local origin
 * o'_a = o_a - w_a n clamped into [0, n].  The walk runs in local coordinates with o' in the place of R->o: ray_locate, ray_exit,
 * ray_far, the clamp of the transverse coordinates and the "chord <= 0 gives nothing" rule are used as they stand.
 *
 * The wrap: where the non-periodic walk leaves the box (the exit axis's far face is >= n or <= 0) the periodic one steps w_a by
 * +-1, recomputes o'_a = o_a - w_a n from the caller's o_a and the integer image -- never from the previous o'_a, so nothing drifts
 * however many boxes are crossed -- and puts the point on the exit axis on the opposite face, 0 for d_a > 0 and n for d_a < 0; the
 * transverse coordinates are carried as in ray_cross.  The one-ulp disorder of t between two images of an axis is absorbed by the
 * chord rule.  The segments tile [0, tmax] by construction.  Every step still crosses a leaf face forwards on its exit axis:
 * ray_step_bound_periodic.
 *
 * What a segment gives the line is as above: s is the midpoint's distance from the caller's origin, so the Hubble velocity keeps
 * growing across images (the line's period folds velocities, not positions).  For d = +-e_a, an origin on a base cell's face and
 * dyadic transverse coordinates every t is exact: a ray of length k n gives the one-box list k times, t shifted by exactly j n. */
#define FTTE_RAY_MAX_BOXES 0x1p20 /* tmax / n a periodic call may ask for */

/* the caller's origin and the image the walk is in */
typedef struct {
    double cox, coy, coz;
    int32_t wx, wy, wz; /* (inside +-(2^21 + 1): ray_periodic_refusal, ray_step_bound_periodic) */
} ftte_ray_image;

/* 3 (n 2^maxlevel) (ceil(tmax / n) + 1) + 3, or 0 where the tree is deeper than the walk goes, tmax / n is above 2^20 (or tmax
 * is not > 0) or the product would leave 2^62 */
FTTE_HD int64_t ray_step_bound_periodic(int n, int max_level, double tmax)
{
    if (max_level < 0 || max_level > FTTE_RAY_MAX_LEVEL || n < 1) return 0;
    const double boxes = tmax / (double)n;
    if (!(tmax > 0.0) || !(boxes <= FTTE_RAY_MAX_BOXES)) return 0;
    const double images = __builtin_ceil(boxes) + 1.0, fine = (double)n * (double)((int64_t)1 << max_level);
    if (!(3.0 * fine * images + 3.0 < 0x1p62)) return 0;
    return 3 * ((int64_t)n << max_level) * (int64_t)images + 3;
}

/* What a periodic call refuses beyond ray_arguments_ok: 1 a tmax that is absent or not > 0; 2 an origin more than 2^20 boxes from
 * the box on an axis (the image counters and w_a n stay exact integers far inside 2^53).  0: a good ray. */
FTTE_HD int ray_periodic_refusal(const double *o, const double *tmax, int n)
{
    if (!tmax || !(*tmax > 0.0)) return 1;
    const double far = FTTE_RAY_MAX_BOXES * (double)n;
    if (!(o[0] >= -far && o[0] <= far && o[1] >= -far && o[1] <= far && o[2] >= -far && o[2] <= far)) return 2;
    return 0;
}

/* one axis of the image and of the local origin */
FTTE_HD double ray_image_axis(double o, double d, double dn, int32_t *w)
{
    double fl = __builtin_floor(o / dn);
    if (d < 0.0 && o == fl * dn) fl = fl - 1.0;
    *w = (int32_t)fl;
    return ray_clamp(o - fl * dn, 0.0, dn);
}

/* The periodic ray and the point its walk starts from: its origin, in the image that holds it. */
FTTE_HD void ray_begin_periodic(ftte_ray *R, ftte_ray_walk *W, ftte_ray_image *I, int n, const double *o, const double *d, double tmax)
{
    const double dn = (double)n;
    I->cox = o[0]; I->coy = o[1]; I->coz = o[2];
    R->dx = d[0]; R->dy = d[1]; R->dz = d[2];
    R->ix = d[0] != 0.0 ? 1.0 / d[0] : 0.0;
    R->iy = d[1] != 0.0 ? 1.0 / d[1] : 0.0;
    R->iz = d[2] != 0.0 ? 1.0 / d[2] : 0.0;
    R->ox = ray_image_axis(o[0], d[0], dn, &I->wx);
    R->oy = ray_image_axis(o[1], d[1], dn, &I->wy);
    R->oz = ray_image_axis(o[2], d[2], dn, &I->wz);
    R->t_start = 0.0;
    R->t_end = tmax;
    R->hit = tmax > 0.0 && (R->dx != 0.0 || R->dy != 0.0 || R->dz != 0.0);
    W->t = 0.0; W->px = R->ox; W->py = R->oy; W->pz = R->oz;
    W->lox = W->loy = W->loz = 0.0; W->h = 1.0;
    W->leaf = -1;
    W->done = !R->hit;
}

/* ray_cross with the wrap: through the leaf found, its segment where the return is 1, and on to the point the next leaf is found
 * from -- across the box's face that is the opposite face of the next image -- or W->done at tmax. */
FTTE_HD int ray_cross_periodic(ftte_ray *R, ftte_ray_walk *W, ftte_ray_image *I, int n, double *t_in, double *t_out)
{
    const double h = W->h, dn = (double)n;
    int axis;
    const double t = ray_exit(R, W, &axis);
    const double cut = t < R->t_end ? t : R->t_end;
    const int some = cut - W->t > 0.0;
    if (some) { *t_in = W->t; *t_out = cut; W->t = cut; }
    if (!(t < R->t_end)) { W->done = 1; return some; }
    /* (values first, then the selects, as in ray_cross) */
    const double farx = ray_far(W->lox, h, R->dx), fary = ray_far(W->loy, h, R->dy), farz = ray_far(W->loz, h, R->dz);
    const double far = axis == 0 ? farx : axis == 1 ? fary : farz, d = axis == 0 ? R->dx : axis == 1 ? R->dy : R->dz;
    const int wrap = d > 0.0 ? far >= dn : far <= 0.0;
    const double px = ray_clamp(R->ox + t * R->dx, W->lox, W->lox + h);
    const double py = ray_clamp(R->oy + t * R->dy, W->loy, W->loy + h);
    const double pz = ray_clamp(R->oz + t * R->dz, W->loz, W->loz + h);
    const double face = !wrap ? far : d > 0.0 ? 0.0 : dn;
    const int32_t step = !wrap ? 0 : d > 0.0 ? 1 : -1;
    I->wx = axis == 0 ? I->wx + step : I->wx;
    I->wy = axis == 1 ? I->wy + step : I->wy;
    I->wz = axis == 2 ? I->wz + step : I->wz;
    /* the exit axis's local origin from the caller's origin and the integer image */
    const double ox = I->cox - (double)I->wx * dn, oy = I->coy - (double)I->wy * dn, oz = I->coz - (double)I->wz * dn;
    R->ox = wrap && axis == 0 ? ox : R->ox;
    R->oy = wrap && axis == 1 ? oy : R->oy;
    R->oz = wrap && axis == 2 ? oz : R->oz;
    W->px = axis == 0 ? face : px;
    W->py = axis == 1 ? face : py;
    W->pz = axis == 2 ? face : pz;
    return some;
}

#endif /* FTTE_RAY_MATH_H */
