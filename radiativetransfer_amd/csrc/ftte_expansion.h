// ftte_expansion.h -- the start-up expansion of HII regions (equiSources.f90:1035-1069: computeExpansionParameters :4395,
// findExpansion :4431, applyExpansion :4476): the records the kernel of ftte_expansion.hip reads, and the arithmetic the host and
// the device share -- a leaf's centre, the exact star-leaf test in the reference's operations, and the conservative test of a
// star's sphere against the box around a workgroup's leaf centres.  Needs nothing of the HIP runtime, so that the rules can be
// compiled and checked on their own (tests/host/expansion_cull_check.cpp).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define FTTE_XHD __host__ __device__ __forceinline__
#else
#define FTTE_XHD static inline
#endif

namespace ftte {

constexpr int kExpMaxLevels = 60; // the deepest tree ftte_set_grid accepts (AmrTree::build)
constexpr int kExpGroup = 256;    // leaves of a workgroup = threads = stars of an LDS tile
constexpr int kExpPathWords = 6;  // ten levels of three bits in each word

// Where a leaf of a refined cell array lies: its base cell (storage order, k fastest) and, for each refined ancestor from the base
// cell down, which child follows: bits (a << 2 | b << 1 | c) of step l at bit 3 (l % 10) of word l / 10, a, b, c = 0 for the lower
// half along x, y, z (the reference's cell(i,j,k), i, j, k = 1)
struct LeafPos {
    int32_t base;
    int32_t depth;
    uint32_t path[kExpPathWords];
};

// What the cull reads of a star, box units: the centre of its host leaf (absoluteCoordinates, equiSources.f90:3011-3047) and
// (finalRadius / physicalBoxSize)^2 inflated by a relative 2^-39, i.e. the radius by 2^-40
struct ExpStar { double x, y, z, r2; };
// What the exact test reads beside the centre: finalRadius [cm], densityCoefficient, 1.0001 * sourceTotalHydrogenDensity
struct ExpStarTest { double radius, coef, limit, reserved_; };

struct ExpandRec {
    const ExpStar *star;      // [nsrc]
    const ExpStarTest *test;  // [nsrc]
    const LeafPos *pos;       // [ncell], or nullptr on a uniform grid: the centre comes from the index
    double *rho, *HI, *HeI, *HeII; // scaled in place where rhoCoef < 1
    double *rho_coef;         // [ncell] or nullptr
    unsigned long long *counters; // [0] exact star-leaf tests, [1] leaves with rhoCoef < 1
    int64_t ncell;
    int32_t n, nsrc;
    double box;
    float shift[kExpMaxLevels]; // findExpansion's shift of a refined cell of level l: 0.25 / (float(2**l) * float(nx)), single precision
};

// shift = 0.25 / (float(2**currentCell%level)*float(nx)), equiSources.f90:4443: a single-precision product and quotient (inexact
// where nx is no power of two).  2**level is a default integer there and overflows from level 31 on; here the power of two goes on.
inline float expansion_shift(int level, int n)
{
    float p = 1.0f;
    for (int l = 0; l < level; ++l) p = p * 2.0f;
    const float den = p * (float)n;
    return 0.25f / den;
}

// (dfloat(i)-0.5)/dfloat(nx), i = 1..nx (equiSources.f90:1056): i0 = i - 1
FTTE_XHD double expansion_base_centre(int i0, int n) { return ((double)(i0 + 1) - 0.5) / (double)n; }

// findExpansion's descent (:4443-4462) along one axis: coarse to fine, minus the shift into the lower child, plus into the upper
FTTE_XHD void expansion_leaf_centre(const LeafPos &P, int n, const float *shift, double *x, double *y, double *z)
{
    const int k0 = P.base % n, j0 = (P.base / n) % n, i0 = P.base / (n * n);
    double cx = expansion_base_centre(i0, n), cy = expansion_base_centre(j0, n), cz = expansion_base_centre(k0, n);
    for (int l = 0; l < P.depth; ++l) {
        const uint32_t bits = P.path[l / 10] >> (3 * (l % 10));
        const double s = (double)shift[l];
        cx = (bits & 4u) ? cx + s : cx - s;
        cy = (bits & 2u) ? cy + s : cy - s;
        cz = (bits & 1u) ? cz + s : cz - s;
    }
    *x = cx; *y = cy; *z = cz;
}

// The correctly rounded square root whatever the library's last bit is (Tuckerman's test: s is it if and only if
// s * pred(s) < q <= s * succ(s); the fused multiply-add gives the sign of each difference exactly)
FTTE_XHD double expansion_sqrt(double q)
{
    double s = __builtin_sqrt(q);
    if (q > 0.0 && q < 1.0e300) {
        union { double d; uint64_t u; } lo, hi;
        lo.d = s; hi.d = s;
        lo.u -= 1; hi.u += 1;
        if (__builtin_fma(s, lo.d, -q) >= 0.0) s = lo.d;
        else if (__builtin_fma(s, hi.d, -q) < 0.0) s = hi.d;
    }
    return s;
}

// findExpansion's leaf branch (:4467-4469) for one star: dist = physicalBoxSize * sqrt((xbase-x)**2+(ybase-y)**2+(zbase-z)**2),
// summed left to right, nothing fused; nh_leaf = psi*rho/mh of the leaf before any expansion
FTTE_XHD bool expansion_accepts(const ExpStar &S, const ExpStarTest &T, double x, double y, double z, double nh_leaf, double box)
{
    const double dx = S.x - x, dy = S.y - y, dz = S.z - z;
    const double q = dx * dx + dy * dy + dz * dz;
    const double dist = box * expansion_sqrt(q);
    return dist < T.radius && nh_leaf <= T.limit;
}

// Can the star's sphere hold a leaf centre of the box [lo, hi]?  Conservative: never false where expansion_accepts is true for a
// centre inside the box.  Along each axis the distance to the box is the exact test's own subtraction against the nearer face (or
// zero inside), so by the monotonicity of rounding it is no larger in magnitude than the subtraction against any centre of the box;
// squares and the left-to-right sum keep that order, so q_box <= q of every leaf, bit for bit.  The exact test accepts where
// fl(box * fl(sqrt(q))) < radius, which bounds q by (radius / box)^2 (1 + 2^-50); r2 carries 2^-39.
FTTE_XHD bool expansion_sphere_reaches_box(const ExpStar &S, const double *lo, const double *hi)
{
    const double dx = S.x < lo[0] ? S.x - lo[0] : S.x > hi[0] ? S.x - hi[0] : 0.0;
    const double dy = S.y < lo[1] ? S.y - lo[1] : S.y > hi[1] ? S.y - hi[1] : 0.0;
    const double dz = S.z < lo[2] ? S.z - lo[2] : S.z > hi[2] ? S.z - hi[2] : 0.0;
    const double q = dx * dx + dy * dy + dz * dz;
    return q <= S.r2;
}

// the cull's radius of a star: (finalRadius / physicalBoxSize)^2 (1 + 2^-39)
inline double expansion_cull_r2(double radius_cm, double box)
{
    const double r = radius_cm / box;
    return r * r * (1.0 + 0x1p-39);
}

// computeExpansionParameters(nh), equiSources.f90:4395-4429 (host; libm's log10 and pow)
void expansion_parameters(double nh, double *final_radius_cm, double *density_coefficient);
// the centre of a star's host leaf as absoluteCoordinates forms it (:3011-3047) from (.5, .5, .5): i0, j0, k0 the base cell
// (0-based), P the leaf's path
void expansion_star_centre(const LeafPos &P, int n, double *x, double *y, double *z);

// asynchronous on `stream`; 0, -1 bad argument, -2 launch failure
int launch_expansion(const ExpandRec &R, void *stream);
int launch_gather(const double *field, const int64_t *cells, int count, double *out, void *stream);

} // namespace ftte
