// The host-testable rules of the expansion of HII regions (radiativetransfer_amd/csrc/ftte_expansion.h) under the address and
// undefined-behaviour sanitizers: the sphere-against-box cull never rejects a star that the exact test accepts for a centre inside
// the box (radii set on, one ulp below and one ulp above the distance of a centre included), the square root is the correctly
// rounded one, the position record holds the deepest tree's path, and the single-precision shifts are what findExpansion forms.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ftte_expansion.h"

using namespace ftte;

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); }       \
    } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_bits()
{
    g_state += 0x9E3779B97F4A7C15ull;
    uint64_t z = g_state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uniform01() { return (double)(next_bits() >> 11) * (1.0 / 9007199254740992.0); }

int main()
{
    // the square root
    CHECK(expansion_sqrt(0.0) == 0.0);
    for (int t = 0; t < 200000; ++t) {
        const double q = std::ldexp(uniform01() + 0.5, (int)(next_bits() % 80) - 70);
        CHECK(expansion_sqrt(q) == std::sqrt(q));
        const double r = std::floor(uniform01() * 1.0e6);
        CHECK(expansion_sqrt(r * r) == r);
    }

    // the shifts: 0.25 / (float(2**level) * float(nx)) in single precision
    const int sizes[] = {1, 3, 12, 16, 100, 1290, 32000};
    for (int n : sizes)
        for (int l = 0; l < kExpMaxLevels; ++l) {
            const float s = expansion_shift(l, n);
            CHECK(s > 0.0f && std::isfinite(s));
            if (l <= 30) CHECK(s == 0.25f / ((float)(1 << l) * (float)n));
            if (l > 0) CHECK(s < expansion_shift(l - 1, n));
        }

    // the position record: the deepest path, every step readable, the centre inside its base cell
    {
        const int n = 12;
        float shift[kExpMaxLevels];
        for (int l = 0; l < kExpMaxLevels; ++l) shift[l] = expansion_shift(l, n);
        for (int t = 0; t < 2000; ++t) {
            LeafPos P;
            std::memset(&P, 0, sizeof P);
            P.depth = t < 10 ? kExpMaxLevels : (int)(next_bits() % (kExpMaxLevels + 1));
            P.base = (int32_t)(next_bits() % (uint64_t)(n * n * n));
            int taken[kExpMaxLevels];
            for (int l = 0; l < P.depth; ++l) {
                taken[l] = (int)(next_bits() % 8);
                P.path[l / 10] |= (uint32_t)taken[l] << (3 * (l % 10));
            }
            for (int l = 0; l < P.depth; ++l) CHECK((int)((P.path[l / 10] >> (3 * (l % 10))) & 7u) == taken[l]);
            double x, y, z;
            expansion_leaf_centre(P, n, shift, &x, &y, &z);
            const int i0 = P.base / (n * n), j0 = (P.base / n) % n, k0 = P.base % n;
            const double slack = 1.0e-9; // (the shifts are rounded in single precision)
            CHECK(x > (double)i0 / n - slack && x < (double)(i0 + 1) / n + slack);
            CHECK(y > (double)j0 / n - slack && y < (double)(j0 + 1) / n + slack);
            CHECK(z > (double)k0 / n - slack && z < (double)(k0 + 1) / n + slack);
            if (P.depth > 0) {
                const double s0 = (double)shift[0], c = expansion_base_centre(i0, n);
                CHECK(((taken[0] & 4) ? x > c : x < c) && std::fabs(x - c) < 2.0 * s0);
            }
        }
    }

    // the cull against the exact test
    long accepted = 0, culled = 0;
    for (int t = 0; t < 20000; ++t) {
        const double box = std::ldexp(1.0 + uniform01(), 70 + (int)(next_bits() % 8)); // some 1e21 .. 1e23 cm
        double lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            const double p = uniform01(), w = (t % 3 == 0) ? 0.0 : uniform01() * 0.1;
            lo[a] = p; hi[a] = p + w;
        }
        ExpStar S;
        S.x = uniform01() * 1.2 - 0.1; S.y = uniform01() * 1.2 - 0.1; S.z = uniform01() * 1.2 - 0.1;
        if (t % 5 == 0) S.x = lo[0]; // on a face
        if (t % 7 == 0) { S.x = lo[0] + 0.5 * (hi[0] - lo[0]); S.y = lo[1]; S.z = hi[2]; } // inside
        for (int leaf = 0; leaf < 8; ++leaf) {
            // centres of the box: its corners, then points inside
            double c[3];
            for (int a = 0; a < 3; ++a) c[a] = leaf < 4 ? (((leaf >> a) & 1) ? hi[a] : lo[a]) : lo[a] + uniform01() * (hi[a] - lo[a]);
            for (int a = 0; a < 3; ++a) c[a] = c[a] < lo[a] ? lo[a] : c[a] > hi[a] ? hi[a] : c[a];
            const double dx = S.x - c[0], dy = S.y - c[1], dz = S.z - c[2];
            const double dist = box * expansion_sqrt(dx * dx + dy * dy + dz * dz);
            for (int k = -2; k <= 3; ++k) {
                // radii around this centre's distance: one and two ulps off on both sides, and far off
                double radius = dist;
                if (k == 3) radius = dist * (0.25 + 2.0 * uniform01());
                else for (int u = 0; u < (k < 0 ? -k : k); ++u) radius = std::nextafter(radius, k < 0 ? 0.0 : INFINITY);
                ExpStarTest T = {radius, 0.5, 1.0, 0.0};
                S.r2 = expansion_cull_r2(radius, box);
                const bool exact = expansion_accepts(S, T, c[0], c[1], c[2], 0.5, box);
                const bool reach = expansion_sphere_reaches_box(S, lo, hi);
                CHECK(exact == (dist < radius));
                CHECK(!exact || reach);
                accepted += exact;
                culled += !reach;
                CHECK(!expansion_accepts(S, T, c[0], c[1], c[2], 1.5, box)); // too dense
            }
        }
    }
    CHECK(accepted > 100000 && culled > 1000);
    std::printf("accepted %ld, culled %ld\nexpansion rules under the sanitizers: ok\n", accepted, culled);
    return 0;
}
