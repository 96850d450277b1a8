// ray_periodic_check.cpp -- the periodic ray walk of radiativetransfer_amd/csrc/ftte_ray_math.h evaluated on the host.  One source,
// two builds (tests/test_rays_periodic_host.py, tests/_rays_periodic.py), as ray_check.cpp is for the walk that ends at the box:
//   * a shared library without sanitizers: ryp_walk is the header's loop over periodic rays through a node array, which the Python
//     tests hold against the brute-force intersection over the box's images and the bitwise GPU tests compare with;
//   * with -DRAY_PERIODIC_CHECK_MAIN a program: a uniform 4^3 grid and one with a corner refined two levels, the named rays (the body
//     diagonal over two boxes both ways, a ray in a face plane and one along a box edge, origins on the box's face and corner moving
//     in and out, negative zeros, a tmax inside a leaf, on a box face and shorter than the first leaf, the six +-e_a over three
//     boxes, an origin 1 000 boxes away) and random ones; it checks that the segments tile [0, tmax], come in order with chords > 0
//     and name leaves of the grid, and that the axis rays repeat with equal bits; built with -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ftte_ray_math.h"

extern "C" {

long long ryp_step_bound(int n, int max_level, double tmax) { return ray_step_bound_periodic(n, max_level, tmax); }
int ryp_refusal(const double *o, const double *tmax, int n) { return ray_periodic_refusal(o, tmax, n); }

// the image and the local origin a periodic ray starts in
void ryp_image(int n, const double *o, const double *d, long long *w, double *local)
{
    ftte_ray R;
    ftte_ray_walk W;
    ftte_ray_image I;
    ray_begin_periodic(&R, &W, &I, n, o, d, 1.0);
    w[0] = I.wx; w[1] = I.wy; w[2] = I.wz;
    local[0] = R.ox; local[1] = R.oy; local[2] = R.oz;
}

// Ray r's segments go to offset[r] .. offset[r + 1] - 1 of leaf, t_in, t_out where capacity holds them all; the offsets and
// steps[r], the steps ray r's walk took, are written either way.  Every ray walks under its own bound.  Returns the number of
// segments, or -1 - r where ray r is refused or passed its step bound.
long long ryp_walk(int n, int max_level, const int32_t *nodes, long long nray, const double *origin, const double *dir, const double *tmax,
                   long long *offset, long long *steps, long long capacity, long long *leaf, double *t_in, double *t_out)
{
    const ftte_ray_node *node = reinterpret_cast<const ftte_ray_node *>(nodes);
    for (int pass = 0; pass < 2; ++pass) {
        long long at = 0;
        for (long long r = 0; r < nray; ++r) {
            if (ray_periodic_refusal(origin + 3 * r, tmax + r, n)) return -1 - r;
            const int64_t bound = ray_step_bound_periodic(n, max_level, tmax[r]);
            ftte_ray R;
            ftte_ray_walk W;
            ftte_ray_image I;
            ray_begin_periodic(&R, &W, &I, n, origin + 3 * r, dir + 3 * r, tmax[r]);
            if (pass == 0) offset[r] = at;
            int64_t count = 0;
            while (!W.done) {
                if (++count > bound || !ray_locate(&R, &W, n, node)) return -1 - r;
                double a = 0.0, b = 0.0;
                if (!ray_cross_periodic(&R, &W, &I, n, &a, &b)) continue;
                if (pass == 1) { leaf[at] = W.leaf; t_in[at] = a; t_out[at] = b; }
                ++at;
            }
            if (pass == 0 && steps) steps[r] = count;
        }
        if (pass == 0) {
            offset[nray] = at;
            if (at > capacity || at == 0) return at;
        }
    }
    return offset[nray];
}

} // extern "C"

#ifdef RAY_PERIODIC_CHECK_MAIN
namespace {

int failures = 0;

void expect(bool ok, const char *what, long long at, double a, double b)
{
    if (ok) return;
    if (++failures <= 20) std::printf("FAILED %s: at %lld, %.17g vs %.17g\n", what, at, a, b);
}

struct Lcg { // (no <random>: the same rays everywhere)
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1p-53; }
    double between(double a, double b) { return a + (b - a) * next(); }
};

struct Grid {
    int n = 0, max_level = 0;
    long long ncell = 0;
    std::vector<int32_t> nodes; // {child0, leaf, parent, level} records; empty: uniform
};

// base cells in storage order; base cell 0 refined `depth` levels, always the first child again; leaves numbered depth first
Grid corner_grid(int n, int depth)
{
    Grid G;
    G.n = n; G.max_level = depth;
    const int nbase = n * n * n;
    if (!depth) { G.ncell = nbase; return G; }
    std::vector<int32_t> child0((size_t)nbase, -1), leaf((size_t)nbase, -1);
    int at = 0;
    for (int d = 0; d < depth; ++d) {
        child0[(size_t)at] = (int32_t)child0.size();
        for (int q = 0; q < 8; ++q) { child0.push_back(-1); leaf.push_back(-1); }
        at = child0[(size_t)at];
    }
    int32_t cursor = 0;
    for (int d = depth; d >= 1; --d) {
        int node = 0;
        for (int q = 0; q < d - 1; ++q) node = child0[(size_t)node];
        const int first = child0[(size_t)node];
        for (int q = (d == depth ? 0 : 1); q < 8; ++q) leaf[(size_t)(first + q)] = cursor++;
    }
    for (int b = 1; b < nbase; ++b) leaf[(size_t)b] = cursor++;
    G.ncell = cursor;
    for (size_t v = 0; v < child0.size(); ++v) { G.nodes.push_back(child0[v]); G.nodes.push_back(leaf[v]); G.nodes.push_back(-1); G.nodes.push_back(0); }
    return G;
}

struct Lists {
    std::vector<long long> off, leaf, steps;
    std::vector<double> a, b;
};

Lists walk_and_check(const Grid &G, const std::vector<double> &o, const std::vector<double> &d, const std::vector<double> &tmax, long long *segments)
{
    Lists L;
    const long long nray = (long long)tmax.size();
    L.off.resize((size_t)nray + 1); L.steps.resize((size_t)nray);
    const int32_t *nodes = G.nodes.empty() ? nullptr : G.nodes.data();
    const long long total = ryp_walk(G.n, G.max_level, nodes, nray, o.data(), d.data(), tmax.data(), L.off.data(), L.steps.data(), 0, nullptr, nullptr, nullptr);
    expect(total > 0, "no walk refused or beyond its bound", total, 0, 0);
    if (total <= 0) return L;
    L.leaf.resize((size_t)total); L.a.resize((size_t)total); L.b.resize((size_t)total);
    const long long again = ryp_walk(G.n, G.max_level, nodes, nray, o.data(), d.data(), tmax.data(), L.off.data(), L.steps.data(), total, L.leaf.data(), L.a.data(), L.b.data());
    expect(again == total, "the second pass counts the same", again, (double)total, 0);
    for (long long r = 0; r < nray; ++r) {
        const double tol = 1e-12 * (tmax[(size_t)r] + G.n);
        double sum = 0.0, t = 0.0;
        expect(L.off[(size_t)r + 1] > L.off[(size_t)r], "a periodic ray always hits", r, 0, 0);
        for (long long q = L.off[(size_t)r]; q < L.off[(size_t)r + 1]; ++q) {
            expect(L.leaf[(size_t)q] >= 0 && L.leaf[(size_t)q] < G.ncell, "a leaf of the grid", q, (double)L.leaf[(size_t)q], (double)G.ncell);
            expect(L.a[(size_t)q] == t, "a segment starts where the last one ended", q, L.a[(size_t)q], t);
            expect(L.b[(size_t)q] > L.a[(size_t)q], "a chord above 0", q, L.a[(size_t)q], L.b[(size_t)q]);
            t = L.b[(size_t)q];
            sum += L.b[(size_t)q] - L.a[(size_t)q];
        }
        expect(t == tmax[(size_t)r], "the last segment ends at tmax", r, t, tmax[(size_t)r]);
        expect(std::fabs(sum - tmax[(size_t)r]) <= tol, "the chords add up", r, sum, tmax[(size_t)r]);
        expect(L.steps[(size_t)r] <= ray_step_bound_periodic(G.n, G.max_level, tmax[(size_t)r]), "inside the bound", r, (double)L.steps[(size_t)r], 0);
    }
    *segments += total;
    return L;
}

} // namespace

int main()
{
    long long segments = 0, rays = 0;
    const double r3 = 1.0 / std::sqrt(3.0), r2 = 1.0 / std::sqrt(2.0);
    for (int depth : {0, 2}) {
        const Grid G = corner_grid(4, depth);
        const double n = 4.0;
        std::vector<double> o, d, tmax;
        auto ray = [&](double ox, double oy, double oz, double dx, double dy, double dz, double tm) {
            for (double v : {ox, oy, oz}) o.push_back(v);
            for (double v : {dx, dy, dz}) d.push_back(v);
            tmax.push_back(tm);
        };
        for (int a = 0; a < 3; ++a) // rays 0 .. 5: +-e_a over three boxes from a base cell's face
            for (double sign : {1.0, -1.0}) ray(a == 0 ? 2.0 - 3.0 * sign : 0.125, a == 1 ? 2.0 - 3.0 * sign : 0.625, a == 2 ? 2.0 - 3.0 * sign : 3.5, a == 0 ? sign : 0.0, a == 1 ? sign : 0.0, a == 2 ? sign : 0.0, 3.0 * n);
        ray(0, 0, 0, r3, r3, r3, (2.0 * n) * (1.0 / r3));       // the body diagonal over two boxes
        ray(n, n, n, -r3, -r3, -r3, (2.0 * n) * (1.0 / r3));    // and the other way
        ray(0.1, 2.0, 0.3, r2, 0.0, r2, 3.3 * n);               // in a face plane between cells
        ray(0.0, 0.0, 0.5, 0.0, 0.0, 1.0, 2.5 * n);             // along a box edge
        ray(n, n, 1.5, 0.0, 0.0, -1.0, 2.5 * n);                // along the opposite one
        ray(n, 0.5, 0.5, 1.0, 0.0, 0.0, 1.5 * n);               // on the box's face, outwards
        ray(n, 0.5, 0.5, -1.0, 0.0, 0.0, 1.5 * n);              // and inwards
        ray(n, n, n, r3, r3, r3, 5.0);                          // on the corner, outwards
        ray(0, 0, 0, -r3, -r3, -r3, 5.0);                       // on the opposite corner, outwards
        ray(0.5, 0.5, n, -0.0, -0.0, -1.0, 2.0 * n);            // negative zeros
        ray(-0.0, 0.5, 0.5, -1.0, -0.0, 0.0, 2.0 * n);          // a negative zero for an origin
        ray(0.3, 0.2, 0.1, r3, r3, r3, 9.7);                    // a tmax inside a leaf
        ray(0.5, 0.5, 0.0, 0.0, 0.0, 1.0, 2.0 * n);             // a tmax on a box face
        ray(0.3, 0.2, 0.1, r3, r3, r3, 0.01);                   // a tmax shorter than the first leaf
        ray(1000.0 * n + 0.5, -1000.0 * n + 0.25, 0.3, r3, -r3, r3, 3.0 * n);  // 1 000 boxes away, o' exact
        ray(1000.0 * n + 0.3, -1000.0 * n + 0.6, -0.45, -r3, r3, r3, 3.0 * n);  // o' rounded
        Lcg r{20261021ull + (uint64_t)depth};
        for (int q = 0; q < 2000; ++q) {
            double v[3], norm = 0.0;
            for (double &c : v) { c = r.between(-1.0, 1.0); norm += c * c; }
            if (norm < 1e-3) continue;
            if (q % 10 == 0) { norm -= v[q / 10 % 3] * v[q / 10 % 3]; v[q / 10 % 3] = 0.0; }
            norm = std::sqrt(norm);
            ray(r.between(-n, 2.0 * n), r.between(-n, 2.0 * n), r.between(-n, 2.0 * n), v[0] / norm, v[1] / norm, v[2] / norm, r.between(0.01, 5.0 * n));
        }
        for (size_t q = 0; q < tmax.size(); ++q)
            expect(ray_arguments_ok(&o[3 * q], &d[3 * q], &tmax[q]) == 1 && !ray_periodic_refusal(&o[3 * q], &tmax[q], G.n), "a good ray", (long long)q, 0, 0);
        const Lists L = walk_and_check(G, o, d, tmax, &segments);
        rays += (long long)tmax.size();
        if (L.leaf.empty()) continue;
        for (long long q = 0; q < 6; ++q) { // three copies of the first box's list, t shifted by exactly j n
            const long long first = L.off[(size_t)q], m = L.off[(size_t)q + 1] - first;
            expect(m % 3 == 0 && m >= 12, "an axis ray over three boxes", q, (double)m, 0);
            for (long long s = 0; m % 3 == 0 && s < m; ++s) {
                const long long base = first + s % (m / 3);
                const double shift = (double)(s / (m / 3)) * n;
                expect(L.leaf[(size_t)(first + s)] == L.leaf[(size_t)base] && L.a[(size_t)(first + s)] == L.a[(size_t)base] + shift && L.b[(size_t)(first + s)] == L.b[(size_t)base] + shift,
                       "the one-box list again", first + s, L.a[(size_t)(first + s)], L.a[(size_t)base] + shift);
            }
        }
    }
    const double good[3] = {0.5, 0.5, 0.5}, away[3] = {0.5, 0x1p23, 0.5}, zero = 0.0, one = 1.0;
    expect(ray_periodic_refusal(good, nullptr, 4) == 1 && ray_periodic_refusal(good, &zero, 4) == 1 && ray_periodic_refusal(away, &one, 4) == 2 && !ray_periodic_refusal(good, &one, 4),
           "the refusals", 0, 0, 0);
    expect(ray_step_bound_periodic(4, 0, 4.0) == 27 && ray_step_bound_periodic(4, 41, 4.0) == 0 && ray_step_bound_periodic(4, 0, 4.0 * 0x1p20 + 1.0) == 0 &&
               ray_step_bound_periodic(1 << 20, 40, 4.0) == 0, "the bound", 0, 0, 0);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("periodic ray walk under the sanitizers: ok (%lld rays, %lld segments)\n", rays, segments);
    return 0;
}
#endif
