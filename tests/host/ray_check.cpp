// ray_check.cpp -- the ray walk of radiativetransfer_amd/csrc/ftte_ray_math.h evaluated on the host.  One source, two builds
// (tests/test_rays_host.py, tests/_rays.py):
//   * a shared library without sanitizers: ry_walk is the header's loop over rays through a node array (the nodes of
//     tests/_analysis.Tree as {child0, leaf, parent, level} records, or none for a uniform grid), which is what the Python tests
//     hold against the brute-force intersection and the bitwise GPU tests compare with; ry_line_inputs what a segment gives the line;
//   * with -DRAY_CHECK_MAIN a program: it builds a uniform 4^3 grid and one with a corner refined two levels, walks the named rays
//     (the body diagonal, a ray in a face plane, one along an edge, one that misses, a tmax inside a leaf, an origin in a deepest
//     leaf, negative zeros, the six +-e_a) and random ones, and checks that the segments tile [t_start, t_end], come in order with
//     chords > 0 and name leaves of the grid; built with -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ftte_ray_math.h"

extern "C" {

int ry_arguments_ok(const double *o, const double *d, const double *tmax) { return ray_arguments_ok(o, d, tmax); }
long long ry_step_bound(int n, int max_level) { return ray_step_bound(n, max_level); }

// the exit axis of the first leaf a ray is in (-1: it misses), and that leaf's t_out
int ry_first_exit(int n, const int32_t *nodes, const double *o, const double *d, double *t_out)
{
    ftte_ray R;
    ftte_ray_walk W;
    ray_begin(&R, &W, n, o, d, 0.0);
    if (W.done || !ray_locate(&R, &W, n, reinterpret_cast<const ftte_ray_node *>(nodes))) return -1;
    int axis = -1;
    *t_out = ray_exit(&R, &W, &axis);
    return axis;
}

// start[2 nray]: t_start, t_end of every ray (both 0 for a miss).  Ray r's segments go to offset[r] .. offset[r + 1] - 1 of leaf,
// t_in, t_out where capacity holds them all; the offsets are written either way.  Returns the number of segments, or -1 - r where
// ray r passed the step bound.
long long ry_walk(int n, int max_level, const int32_t *nodes, long long nray, const double *origin, const double *dir, const double *tmax,
                  long long *offset, double *start, long long capacity, long long *leaf, double *t_in, double *t_out)
{
    const ftte_ray_node *node = reinterpret_cast<const ftte_ray_node *>(nodes);
    const int64_t bound = ray_step_bound(n, max_level);
    for (int pass = 0; pass < 2; ++pass) {
        long long at = 0;
        for (long long r = 0; r < nray; ++r) {
            ftte_ray R;
            ftte_ray_walk W;
            ray_begin(&R, &W, n, origin + 3 * r, dir + 3 * r, tmax ? tmax[r] : 0.0);
            if (pass == 0) {
                offset[r] = at;
                if (start) { start[2 * r] = R.hit ? R.t_start : 0.0; start[2 * r + 1] = R.hit ? R.t_end : 0.0; }
            }
            int64_t steps = 0;
            while (!W.done) {
                if (++steps > bound || !ray_locate(&R, &W, n, node)) return -1 - r;
                double a = 0.0, b = 0.0;
                if (!ray_cross(&R, &W, n, &a, &b)) continue;
                if (pass == 1) { leaf[at] = W.leaf; t_in[at] = a; t_out[at] = b; }
                ++at;
            }
        }
        if (pass == 0) {
            offset[nray] = at;
            if (at > capacity || at == 0) return at;
        }
    }
    return offset[nray];
}

// per segment of ray r (offset as above): size = chord cell_cm, s = midpoint cell_cm, u = d . v of the leaf (vel: three arrays per
// leaf, or NULL for 0)
void ry_line_inputs(long long nray, const double *origin, const double *dir, int n, const long long *offset, const long long *leaf, const double *t_in,
                    const double *t_out, double cell_cm, const double *vx, const double *vy, const double *vz, double *size, double *s, double *u)
{
    for (long long r = 0; r < nray; ++r) {
        ftte_ray R;
        ftte_ray_walk W;
        ray_begin(&R, &W, n, origin + 3 * r, dir + 3 * r, 0.0);
        for (long long q = offset[r]; q < offset[r + 1]; ++q) {
            size[q] = (t_out[q] - t_in[q]) * cell_cm;
            s[q] = ray_segment_s(t_in[q], t_out[q]) * cell_cm;
            u[q] = vx ? ray_segment_u(&R, vx[leaf[q]], vy[leaf[q]], vz[leaf[q]]) : 0.0;
        }
    }
}

} // extern "C"

#ifdef RAY_CHECK_MAIN
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
    std::vector<int32_t> nodes; // empty: uniform
};

// base cells in storage order; base cell 0 refined `depth` levels, always the first child again
Grid corner_grid(int n, int depth)
{
    Grid G;
    G.n = n; G.max_level = depth;
    const int nbase = n * n * n;
    if (!depth) { G.ncell = nbase; return G; }
    std::vector<int32_t> child0((size_t)nbase, -1), leaf((size_t)nbase, -1);
    int32_t cursor = 0;
    int at = 0;
    for (int d = 0; d < depth; ++d) { // the refined chain comes first in the depth-first leaf order
        child0[(size_t)at] = (int32_t)child0.size();
        for (int q = 0; q < 8; ++q) { child0.push_back(-1); leaf.push_back(-1); }
        at = child0[(size_t)at];
    }
    // leaves depth first: the deepest children, then the siblings of every level going up
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

void walk_and_check(const Grid &G, const std::vector<double> &o, const std::vector<double> &d, const std::vector<double> &tmax, long long *segments)
{
    const long long nray = (long long)o.size() / 3;
    std::vector<long long> off((size_t)nray + 1), leaf;
    std::vector<double> start((size_t)nray * 2), a, b;
    const int32_t *nodes = G.nodes.empty() ? nullptr : G.nodes.data();
    long long total = ry_walk(G.n, G.max_level, nodes, nray, o.data(), d.data(), tmax.data(), off.data(), start.data(), 0, nullptr, nullptr, nullptr);
    expect(total >= 0, "no walk beyond its bound", total, 0, 0);
    if (total < 0) return;
    leaf.resize((size_t)total + 1); a.resize((size_t)total + 1); b.resize((size_t)total + 1);
    const long long again = ry_walk(G.n, G.max_level, nodes, nray, o.data(), d.data(), tmax.data(), off.data(), start.data(), total, leaf.data(), a.data(), b.data());
    expect(again == total, "the second pass counts the same", again, (double)total, 0);
    const double tol = 1e-12 * G.n;
    for (long long r = 0; r < nray; ++r) {
        double sum = 0.0, t = start[(size_t)(2 * r)];
        for (long long q = off[(size_t)r]; q < off[(size_t)r + 1]; ++q) {
            expect(leaf[(size_t)q] >= 0 && leaf[(size_t)q] < G.ncell, "a leaf of the grid", q, (double)leaf[(size_t)q], (double)G.ncell);
            expect(a[(size_t)q] == t, "a segment starts where the last one ended", q, a[(size_t)q], t);
            expect(b[(size_t)q] > a[(size_t)q], "a chord above 0", q, a[(size_t)q], b[(size_t)q]);
            t = b[(size_t)q];
            sum += b[(size_t)q] - a[(size_t)q];
        }
        expect(t == start[(size_t)(2 * r + 1)] || off[(size_t)r] == off[(size_t)r + 1], "the last segment ends at t_end", r, t, start[(size_t)(2 * r + 1)]);
        expect(std::fabs(sum - (start[(size_t)(2 * r + 1)] - start[(size_t)(2 * r)])) <= tol, "the chords add up", r, sum, start[(size_t)(2 * r + 1)] - start[(size_t)(2 * r)]);
    }
    *segments += total;
}

} // namespace

int main()
{
    long long segments = 0, rays = 0;
    const double r3 = 1.0 / std::sqrt(3.0), r2 = 1.0 / std::sqrt(2.0);
    for (int depth : {0, 2}) {
        const Grid G = corner_grid(4, depth);
        std::vector<double> o, d, tmax;
        auto ray = [&](double ox, double oy, double oz, double dx, double dy, double dz, double tm) {
            for (double v : {ox, oy, oz}) o.push_back(v);
            for (double v : {dx, dy, dz}) d.push_back(v);
            tmax.push_back(tm);
        };
        ray(0, 0, 0, r3, r3, r3, 0);                 // the body diagonal: three-way ties
        ray(0.1, 2.0, 0.3, r2, 0.0, r2, 0);          // in a face plane between cells
        ray(1.0, 2.0, -1.0, 0.0, 0.0, 1.0, 0);       // along an edge
        ray(-1.0, 5.0, 0.5, 1.0, 0.0, 0.0, 0);       // misses
        ray(9.0, 9.0, 9.0, r3, r3, r3, 0);           // points away
        ray(0.3, 0.2, 0.1, r3, r3, r3, 1.7);         // a tmax inside a leaf
        ray(0.01, 0.02, 0.03, -r3, r3, -r3, 0);      // an origin inside a deepest leaf
        ray(0.5, 0.5, 4.0, -0.0, -0.0, -1.0, 0);     // negative zeros
        ray(4.0, 0.5, 0.5, 1.0, 0.0, 0.0, 0);        // on the far face, outwards
        for (int a = 0; a < 3; ++a)
            for (double sign : {1.0, -1.0}) ray(a == 0 ? 2.0 - 3.0 * sign : 0.125, a == 1 ? 2.0 - 3.0 * sign : 0.625, a == 2 ? 2.0 - 3.0 * sign : 3.5, a == 0 ? sign : 0.0, a == 1 ? sign : 0.0, a == 2 ? sign : 0.0, 0);
        Lcg r{20261021ull + (uint64_t)depth};
        for (int q = 0; q < 2000; ++q) {
            double v[3], norm = 0.0;
            for (double &c : v) { c = r.between(-1.0, 1.0); norm += c * c; }
            if (norm < 1e-3) continue;
            norm = std::sqrt(norm);
            ray(r.between(-2.0, 6.0), r.between(-2.0, 6.0), r.between(-2.0, 6.0), v[0] / norm, v[1] / norm, v[2] / norm, q % 5 ? 0.0 : r.between(0.0, 6.0));
        }
        for (size_t q = 0; q < tmax.size(); ++q) expect(ray_arguments_ok(&o[3 * q], &d[3 * q], &tmax[q]) == 1, "a good ray", (long long)q, 0, 0);
        walk_and_check(G, o, d, tmax, &segments);
        rays += (long long)tmax.size();
    }
    const double nan = std::nan(""), good[3] = {0.0, 0.0, 1.0}, bad[3] = {0.0, 0.1, 1.0}, inf[3] = {INFINITY, 0.0, 0.0};
    expect(!ray_arguments_ok(good, bad, nullptr) && !ray_arguments_ok(inf, good, nullptr) && !ray_arguments_ok(good, good, &nan) && ray_arguments_ok(good, good, nullptr),
           "the refusals", 0, 0, 0);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ray walk under the sanitizers: ok (%lld rays, %lld segments)\n", rays, segments);
    return 0;
}
#endif
