// The host-testable rules of the star catalogue (radiativetransfer_amd/csrc/ftte_catalogue.h) and its owner
// (ftte_star_catalogue.h, against the stub of the HIP runtime) under the address and undefined-behaviour sanitizers: the unit-cube
// coordinate, the base index with its range test in front of the conversion, the descent through a hand-built tree of three
// levels, faces and midplanes, -0.0, nextafter(1, 0), 1.0, NaN, infinities and values beyond 2^31, the location key with a
// colliding pair of leaves, the metallicity bracket and the population slots.
//
// With two arguments (a case file as tests/golden/make_golden_catalogue.py writes it, an output file) it locates the stars of the
// case instead and writes per star the host leaf, its level and its location key as int64: tests/test_star_catalogue_host.py
// compares them with the reference's.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ftte_catalogue.h"
#include "ftte_gas.h"
#include "ftte_star_catalogue.h"

using namespace ftte;

#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::fprintf(stderr, "ERROR %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); }       \
    } while (0)

struct Node { int32_t child0, leaf; };

// the tree of a depth-first level list, numbered as AmrTree::build numbers it
static std::vector<Node> build(int n, const std::vector<int32_t> &level)
{
    std::vector<Node> node((size_t)n * n * n, Node{-1, -1});
    size_t cursor = 0;
    struct Rec {
        static void grow(std::vector<Node> &node, const std::vector<int32_t> &level, size_t &cursor, int32_t at, int depth)
        {
            CHECK(cursor < level.size());
            if (level[cursor] == depth) { node[(size_t)at].leaf = (int32_t)cursor++; return; }
            CHECK(level[cursor] > depth);
            const int32_t c0 = (int32_t)node.size();
            node[(size_t)at].child0 = c0;
            node.resize(node.size() + 8, Node{-1, -1});
            for (int c = 0; c < 8; ++c) grow(node, level, cursor, c0 + c, depth + 1);
        }
    };
    for (int32_t b = 0; b < n * n * n; ++b) Rec::grow(node, level, cursor, b, 0);
    CHECK(cursor == level.size());
    return node;
}

static LeafPos position_of(const std::vector<Node> &node, int n, double x, double y, double z, int64_t *leaf)
{
    LeafPos P;
    std::memset(&P, 0, sizeof P);
    int i, j, k;
    double r;
    *leaf = catalogue_leaf(node.data(), n, x, y, z, &P.depth, P.path);
    if (*leaf >= 0 && catalogue_base(x, n, &i, &r) && catalogue_base(y, n, &j, &r) && catalogue_base(z, n, &k, &r)) P.base = (i * n + j) * n + k;
    return P;
}

static int run_case(const char *in, const char *out)
{
    std::FILE *f = std::fopen(in, "rb");
    CHECK(f);
    int32_t head[3];
    double lo[3], hi[3];
    CHECK(std::fread(head, sizeof(int32_t), 3, f) == 3 && std::fread(lo, 8, 3, f) == 3 && std::fread(hi, 8, 3, f) == 3);
    const int n = head[0];
    const size_t ncell = (size_t)head[1], ns = (size_t)head[2];
    std::vector<int32_t> level(ncell);
    std::vector<double> abun2(ncell), xyz(3 * ns);
    CHECK(std::fread(level.data(), 4, ncell, f) == ncell && std::fread(abun2.data(), 8, ncell, f) == ncell);
    CHECK(std::fread(xyz.data(), 8, 3 * ns, f) == 3 * ns);
    std::fclose(f);
    const std::vector<Node> node = build(n, level);
    std::vector<int64_t> res(3 * ns);
    for (size_t s = 0; s < ns; ++s) {
        const double x = catalogue_unit(xyz[3 * s], lo[0], hi[0]), y = catalogue_unit(xyz[3 * s + 1], lo[1], hi[1]),
                     z = catalogue_unit(xyz[3 * s + 2], lo[2], hi[2]);
        int64_t leaf;
        const LeafPos P = position_of(node, n, x, y, z, &leaf);
        res[s] = leaf;
        res[ns + s] = leaf < 0 ? -1 : P.depth;
        res[2 * ns + s] = leaf < 0 ? -1 : catalogue_location_key(P);
    }
    f = std::fopen(out, "wb");
    CHECK(f && std::fwrite(res.data(), 8, res.size(), f) == res.size());
    std::fclose(f);
    std::printf("star catalogue case: ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3) return run_case(argv[1], argv[2]);

    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double last = std::nextafter(1.0, 0.0);

    // the unit-cube coordinate: plain IEEE operations
    CHECK(catalogue_unit(3.0, 1.0, 5.0) == 0.5 && catalogue_unit(1.0, 1.0, 5.0) == 0.0 && catalogue_unit(5.0, 1.0, 5.0) == 1.0);
    CHECK(catalogue_unit(0.1, 0.0, 0.3) == 0.1 / 0.3);

    // the base index: the range test comes first
    int i = -7;
    double r = -7.0;
    const int sizes[] = {1, 2, 6, 12, 16, 1290, 32000};
    for (int n : sizes) {
        CHECK(catalogue_base(0.0, n, &i, &r) && i == 0 && r == 0.0);
        CHECK(catalogue_base(-0.0, n, &i, &r) && i == 0 && r == 0.0);
        CHECK(catalogue_base(last, n, &i, &r) && i == n - 1 && r <= 1.0);
        CHECK(!catalogue_base(1.0, n, &i, &r) && !catalogue_base(1.5, n, &i, &r) && !catalogue_base(-1.0, n, &i, &r));
        CHECK(!catalogue_base(nan, n, &i, &r) && !catalogue_base(inf, n, &i, &r) && !catalogue_base(-inf, n, &i, &r));
        CHECK(!catalogue_base(1.0e300, n, &i, &r) && !catalogue_base(-1.0e300, n, &i, &r) && !catalogue_base(3.0e9, n, &i, &r));
        CHECK(!catalogue_base(-2147483649.0 / n, n, &i, &r) && !catalogue_base(2147483648.0, n, &i, &r));
        for (int c = 0; c < n && c < 40; ++c) {
            const double x = (double)c / (double)n; // a face: the upper cell, where x * n rounds to c
            if (x * (double)n == (double)c) CHECK(catalogue_base(x, n, &i, &r) && i == c && r == 0.0);
        }
    }
    // int() truncates, as the reference's: -1/n < x < 0 stays in cell 0 with a negative remainder
    CHECK(catalogue_base(-0.01, 16, &i, &r) && i == 0 && r == -0.01 * 16.0);
    CHECK(!catalogue_base(-0.0625, 16, &i, &r));

    // the descent: upper where >= 0.5
    double p[3] = {0.5, 0.49999999999999994, 0.75};
    CHECK(catalogue_descend(p) == 4 + 0 + 1 && p[0] == 0.0 && p[1] == 0.9999999999999999 && p[2] == 0.5);
    CHECK(catalogue_descend(p) == 0 + 2 + 1 && p[0] == 0.0 && p[2] == 0.0);

    // three levels by hand: 2^3 base cells; base cell 3 = (0, 1, 1) refined, its child 5 = (1, 0, 1) refined again
    std::vector<int32_t> level = {0, 0, 0};
    for (int c = 0; c < 8; ++c) {
        if (c == 5) for (int d = 0; d < 8; ++d) level.push_back(2);
        else level.push_back(1);
    }
    for (int c = 4; c < 8; ++c) level.push_back(0);
    const std::vector<Node> node = build(2, level);
    CHECK(node.size() == 8 + 16 && level.size() == 3 + 7 + 8 + 4);
    CHECK(node[3].child0 == 8 && node[8 + 5].child0 == 16 && node[16].leaf == 8 && node[7].leaf == 21);
    int depth = -1;
    // base leaves
    CHECK(catalogue_leaf(node.data(), 2, 0.1, 0.2, 0.3, &depth) == 0 && depth == 0);
    CHECK(catalogue_leaf(node.data(), 2, 0.75, 0.75, 0.75, &depth) == 21 && depth == 0);
    CHECK(catalogue_leaf(node.data(), 2, 0.5, 0.0, 0.0) == 18); // on the face: base cell (1, 0, 0), the fifth base cell
    // base cell 3 spans x [0, .5), y [.5, 1), z [.5, 1); its children are a quarter wide
    CHECK(catalogue_leaf(node.data(), 2, 0.1, 0.6, 0.6, &depth) == 3 && depth == 1);              // child 0
    CHECK(catalogue_leaf(node.data(), 2, 0.25, 0.75, 0.75, &depth) == 3 + 7 + 8 - 1 + 0 && depth == 1); // midplanes: child 7, the last one
    // child 5 = upper x, lower y, upper z: x [.25, .5), y [.5, .75), z [.75, 1); its children an eighth wide
    LeafPos P;
    std::memset(&P, 0, sizeof P);
    CHECK(catalogue_leaf(node.data(), 2, 0.26, 0.51, 0.76, &P.depth, P.path) == 8 && P.depth == 2 && P.path[0] == (5u | 0u << 3));
    std::memset(&P, 0, sizeof P);
    CHECK(catalogue_leaf(node.data(), 2, 0.375, 0.625, 0.875, &P.depth, P.path) == 15 && P.path[0] == (5u | 7u << 3)); // midplanes again
    CHECK(catalogue_leaf(node.data(), 2, 0.375, 0.6, 0.8) == 8 + 4);
    // the last leaf and the outside
    CHECK(catalogue_leaf(node.data(), 2, last, last, last) == 21 && catalogue_leaf(node.data(), 2, -0.0, -0.0, -0.0) == 0);
    CHECK(catalogue_leaf(node.data(), 2, 1.0, 0.5, 0.5) == -1 && catalogue_leaf(node.data(), 2, 0.5, nan, 0.5) == -1);
    CHECK(catalogue_leaf(node.data(), 2, 0.5, 0.5, -inf) == -1 && catalogue_leaf(node.data(), 2, -0.6, 0.5, 0.5) == -1);
    // a uniform grid: the leaf is the base index
    CHECK(catalogue_leaf((const Node *)nullptr, 16, 5.5 / 16, 9.0 / 16, last, &depth) == (5 * 16 + 9) * 16 + 15 && depth == 0);

    // the location key: base index + 1, then a digit 1..8 per level; base cell 10 b + d and child d of base cell b collide
    P.base = 3; P.depth = 2; P.path[0] = 5u | 7u << 3;
    CHECK(catalogue_location_key(P) == (4 * 10 + 6) * 10 + 8);
    LeafPos A, B;
    std::memset(&A, 0, sizeof A);
    std::memset(&B, 0, sizeof B);
    A.base = 34; A.depth = 1; A.path[0] = 2;      // key 10 * 35 + 3
    B.base = 352;                                  // key 353
    CHECK(catalogue_location_key(A) == 353 && catalogue_location_key(B) == 353);

    // the bracket, :1282-1293
    const double met[5] = {-3.0, -2.0, -1.5, -1.0, 0.0};
    int32_t im = 0;
    double cm = -1.0;
    catalogue_metal_bracket(0.0, 5, met, &im, &cm);     CHECK(im == 1 && cm == 0.0);       // below 1e-20: -20
    catalogue_metal_bracket(1.0e-21, 5, met, &im, &cm); CHECK(im == 1 && cm == 0.0);
    catalogue_metal_bracket(nan, 5, met, &im, &cm);     CHECK(im == 1 && cm == 0.0);
    catalogue_metal_bracket(1.0e-4, 5, met, &im, &cm);  CHECK(im == 1 && cm == 0.0);       // below the grid
    catalogue_metal_bracket(std::pow(10.0, -2.5), 5, met, &im, &cm); CHECK(im == 1 && cm == (std::log10(std::pow(10.0, -2.5)) + 3.0) / 1.0);
    catalogue_metal_bracket(0.02, 5, met, &im, &cm);    CHECK(im == 2 && cm == (std::log10(0.02) + 2.0) / 0.5);
    catalogue_metal_bracket(0.05, 5, met, &im, &cm);    CHECK(im == 3 && cm > 0.0 && cm < 1.0);
    catalogue_metal_bracket(0.5, 5, met, &im, &cm);     CHECK(im == 4 && cm == (std::log10(0.5) + 1.0) / 1.0);
    catalogue_metal_bracket(7.0, 5, met, &im, &cm);     CHECK(im == 4 && cm == 1.0);       // beyond the grid
    const double met10[3] = {0.0, 2.0, 3.0};
    catalogue_metal_bracket(100.0, 3, met10, &im, &cm); CHECK(im == 1 && cm == 1.0);       // on a node: the interval below
    catalogue_metal_bracket(7.0, 2, met, &im, &cm);     CHECK(im == 1 && cm == 1.0);       // two nodes: never past nmetal - 1
    catalogue_metal_bracket(2.0e-2, 3, met, &im, &cm);  CHECK(im == 2 && cm > 0.0 && cm < 1.0);
    // the float32 literal 1.e-20 widened lies below 1e-20: a value between the two is above the threshold
    CHECK((double)1.e-20f < 1.0e-20);
    catalogue_metal_bracket(1.0e-20, 5, met, &im, &cm); CHECK(im == 1 && cm == 0.0);

    // the slots: one per distinct pair, in order of first appearance
    const int32_t ims[7] = {2, 1, 2, 2, 1, 4, 1};
    const double cms[7] = {0.25, 0.0, 0.25, 0.5, 0.0, 1.0, std::nextafter(0.0, 1.0)};
    int32_t slot[7];
    int64_t first[7];
    CHECK(catalogue_slots(7, ims, cms, slot, first) == 5);
    const int32_t want_slot[7] = {0, 1, 0, 2, 1, 3, 4};
    const int64_t want_first[5] = {0, 1, 3, 5, 6};
    CHECK(!std::memcmp(slot, want_slot, sizeof want_slot) && !std::memcmp(first, want_first, sizeof want_first));
    CHECK(catalogue_slots(0, ims, cms, slot, nullptr) == 0);
    const int32_t one[4] = {1, 1, 1, 1};
    const double zero[4] = {0.0, 0.0, 0.0, 0.0};
    CHECK(catalogue_slots(4, one, zero, slot, first) == 1 && slot[3] == 0 && first[0] == 0);

    // the owner: a catalogue is there once made, gone with the grid; the gas knows whether it came with an abun2
    {
        StarCatalogue K;
        CHECK(K.sources() == -1 && K.stars() == 0);
        CHECK(K.count.reserve(100) == hipSuccess && K.src_cell.reserve(10) == hipSuccess);
        K.begin();
        K.made(50, 10);
        CHECK(K.sources() == 10 && K.stars() == 50);
        K.begin();
        CHECK(K.sources() == -1);
        K.made(0, 0);
        CHECK(K.sources() == 0);
        AmrTree T;
        T.n = 2; T.ncell = (int64_t)level.size(); T.max_level = 2;
        for (const Node &v : node) { T.child0.push_back(v.child0); T.leaf.push_back(v.leaf); }
        const std::vector<int32_t> &ln = K.leaf_nodes(T);
        CHECK(ln.size() == level.size() && ln[0] == 0 && ln[3] == 8 && ln[8] == 16 && ln[21] == 7);
        K.drop_grid();
        CHECK(K.sources() == -1 && !K.count.get() && !K.src_cell.get());
        GasState G;
        CHECK(G.reserve(10) == hipSuccess);
        G.filled(10, 0, true);
        CHECK(G.ready(10) && !G.ready_with_abundance(10));
        G.filled(10, 1, true, true);
        CHECK(G.ready_with_abundance(10) && !G.ready_with_abundance(11));
        G.drop();
        CHECK(!G.ready_with_abundance(10));
    }
    CHECK(g_device_objects.load() == 0);

    std::printf("star catalogue rules under the sanitizers: ok\n");
    return 0;
}
