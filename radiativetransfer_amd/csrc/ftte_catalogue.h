// ftte_catalogue.h -- the star catalogue (equiSources.f90:746-769: star coordinates -> unit cube -> localizeSplitContinuationCell
// :3049-3118 -> host leaf; :1169-1212: stars of one host cell merged into one source; :1282-1293: the metallicity bracket of a
// source): the records the kernels of ftte_catalogue.hip read, and the rules the host and the device share -- the unit-cube
// coordinate, the base index with its range test, the descent, the reference's location key, the bracket and the population slots.
// Needs nothing of the HIP runtime, so that the rules can be compiled and checked on their own (tests/host/star_catalogue_check.cpp).
//
// Stars are merged by HOST LEAF, which is what the reference's comment says it does.  Its key (location = 10 location + digit per
// level on top of the base index) is not injective -- base cell 10 b + d, unrefined, and child d of base cell b share one -- so on
// some trees the reference merges stars of two leaves; which one survives depends on an unstable heapsort.  That is not reproduced.
#pragma once

#include <cmath>
#include <cstdint>
#include <map>
#include <utility>

#include "ftte_expansion.h"

namespace ftte {

constexpr int kCatGroup = 256;           // threads of every catalogue kernel: four wave64
constexpr int kCatRounds = 4;            // leaves per thread of the compaction, one per round
constexpr int kCatTile = kCatGroup * kCatRounds; // leaves of a compaction workgroup
constexpr int32_t kCatNoStar = 0x7fffffff;       // `first` of a leaf without a star of weight > 0

// What star_locate_kernel reads and writes.  Node is NodeRec (ftte_node_rec.h): child0, leaf.
template <class Node> struct LocateRecT {
    const double *xyz;        // [nstars][3], the units of lo / hi
    const int32_t *weight;    // [nstars] >= 0, or nullptr: 1 each
    const Node *node;         // nullptr on a uniform grid: the leaf is the base index
    int64_t *star_cell;       // [nstars] host leaf, -1 outside the box
    int32_t *count;           // [ncell] summed weight, cleared by the caller
    int32_t *first;           // [ncell] lowest star index with weight > 0, kCatNoStar set by the caller
    unsigned long long *outside; // stars outside the box, cleared by the caller
    double lo[3], hi[3];
    int32_t n, nstars;
};

// What the compaction reads and writes (ascending cell-array index)
struct CompactRec {
    const int32_t *count, *first; // [ncell]
    int32_t *block_total;         // [nblock + 1]: pass one writes the tiles' counts, pass two turns them into offsets; [nblock] = nsrc
    int64_t *src_cell;            // [nsrc] pass three
    int32_t *src_weight;
    int64_t *src_first;
    int64_t ncell;
    int32_t nblock;
};

// (tmp1-xa)/(xb-xa), :750-752: the compiler's own IEEE subtraction and division -- a last bit decides the cell on a face
FTTE_XHD double catalogue_unit(double p, double lo, double hi) { return (p - lo) / (hi - lo); }

// i = int(x*nx) (+ 1 there) and xnew = x*float(nx) - float(i-1), :3060-3062 and :3086-3088, along one axis.  A star is inside where
// 0 <= int(x*nx) < nx, int() truncating as the reference's: that is -1 < x*nx < nx, tested before the conversion, so that NaN,
// +-inf and |x*nx| >= 2^31 never reach it.  -0.0 and nextafter(1, 0) are inside, 1.0 is not; like the reference's int(), the test
// keeps -1/nx < x < 0 in cell 0.
FTTE_XHD bool catalogue_base(double x, int n, int *i0, double *rem)
{
    const double xn = x * (double)n;
    if (!(xn > -1.0 && xn < (double)n)) return false;
    const int i = (int)xn;
    *i0 = i;
    *rem = x * (double)(float)n - (double)(float)i;
    return true;
}

// One level down (:3065-3107): the child is upper where the coordinate is >= 0.5, which then becomes 2x - 1, else 2x.  Returns the
// child's place 4 a + 2 b + c among its parent's eight.
FTTE_XHD int catalogue_descend(double *p)
{
    int h[3];
    for (int q = 0; q < 3; ++q) {
        h[q] = p[q] < 0.5 ? 0 : 1;
        p[q] = h[q] ? 2. * p[q] - 1. : 2. * p[q];
    }
    return 4 * h[0] + 2 * h[1] + h[2];
}

// The host leaf of the unit-cube point (x, y, z), or -1 outside the box.  node == nullptr: a uniform grid.  depth and path (may be
// nullptr): the level of the leaf and the child taken at each level, as LeafPos packs them.
template <class Node> FTTE_XHD int64_t catalogue_leaf(const Node *node, int n, double x, double y, double z, int *depth = nullptr, uint32_t *path = nullptr)
{
    int i, j, k;
    double p[3];
    if (!catalogue_base(x, n, &i, &p[0]) || !catalogue_base(y, n, &j, &p[1]) || !catalogue_base(z, n, &k, &p[2])) return -1;
    int64_t at = ((int64_t)i * n + j) * n + k;
    int level = 0;
    if (node) {
        for (int32_t child0 = node[at].child0; child0 >= 0; child0 = node[at].child0) {
            const int child = catalogue_descend(p);
            if (path && level < 10 * kExpPathWords) path[level / 10] |= (uint32_t)child << (3 * (level % 10));
            at = (int64_t)child0 + child;
            ++level;
        }
        at = node[at].leaf;
    }
    if (depth) *depth = level;
    return at;
}

// The reference's key of a leaf (:1177-1192): ((i-1)*ny+(j-1))*nz + k on the base level, then 10 * key + 1..8 per level, the digit
// counting (i,j,k) = (1,1,1), (1,1,2), (1,2,1) .. (2,2,2).  An integer*8 there; here it wraps the same way without overflowing a
// signed type.  Only the tests and the maker of the golden files use it, to tell which leaves collide.
inline int64_t catalogue_location_key(const LeafPos &P)
{
    uint64_t key = (uint64_t)P.base + 1u;
    for (int l = 0; l < P.depth; ++l) key = 10u * key + ((P.path[l / 10] >> (3 * (l % 10))) & 7u) + 1u;
    return (int64_t)key;
}

// (iMetal, coefMetal) of a source from its host cell's abun2, :1282-1293, the float32 literals 1.e-20 and -20. widened; libm's
// log10 as the reference's dlog10.  iMetal is 1-based and never exceeds nmetal - 1 (for nMetallicity = 2 the reference's loop reads
// past its array); coefMetal is clamped to [0, 1].
inline void catalogue_metal_bracket(double abun2, int nmetal, const double *metallicity, int32_t *iMetal, double *coefMetal)
{
    const double tmp = abun2 > (double)1.e-20f ? std::log10(abun2) : (double)-20.f;
    int i = 1;
    while (i + 1 < nmetal && tmp > metallicity[i]) ++i;
    double coef = (tmp - metallicity[i - 1]) / (metallicity[i] - metallicity[i - 1]);
    coef = coef > 0.0 ? coef : 0.0; // min(max(0.d0,coefMetal),1.d0)
    coef = coef < 1.0 ? coef : 1.0;
    *iMetal = i;
    *coefMetal = coef;
}

// One population slot per distinct (iMetal, bit pattern of coefMetal), numbered in order of first appearance; pop_first[p] is the
// first source that carries slot p's parameters (may be nullptr).  Returns the number of slots.
inline int64_t catalogue_slots(int64_t nsrc, const int32_t *iMetal, const double *coefMetal, int32_t *src_slot, int64_t *pop_first)
{
    std::map<std::pair<int32_t, uint64_t>, int32_t> seen;
    for (int64_t s = 0; s < nsrc; ++s) {
        union { double d; uint64_t u; } bits;
        bits.d = coefMetal[s];
        const auto at = seen.emplace(std::make_pair(iMetal[s], bits.u), (int32_t)seen.size());
        if (at.second && pop_first) pop_first[at.first->second] = s;
        src_slot[s] = at.first->second;
    }
    return (int64_t)seen.size();
}

// asynchronous on `stream`; 0, -1 bad argument, -2 launch failure
struct NodeRec;
int launch_star_locate(const LocateRecT<NodeRec> &R, void *stream);
int launch_compact_count(const CompactRec &R, void *stream);  // pass one
int launch_compact_scan(const CompactRec &R, void *stream);   // pass two
int launch_compact_emit(const CompactRec &R, void *stream);   // pass three

} // namespace ftte
