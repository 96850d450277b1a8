// ftte_catalogue.hip -- the star catalogue on the device (equiSources.f90:746-769 and :1169-1212): every star's host leaf, and the
// stars of one leaf merged into one source.
//
// star_locate_kernel: one thread per star.  The star's coordinates become unit-cube coordinates, the base cell follows from them
// and the tree is descended through its node records, one dependent 16-byte load per level (ftte_catalogue.h holds the rules, in the
// reference's operations).  A star inside the box with weight > 0 adds its weight to count[leaf] and offers its index to
// first[leaf]: two integer atomics without a return value, so that neither depends on the order in which the stars arrive.
//
// The sources are the leaves with count > 0 in ascending cell-array index, compacted in three passes over tiles of kCatTile leaves:
// the tiles' counts, one scan of those counts by a single workgroup, then the emission.  Inside a tile a thread looks at one leaf per
// round, kCatRounds rounds of kCatGroup consecutive leaves; its rank is the ballot of its wave (64 bits: a wave is 64 lanes wide)
// below its own lane plus the counts of the waves and rounds before it.  Nothing is sorted and nothing is hashed; the result is
// the same whatever the order of the stars.
#include <hip/hip_runtime.h>

#include "ftte_catalogue.h"
#include "ftte_node_rec.h"

namespace ftte {

namespace {

constexpr int kWaves = kCatGroup / 64;

__global__ void __launch_bounds__(kCatGroup) star_locate_kernel(const LocateRecT<NodeRec> R)
{
    const int64_t s = (int64_t)blockIdx.x * kCatGroup + threadIdx.x;
    bool out = false;
    if (s < R.nstars) {
        const double *p = R.xyz + 3 * s;
        const double x = catalogue_unit(p[0], R.lo[0], R.hi[0]);
        const double y = catalogue_unit(p[1], R.lo[1], R.hi[1]);
        const double z = catalogue_unit(p[2], R.lo[2], R.hi[2]);
        const int64_t leaf = catalogue_leaf(R.node, R.n, x, y, z);
        R.star_cell[s] = leaf;
        out = leaf < 0;
        const int32_t w = R.weight ? R.weight[s] : 1;
        if (!out && w > 0) {
            atomicAdd(R.count + leaf, w);
            atomicMin(R.first + leaf, (int32_t)s);
        }
    }
    // stars outside are counted: one addition per wave
    const unsigned long long mask = __ballot(out);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(R.outside, (unsigned long long)__popcll(mask));
}

// Pass one (EMIT false): block_total[b] = occupied leaves of tile b.  Pass three (EMIT true): block_total[b] is the tile's offset
// among the sources; every occupied leaf writes its source.
template <bool EMIT> __global__ void __launch_bounds__(kCatGroup) compact_kernel(const CompactRec R)
{
    __shared__ int s_count[kCatRounds][kWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile0 = (int64_t)blockIdx.x * kCatTile;

    int weight[kCatRounds], rank[kCatRounds];
    for (int r = 0; r < kCatRounds; ++r) {
        const int64_t c = tile0 + (int64_t)r * kCatGroup + tid;
        weight[r] = c < R.ncell ? R.count[c] : 0;
        const unsigned long long mask = __ballot(weight[r] > 0);
        rank[r] = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) s_count[r][wave] = __popcll(mask);
    }
    __syncthreads();
    if (!EMIT) {
        if (tid == 0) {
            int total = 0;
            for (int r = 0; r < kCatRounds; ++r)
                for (int w = 0; w < kWaves; ++w) total += s_count[r][w];
            R.block_total[blockIdx.x] = total;
        }
        return;
    }
    int before = R.block_total[blockIdx.x];
    for (int r = 0; r < kCatRounds; ++r) {
        for (int w = 0; w < wave; ++w) before += s_count[r][w];
        if (weight[r] > 0) {
            const int64_t c = tile0 + (int64_t)r * kCatGroup + tid;
            const int64_t at = (int64_t)before + rank[r];
            R.src_cell[at] = c;
            R.src_weight[at] = weight[r];
            R.src_first[at] = (int64_t)R.first[c];
        }
        for (int w = wave; w < kWaves; ++w) before += s_count[r][w];
    }
}

// Pass two: the tiles' counts become their exclusive prefix sums, block_total[nblock] the number of sources.  One workgroup walks
// the list kCatGroup entries at a time: a wave scans its 64 by shuffles, the waves' totals go through LDS.
__global__ void __launch_bounds__(kCatGroup) compact_scan_kernel(const CompactRec R)
{
    __shared__ int s_wave[kWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int b0 = 0; b0 < R.nblock; b0 += kCatGroup) {
        const int b = b0 + tid;
        const int own = b < R.nblock ? R.block_total[b] : 0;
        int incl = own;
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        __syncthreads(); // the last round's totals have been read by everyone
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = carry, all = 0;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) before += s_wave[w];
            all += s_wave[w];
        }
        if (b < R.nblock) R.block_total[b] = before + incl - own;
        carry += all;
    }
    if (tid == 0) R.block_total[R.nblock] = carry;
}

} // namespace

int launch_star_locate(const LocateRecT<NodeRec> &R, void *stream)
{
    if (R.nstars < 1 || R.n < 1 || !R.xyz || !R.star_cell || !R.count || !R.first || !R.outside) return -1;
    const unsigned groups = (unsigned)(((int64_t)R.nstars + kCatGroup - 1) / kCatGroup);
    hipLaunchKernelGGL(star_locate_kernel, dim3(groups), dim3(kCatGroup), 0, (hipStream_t)stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

static bool compact_ok(const CompactRec &R)
{
    return R.ncell >= 1 && R.count && R.block_total && R.nblock >= 1 && (int64_t)R.nblock * kCatTile >= R.ncell &&
           ((int64_t)R.nblock - 1) * kCatTile < R.ncell;
}

int launch_compact_count(const CompactRec &R, void *stream)
{
    if (!compact_ok(R)) return -1;
    hipLaunchKernelGGL(compact_kernel<false>, dim3((unsigned)R.nblock), dim3(kCatGroup), 0, (hipStream_t)stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_compact_scan(const CompactRec &R, void *stream)
{
    if (!compact_ok(R)) return -1;
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kCatGroup), 0, (hipStream_t)stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_compact_emit(const CompactRec &R, void *stream)
{
    if (!compact_ok(R) || !R.first || !R.src_cell || !R.src_weight || !R.src_first) return -1;
    hipLaunchKernelGGL(compact_kernel<true>, dim3((unsigned)R.nblock), dim3(kCatGroup), 0, (hipStream_t)stream, R);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

} // namespace ftte
