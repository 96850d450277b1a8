// ftte_layout.h -- constants and launch wrappers of ftte_layout.hip: cell-array order into the sweep layouts, the merge of the
// accumulators into J, the sum of the devices' pieces of J.  All asynchronous on `stream`; return 0, -1 bad argument, -2 launch failure.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace ftte {

constexpr int kMaxAcc = 32;   // J accumulators per memory layout (tile kernel: one per slot; bricks: one per group)
constexpr int kMergeBlock = 32; // cells a side of a merge block (BrickPlan::merge_blocks): one 32 x 32 tile of merge_kernel per ic plane

// cell-array order -> layout 1 ([jc][ic][kc]) or 2 ([kc][ic][jc]); nnu groups, group_stride apart
int launch_to_layout(int layout, const double *src, double *dst, int n, int nnu, long group_stride, hipStream_t stream, bool tiled = false, int tchunk = 0); // tiled: brick order (BrickLaunch::tiled), layout 0 too; tchunk: layers per piece
// cell-array order -> the three layouts in one pass (dst0: a copy; dst1 null: layout 1 left out)
int launch_set_layouts(const double *src, double *dst0, double *dst1, double *dst2, int n, int nnu, long group_stride, hipStream_t stream);
// J (cell-array order) = acc[0] + acc[1] + ... in list order; layout[a] in {0,1,2}
int launch_merge(const double *const *acc, const int *layout, int count, double *J, int n, int nnu, long group_stride,
                 bool accumulate, hipStream_t stream, const int32_t *leaf_of_base = nullptr, long j_stride = 0, bool tiled = false, int tchunk = 0);
// the same sums for the merge blocks blocks[0 .. nblocks) only (BrickPlan::merge_blocks; nmb blocks a side)
int launch_merge_blocks(const double *const *acc, const int *layout, int count, double *J, int n, int nnu, long group_stride,
                        const int32_t *blocks, int nblocks, int nmb, hipStream_t stream, bool tiled = false, int tchunk = 0);
// out[q] = parts[0][q] + parts[1][q] + ... (in that order), q < count: the pieces of J the devices of one context swept for different
// directions (ftte_multi.cpp; the partners' buffers are read where they lie)
int launch_sum_parts(const double *const *parts, int nparts, double *out, long count, hipStream_t stream);

} // namespace ftte
