// ftte_forests.h -- what the two sweeps of a refined cell array share (forest_sweep for the whole tree, hybrid_sweep for the boxes):
// one direction's forest on the device (ForestTables), the packing of a linked forest into the records the device reads
// (pack_segments), the segment scratch with the batch records and per-depth tables of a run (ForestScratch), and the whole-tree
// forests kept from sweep to sweep (ForestCache).  Host only; launches nothing.
#pragma once

#include <cstdint>
#include <vector>

#include "ftte_amr.h"
#include "ftte_device.h"
#include "ftte_forest_rec.h"

namespace ftte {

// One direction's forest on the device.  The whole-tree path has no rays across a surface and one pass: exports, imports,
// pass_first and export_first stay empty there.
struct ForestTables {
    DeviceBuffer<SegRec> rec;          // active segments, depth after depth
    DeviceBuffer<uint8_t> active;      // per leaf (of the tree, or of the hybrid plan's list): AmrDirRec::active
    DeviceBuffer<AmrExport> exports; int64_t nexports = 0; // rays that leave the boxes into the bricks' face buffers
    DeviceBuffer<AmrImport> imports; int64_t nimports = 0; // into the face rings of a fine block's bricks
    std::vector<int64_t> depth_off;    // AmrForest::depth_off
    std::vector<int32_t> pass_first;   // the passes of depth_off (AmrForest::pass_first); empty: one pass
    std::vector<int64_t> export_first; // the passes of exports; empty: all in the first
    double w = 0;
};
// ... as a forest pass takes it: the tables and the direction's face block (hybrid sweep; else null)
struct ForestDir { const ForestTables *tables; double *faces; };

// What the device reads per active segment of a linked forest, in processing order (one zero record for an empty forest)
inline std::vector<SegRec> pack_segments(const AmrForest &f)
{
    std::vector<SegRec> rec(std::max<size_t>(f.order.size(), 1));
    for (size_t q = 0; q < f.order.size(); ++q) {
        const int32_t sg = f.order[q];
        rec[q].seg = sg; rec[q].up = f.up[(size_t)sg]; rec[q].up2 = f.up2[(size_t)sg];
        rec[q].at = f.up[(size_t)sg] == AmrForest::kImport ? f.import_at[(size_t)sg] : 0;
        rec[q].dpath = f.dpath[(size_t)sg];
    }
    return rec;
}

// Outgoing intensity and mean of every segment of every direction of a batch (the same number of elements each), the
// per-direction records of the batches and their per-depth tables (prepare_forests fills the last two).  Both paths use the
// same buffers: whoever sweeps asks for its batch and gets what the capacity the other left behind allows, or a new pair.
struct ForestScratch {
    DeviceBuffer<double> Iout, mean;
    DeviceBuffer<AmrDirRec> dirs;
    DeviceBuffer<int64_t> tables;

    size_t capacity() const { return std::min(Iout.capacity(), mean.capacity()); }
    void drop() { Iout.reset(); mean.reset(); }
    // The batch a sweep of ndir directions wants (at most `most`, per_dir elements per direction and array) fits what is there
    bool fits(size_t per_dir, int ndir, int most) const { return capacity() >= per_dir * (size_t)std::max(1, std::min(ndir, most)); }
    // Directions per batch, with room for them.  Where the scratch has to grow both arrays are released first and the batch is
    // what share_of_free of the free device memory holds; shrink_on_failure halves it until the allocation succeeds.  Where it
    // need not, the batch is what the capacity holds (at most `most`).  0: no memory (*error says what; both arrays are empty).
    int reserve_batch(size_t per_dir, int ndir, int most, double share_of_free, bool shrink_on_failure, hipError_t *error)
    {
        int batch = std::max(1, std::min(ndir, most));
        *error = hipSuccess;
        if (fits(per_dir, ndir, most)) return (int)std::min<size_t>((size_t)most, capacity() / per_dir);
        drop();
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            batch = (int)std::max<size_t>(1, std::min<size_t>((size_t)batch, (size_t)(share_of_free * (double)free_b) / (2 * sizeof(double) * per_dir)));
        for (;;) {
            if ((*error = Iout.reserve(per_dir * (size_t)batch)) == hipSuccess && (*error = mean.reserve(per_dir * (size_t)batch)) == hipSuccess) return batch;
            drop();
            (void)hipGetLastError();
            if (!shrink_on_failure || batch == 1) return 0;
            batch = (batch + 1) / 2;
        }
    }
    void sign(std::vector<uintptr_t> &sig) const
    {
        for (const void *p : {(const void *)Iout.get(), (const void *)mean.get(), (const void *)dirs.get(), (const void *)tables.get()}) sig.push_back((uintptr_t)p);
    }
};

// The forests of the whole tree, resident while the direction list, the tree and the box stay the same
struct ForestCache {
    std::vector<ForestTables> dirs;
    std::vector<double> key; // box, then phi, theta, w
    bool current(const std::vector<double> &k, int ndir) const { return k == key && (int)dirs.size() == ndir; }
    void drop() { dirs.clear(); key.clear(); }
};

} // namespace ftte
