// ftte_star_catalogue.h -- StarCatalogue: what ftte_star_catalogue keeps on the device (ftte_catalogue.cpp) -- the stars as they
// came, each star's host leaf, the per-leaf weight sums and first stars, the compaction's tile totals and the sources of the last
// catalogue -- and, on the host, each leaf's tree node for ftte_cell_position.  Dropped by ftte_set_grid with another tree, kept
// otherwise; the sources of the last catalogue stay until the next one succeeds or the tree changes.
#pragma once

#include <cstdint>
#include <vector>

#include "ftte_amr.h"
#include "ftte_catalogue.h"
#include "ftte_device.h"

namespace ftte {

class StarCatalogue {
public:
    // scratch of a call: the stars, and what is sized by the grid
    DeviceBuffer<double> xyz;              // [nstars][3]
    DeviceBuffer<int32_t> weight;          // [nstars]
    DeviceBuffer<int64_t> star_cell;       // [nstars]
    DeviceBuffer<int32_t> count, first;    // [ncell]
    DeviceBuffer<int32_t> block_total;     // [tiles + 1]
    DeviceBuffer<unsigned long long> outside;
    // the compacted outputs, ascending cell-array index
    DeviceBuffer<int64_t> src_cell, src_first;
    DeviceBuffer<int32_t> src_weight;
    DeviceBuffer<double> src_abun2;        // gathered by ftte_star_sources
    // around the launches of the last catalogue: locate [0, 1], pass one [1, 2], pass two [2, 3], pass three [4, 5]
    Event ev[6];
    bool emitted = false;                  // the last catalogue had sources, so pass three ran

    int64_t sources() const { return nsrc_; } // of the last catalogue; -1: there is none
    int64_t stars() const { return nstars_; }
    void begin() { nsrc_ = -1; nstars_ = 0; }  // the device work of a new catalogue starts: the old sources are being overwritten
    void made(int64_t nstars, int64_t nsrc) { nstars_ = nstars; nsrc_ = nsrc; }

    // node of every leaf of a refined tree, made on first use after ftte_set_grid (host only)
    const std::vector<int32_t> &leaf_nodes(const AmrTree &T)
    {
        if (leaf_node_.empty() && T.refined()) {
            leaf_node_.assign((size_t)T.ncell, -1);
            for (size_t v = 0; v < T.leaf.size(); ++v)
                if (T.leaf[v] >= 0) leaf_node_[(size_t)T.leaf[v]] = (int32_t)v;
        }
        return leaf_node_;
    }

    void drop_grid() // ftte_set_grid: the tree is another one
    {
        xyz.reset(); weight.reset(); star_cell.reset(); count.reset(); first.reset(); block_total.reset();
        src_cell.reset(); src_first.reset(); src_weight.reset(); src_abun2.reset();
        std::vector<int32_t>().swap(leaf_node_);
        nsrc_ = -1; nstars_ = 0;
    }

private:
    std::vector<int32_t> leaf_node_;
    int64_t nsrc_ = -1, nstars_ = 0;
};

// device time of phase 0 locate, 1 pass one, 2 pass two, 3 pass three of the last catalogue in nanoseconds; -1: none (ftte_catalogue.cpp)
long long catalogue_phase_ns(const StarCatalogue &K, int phase);

} // namespace ftte
