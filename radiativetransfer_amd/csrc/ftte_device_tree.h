// ftte_device_tree.h -- DeviceTree: the nodes of the context's AmrTree in device memory, as the point-source tracer and the maps of
// ftte_analysis.cpp descend through them, and each leaf's node on the host.  Uploaded on first use after ftte_set_grid; a uniform
// grid has neither (node == cell).
#pragma once

#include <cstdint>
#include <vector>

#include "ftte_amr.h"
#include "ftte_device.h"
#include "ftte_node_rec.h"

namespace ftte {

class DeviceTree {
public:
    // No-op once made.  On failure nothing is held and the next call tries again.
    hipError_t ensure(hipStream_t stream, const AmrTree &tree)
    {
        if (ready_) return hipSuccess;
        drop();
        if (tree.refined()) {
            const size_t nnode = tree.parent.size();
            std::vector<NodeRec> nodes(nnode);
            node_of_leaf_.assign((size_t)tree.ncell, -1);
            for (size_t v = 0; v < nnode; ++v) {
                nodes[v] = NodeRec{tree.child0[v], tree.leaf[v], tree.parent[v], (int32_t)tree.level[v]};
                if (tree.leaf[v] >= 0) node_of_leaf_[(size_t)tree.leaf[v]] = (int32_t)v;
            }
            hipError_t e = node_.reserve(nnode);
            if (e == hipSuccess) e = hipMemcpyAsync(node_, nodes.data(), sizeof(NodeRec) * nnode, hipMemcpyHostToDevice, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream); // (`nodes` is a local)
            if (e != hipSuccess) { drop(); return e; }
        }
        ready_ = true;
        return hipSuccess;
    }
    const NodeRec *nodes() const { return node_; } // null on a uniform grid
    int32_t node_of(int64_t cell) const { return node_of_leaf_.empty() ? (int32_t)cell : node_of_leaf_[(size_t)cell]; } // cell-array index -> node
    void drop() // ftte_set_grid: the tree is another one
    {
        node_.reset();
        std::vector<int32_t>().swap(node_of_leaf_);
        ready_ = false;
    }

private:
    DeviceBuffer<NodeRec> node_;
    std::vector<int32_t> node_of_leaf_;
    bool ready_ = false;
};

} // namespace ftte
