// ftte_node_rec.h -- a node of the context's tree as the device holds it (DeviceTree, ftte_device_tree.h) and the kernels that
// descend through it read it: the point-source tracer, the maps of the analysis, the star catalogue.  The record alone, for device code.
#pragma once
#include <cstdint>

namespace ftte {

struct NodeRec { int32_t child0, leaf, parent, level; }; // a tree node: first child or -1, cell-array index or -1, parent or -1

} // namespace ftte
