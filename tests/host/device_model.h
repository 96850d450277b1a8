// device_model.h -- what tests/host/device_model.cpp (host definitions of the launches, ftte_*_rec.h and ftte_layout.h, that the refined-grid sweeps
// reach) shares with the program that drives it: the oracle's per-direction values that the oracle brick reads and writes, the
// patterns the face block and the scratch are poisoned with, and the record of what the model found.  tests/host/ only.
#pragma once

#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "ftte_context.h"

namespace model {

// a signalling NaN with a payload: what the face block and the segment scratch hold before a sweep
constexpr uint64_t kPoisonBits = 0x7ff4dead0badf00dull;
// another: what the oracle brick writes where the kernel hands on rays of cells that are not in the grid (padding), or rays nobody
// the oracle knows takes
constexpr uint64_t kJunkBits = 0x7ff40bad0000beefull;
inline double from_bits(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }
inline uint64_t bits_of(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }
inline void poison(double *p, size_t count) { const double x = from_bits(kPoisonBits); for (size_t q = 0; q < count; ++q) p[q] = x; }

// One direction of the whole tree, evaluated by a loop of the test's own on build_forest without regions: per segment
// (3 * leaf + slot; slot 0 xy, 1 xz, 2 yz) and frequency group the incoming intensity, the outgoing intensity and the mean
struct DirOracle {
    int izone = 0;
    double w = 0;
    std::vector<int32_t> up;             // [3 ncell] AmrForest::up (kInactive: the leaf has no such segment)
    std::vector<double> Iin, Iout, mean; // [3 ncell][nnu]
    std::vector<double> cell;            // [ncell][nnu] what the direction adds to J of a leaf: ftte_cell_mean of its segments' means
    // a fine block swept by bricks of its own: 3 * leaf + face of a leaf of the block -> the segment whose outgoing intensity a
    // leaf outside the block takes through that face
    std::map<int32_t, int32_t> handed;
};

struct State {
    const ftte_ctx *c = nullptr;        // the context that sweeps
    int nnu = 0;
    std::vector<const DirOracle *> dir; // the directions of the call, in the caller's order
    const void *drop_task = nullptr;    // seeded fault: the brick task at this address is left out
    // what the model found: comparisons made, those that failed, the first one in words
    long compared = 0, failures = 0;
    std::string first;
    long brick_tasks = 0, masked_tasks = 0, sub_tasks = 0, levels = 0, fused = 0, exports = 0, imports = 0; // what ran
    void clear() { compared = failures = 0; first.clear(); brick_tasks = masked_tasks = sub_tasks = levels = fused = exports = imports = 0; }
};
State &state();

} // namespace model
