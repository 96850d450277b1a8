// ftte_medium.h -- MediumField: one field of the medium (the opacities; the emissivity or source function) as the caller handed it
// over, [nnu][ncell] in cell-array order, and every copy of it the sweeps read in another order.  The field owns the buffers and
// knows which copies still hold what the source holds: the source has a version, a copy remembers the version it was made from
// and the parameter it was made with, and it is current while both are still the source's and the caller's.  A copy whose buffer
// is new has never been made; a source that has to grow takes its copies with it.  Launches nothing: whoever makes a copy asks
// current(), launches, and says made().
#pragma once

#include <cstdint>

#include "ftte_device.h"

namespace ftte {

class MediumField {
public:
    // The copies.  Layouts 1 ([jc][ic][kc]) and 2 ([kc][ic][jc]): no parameter.  Brick order per axis order (option "tiled"): the
    // layers per piece.  Cell-major (the forests; all groups of a cell side by side): 0 = every leaf in cell-array order, else the
    // id of the hybrid plan's leaf list (HybridDevice::cells_id).
    enum Copy { kLayout1, kLayout2, kBricks0, kBricks1, kBricks2, kCellMajor, kCopies };
    static Copy layout(int l) { return Copy(kLayout1 + l - 1); } // l = 1, 2
    static Copy bricks(int l) { return Copy(kBricks0 + l); }     // l = 0, 1, 2

    double *source() const { return src_; }
    size_t capacity() const { return src_.capacity(); }
    bool valid() const { return valid_; } // the source holds what the caller set last (nothing in the library asks; for assertions)
    double *copy(Copy x) const { return copy_[x].buf; }
    double *in_layout(int l) const { return l ? copy(layout(l)) : source(); }
    // the addresses a captured hybrid sweep names: the source and its cell-major copy
    template <typename Sig> void sign(Sig &sig) const { sig.push_back((uintptr_t)source()); sig.push_back((uintptr_t)copy(kCellMajor)); }

    // Room for `need` elements in the source.  One that has to grow is released first together with every copy (they are sized
    // by it); on failure the field is empty.
    hipError_t reserve_source(size_t need)
    {
        if (src_ && src_.capacity() >= need) return hipSuccess;
        release();
        return src_.reserve(need);
    }
    // The source has new contents: no copy is current.  (A copy that one pass wrote together with the source is made() behind this.)
    void set() { ++version_; valid_ = true; }
    // ... is being written, or was left half written: no copy is current and the source is not valid until set()
    void invalidate() { ++version_; valid_ = false; }
    void release()
    {
        src_.reset();
        for (Derived &d : copy_) { d.buf.reset(); d.from = kNever; }
        invalidate();
    }

    bool current(Copy x, long long param = 0) const { return copy_[x].buf && copy_[x].from == version_ && copy_[x].param == param; }
    void made(Copy x, long long param = 0) { copy_[x].from = version_; copy_[x].param = param; }
    // Room for copy x: `need` elements, or as many as the source has.  A new buffer holds nothing, and one that could not be had
    // even less: not current.
    hipError_t reserve(Copy x, size_t need = 0)
    {
        bool fresh = false;
        const hipError_t e = copy_[x].buf.reserve(need ? need : src_.capacity(), &fresh);
        if (fresh || e != hipSuccess) copy_[x].from = kNever;
        return e;
    }

private:
    static constexpr long long kNever = -1;
    struct Derived { DeviceBuffer<double> buf; long long from = kNever, param = 0; };
    DeviceBuffer<double> src_;
    long long version_ = 0;
    bool valid_ = false;
    Derived copy_[kCopies];
};

} // namespace ftte
