// ftte_device.h -- the owners of everything the host side keeps on or for the device: DeviceBuffer<T> (hipMalloc), PinnedBuffer<T>
// (hipHostMalloc), Event, Stream, Graph, GraphExec.  Move-only; the destructor releases; the capacity of a buffer travels with its
// pointer.  Nothing outside this header allocates, creates, frees or destroys.  The owners never select a device: whoever creates
// or releases one has selected the context's device (ftte_destroy and multi_destroy do so before they delete the context).
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstddef>

namespace ftte {

// owned objects alive in this process: ftte_counter(ctx, "device_objects")
inline std::atomic<long> g_device_objects{0};

template <typename T, bool Pinned = false> class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~DeviceBuffer() { reset(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t capacity() const { return cap_; } // elements asked for; 0 while there is no buffer
    void reset()
    {
        if (p_) { (void)(Pinned ? hipHostFree(p_) : hipFree(p_)); --g_device_objects; }
        p_ = nullptr; cap_ = 0;
    }
    // Room for `need` elements.  A buffer that has it stays; otherwise the old one is freed first and then max(need, 1) elements are
    // allocated (contents are not kept), and *fresh says so.  On failure the buffer is empty and its capacity 0.
    hipError_t reserve(size_t need, bool *fresh = nullptr)
    {
        if (fresh) *fresh = false;
        if (p_ && cap_ >= need) return hipSuccess;
        reset();
        void *p = nullptr;
        const size_t bytes = std::max<size_t>(need, 1) * sizeof(T);
        const hipError_t e = Pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(p); cap_ = need;
        ++g_device_objects;
        if (fresh) *fresh = true;
        return hipSuccess;
    }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};
template <typename T> using PinnedBuffer = DeviceBuffer<T, true>;

// A runtime handle and the call that destroys it
template <typename H, hipError_t (*Destroy)(H)> class Handle {
public:
    Handle() = default;
    Handle(Handle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Handle &operator=(Handle &&o) noexcept
    {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
        return *this;
    }
    ~Handle() { reset(); }

    H get() const { return h_; }
    operator H() const { return h_; }
    void reset()
    {
        if (h_) { (void)Destroy(h_); --g_device_objects; }
        h_ = nullptr;
    }
    // takes over a handle the runtime has just made (hipStreamEndCapture, hipGraphInstantiate); whatever was held is destroyed
    void adopt(H h)
    {
        reset();
        h_ = h;
        if (h_) ++g_device_objects;
    }

private:
    H h_ = nullptr;
};

// create(flags) does nothing when the handle exists
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault)
    {
        if (get()) return hipSuccess;
        hipEvent_t e = nullptr;
        const hipError_t rc = hipEventCreateWithFlags(&e, flags);
        if (rc == hipSuccess) adopt(e);
        return rc;
    }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags = hipStreamDefault)
    {
        if (get()) return hipSuccess;
        hipStream_t s = nullptr;
        const hipError_t rc = hipStreamCreateWithFlags(&s, flags);
        if (rc == hipSuccess) adopt(s);
        return rc;
    }
};
using Graph = Handle<hipGraph_t, hipGraphDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;

} // namespace ftte
