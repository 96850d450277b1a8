// ftte_host.h -- HostBoundary: what the context keeps for host arrays that cross PCIe.  A pageable array goes through two pinned staging
// blocks, one filled or emptied by a few host threads while the other is in flight; a registered array is copied by the DMA engine in place.
// The one rule: nobody, host thread or DMA engine, touches a block before the transfer recorded on it has been waited for, on whatever
// stream that was queued and whether or not its sequence came to its end.  Selects no device.
#pragma once

#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "ftte_device.h"

namespace ftte {

inline void parallel_copy(void *dst, const void *src, size_t bytes)
{
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t nthreads = std::min<size_t>(std::min(8u, hw), std::max<size_t>(1, bytes >> 22));
    if (nthreads <= 1) { std::memcpy(dst, src, bytes); return; }
    const size_t chunk = ((bytes + nthreads - 1) / nthreads + 63) & ~(size_t)63;
    std::vector<std::thread> pool;
    for (size_t t = 0; t < nthreads; ++t) {
        const size_t lo = t * chunk;
        if (lo >= bytes) break;
        const size_t len = std::min(chunk, bytes - lo);
        pool.emplace_back([=] { std::memcpy((char *)dst + lo, (const char *)src + lo, len); });
    }
    for (auto &th : pool) th.join();
}

class HostBoundary {
public:
    explicit HostBoundary(size_t block_bytes = (size_t)64 << 20) : block_bytes_(block_bytes) {}
    ~HostBoundary() // the caller's arrays: pinned here, not owned
    {
        for (const Range &r : ranges_) if (r.own) (void)hipHostUnregister((void *)r.base);
    }

    DeviceBuffer<double> J_dev; // a host-array sweep's J on the device, kept from call to call

    // The registered ranges: pinned here (pin, unpin; the destructor unpins what is left), or by another context of the process,
    // a sibling of one multi-device context (learn, forget: every learnt range with that base).  A contained range is not added again.
    bool contains(const void *p, size_t bytes) const
    {
        const char *b = (const char *)p;
        return std::any_of(ranges_.begin(), ranges_.end(), [&](const Range &r) { return b >= r.base && b + bytes <= r.base + r.bytes; });
    }
    hipError_t pin(void *p, size_t bytes)
    {
        if (contains(p, bytes)) return hipSuccess;
        const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable); // (portable: pinned for every device of the process)
        if (e == hipSuccess) ranges_.push_back({(const char *)p, bytes, true});
        return e;
    }
    bool pinned(const void *base) const { return find(base) != ranges_.end(); }
    hipError_t unpin(void *base) // hipErrorHostMemoryNotRegistered: not the base of a range pinned here
    {
        const auto r = find(base);
        const hipError_t e = r == ranges_.end() ? hipErrorHostMemoryNotRegistered : hipHostUnregister(base);
        if (e == hipSuccess) ranges_.erase(r);
        return e;
    }
    void learn(const void *p, size_t bytes) { if (!contains(p, bytes)) ranges_.push_back({(const char *)p, bytes, false}); }
    void forget(const void *base) { ranges_.erase(std::remove_if(ranges_.begin(), ranges_.end(), [&](const Range &r) { return r.base == base && !r.own; }), ranges_.end()); }
    bool outstanding(int q) const { return out_[q]; } // block q has a transfer recorded that nobody has waited for
    // host -> device: block q is filled while block q^1 is in flight; back when the last piece is the DMA engine's, its blocks left outstanding
    hipError_t send(hipStream_t stream, void *dst_dev, const void *src_host, size_t bytes)
    {
        hipError_t e = hipSuccess;
        int q = 0;
        for (size_t off = 0; off < bytes && e == hipSuccess; off += block_bytes_, q ^= 1) {
            const size_t len = std::min(block_bytes_, bytes - off);
            if ((e = claim(q)) != hipSuccess) break;
            parallel_copy(block_[q], (const char *)src_host + off, len);
            e = issue(q, (char *)dst_dev + off, block_[q], len, hipMemcpyHostToDevice, stream);
        }
        return e;
    }
    // device -> host: the DMA engine fills block q while the host empties block q^1 of the piece before (hence one turn more than pieces)
    hipError_t fetch(hipStream_t stream, void *dst_host, const void *src_dev, size_t bytes)
    {
        hipError_t e = hipSuccess;
        int q = 0;
        for (size_t off = 0; off < bytes + block_bytes_ && e == hipSuccess; off += block_bytes_, q ^= 1) {
            if (off < bytes && (e = claim(q)) == hipSuccess)
                e = issue(q, block_[q], (const char *)src_dev + off, std::min(block_bytes_, bytes - off), hipMemcpyDeviceToHost, stream);
            if (off == 0 || e != hipSuccess || (e = claim(q ^ 1)) != hipSuccess) continue;
            const size_t prev = off - block_bytes_, len_prev = std::min(block_bytes_, bytes - prev); // the piece of the turn before
            parallel_copy((char *)dst_host + prev, block_[q ^ 1], len_prev);
        }
        return e;
    }

private:
    struct Range { const char *base; size_t bytes; bool own; };
    std::vector<Range>::const_iterator find(const void *base) const // among those pinned here
    {
        return std::find_if(ranges_.begin(), ranges_.end(), [&](const Range &r) { return r.base == base && r.own; });
    }
    // block q is there (asked for on first use, and again after a failure) and free: whoever waits for its transfer clears the flag
    hipError_t claim(int q)
    {
        hipError_t e = block_[q].reserve(block_bytes_);
        if (e == hipSuccess) e = event_[q].create(hipEventDisableTiming);
        if (e == hipSuccess && out_[q]) e = hipEventSynchronize(event_[q]);
        if (e == hipSuccess) out_[q] = false;
        return e;
    }
    hipError_t issue(int q, void *dst, const void *src, size_t len, hipMemcpyKind kind, hipStream_t stream)
    {
        hipError_t e = hipMemcpyAsync(dst, src, len, kind, stream);
        if (e == hipSuccess && (e = hipEventRecord(event_[q], stream)) == hipSuccess) out_[q] = true;
        return e;
    }

    const size_t block_bytes_;
    PinnedBuffer<char> block_[2];
    Event event_[2];
    bool out_[2] = {false, false};
    std::vector<Range> ranges_;
};

} // namespace ftte
