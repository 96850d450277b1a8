// ftte_host_arrays.cpp -- host arrays across PCIe: which stream, when an array goes directly, what ends the call (the rest: ftte_host.h).
#include "ftte_context.h"

namespace ftte {

constexpr size_t kDirectBelow = (size_t)1 << 20; // on c->stream an array this small is not worth the staging
bool is_registered(const ftte_ctx *c, const void *p, size_t bytes) { return c->host.contains(p, bytes); }

// host -> device on c->stream; returns with the copy complete
int upload(ftte_ctx *c, void *dst_dev, const void *src_host, size_t bytes)
{
    if (bytes < kDirectBelow) FTTE_HIP(c, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, c->stream));
    else if (int rc = upload_on(c, c->stream, dst_dev, src_host, bytes)) return rc;
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    return FTTE_OK;
}

// device -> host on c->stream (after whatever is queued there); returns with the copy complete
int download(ftte_ctx *c, void *dst_host, const void *src_dev, size_t bytes)
{
    if (!is_registered(c, dst_host, bytes) && bytes >= kDirectBelow) return download_on(c, c->stream, dst_host, src_dev, bytes);
    FTTE_HIP(c, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    FTTE_HIP(c, hipStreamSynchronize(c->stream));
    return FTTE_OK;
}

// host -> device on stream q; returns when the last piece has been handed to the DMA engine (not when it has arrived)
int upload_on(ftte_ctx *c, hipStream_t q, void *dst_dev, const void *src_host, size_t bytes)
{
    if (is_registered(c, src_host, bytes)) FTTE_HIP(c, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, q));
    else FTTE_HIP(c, c->host.send(q, dst_dev, src_host, bytes));
    return FTTE_OK;
}

// device -> pageable host memory (the caller has asked is_registered) behind whatever is queued on stream q; returns with the copy complete
int download_on(ftte_ctx *c, hipStream_t q, void *dst_host, const void *src_dev, size_t bytes)
{
    FTTE_HIP(c, c->host.fetch(q, dst_host, src_dev, bytes));
    return FTTE_OK;
}

} // namespace ftte
