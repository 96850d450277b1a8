// A stand-in for <hip/hip_runtime_api.h> on the CPU: the calls the owners of ftte_device.h use, backed by malloc, with a count of
// live objects, a count of releases, and a switch that makes the next allocation or creation fail; the copies and fills that
// ftte_bricks.h issues, as memcpy / memset with a count of the copies; the free memory that ftte_forests.h asks for.  tests/host/ only.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <cstring>

typedef enum { hipSuccess = 0, hipErrorOutOfMemory = 2 } hipError_t;
typedef struct stub_event *hipEvent_t;
typedef struct stub_stream *hipStream_t;
typedef struct stub_graph *hipGraph_t;
typedef struct stub_graph_exec *hipGraphExec_t;
typedef enum { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 } hipMemcpyKind;
enum { hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamDefault = 0, hipStreamNonBlocking = 1, hipHostMallocDefault = 0 };

struct stub_state {
    long live = 0, released = 0;
    long live_at_last_request = -1; // objects alive when the last allocation was asked for
    bool fail_next = false;
    int fail_countdown = 0;         // k > 0: the k-th allocation or creation from now fails
    long copies = 0;                // hipMemcpy / hipMemcpyAsync calls so far
    size_t free_bytes = (size_t)1 << 30; // what hipMemGetInfo reports
};
inline stub_state &stub() { static stub_state s; return s; }

inline hipError_t stub_make(void **out, size_t bytes)
{
    stub().live_at_last_request = stub().live;
    *out = nullptr;
    if (stub().fail_countdown > 0 && --stub().fail_countdown == 0) stub().fail_next = true;
    if (stub().fail_next) { stub().fail_next = false; return hipErrorOutOfMemory; }
    *out = std::malloc(bytes ? bytes : 1);
    ++stub().live;
    return hipSuccess;
}
inline hipError_t stub_release(void *p)
{
    std::free(p); // (the address sanitizer reports a block released twice)
    --stub().live;
    ++stub().released;
    return hipSuccess;
}

inline hipError_t hipMalloc(void **p, size_t bytes) { return stub_make(p, bytes); }
inline hipError_t hipFree(void *p) { return stub_release(p); }
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return stub_make(p, bytes); }
inline hipError_t hipHostFree(void *p) { return stub_release(p); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return stub_make((void **)e, 1); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return stub_release(e); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return stub_make((void **)s, 1); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return stub_release(s); }
inline hipError_t hipGraphDestroy(hipGraph_t g) { return stub_release(g); }
inline hipError_t hipGraphExecDestroy(hipGraphExec_t g) { return stub_release(g); }
// what hipStreamEndCapture / hipGraphInstantiate hand out
inline hipGraph_t stub_new_graph() { void *p; stub_make(&p, 1); return (hipGraph_t)p; }
inline hipGraphExec_t stub_new_graph_exec() { void *p; stub_make(&p, 1); return (hipGraphExec_t)p; }
// "device" memory is host memory here: a copy is a copy, and the streams run everything at once
inline hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { std::memcpy(dst, src, bytes); ++stub().copies; return hipSuccess; }
inline hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t) { return hipMemcpy(dst, src, bytes, kind); }
inline hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t) { std::memset(dst, value, bytes); return hipSuccess; }
inline hipError_t hipMemGetInfo(size_t *free_b, size_t *total_b) { *free_b = stub().free_bytes; *total_b = 2 * stub().free_bytes; return hipSuccess; }
inline hipError_t hipGetLastError() { return hipSuccess; }
