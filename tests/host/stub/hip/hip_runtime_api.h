// A stand-in for <hip/hip_runtime_api.h> on the CPU: the calls the owners of ftte_device.h use, backed by malloc, with a count of
// live objects, a count of releases, and a switch that makes the next allocation or creation fail; the copies and fills that
// ftte_bricks.h issues, as memcpy / memset with a count of the copies; the free memory that ftte_forests.h asks for; the pinning of
// host ranges and the waits that ftte_host.h calls.  The streams run everything at once unless stub().lazy asks for the laziest
// legal schedule: an asynchronous copy waits on its stream until the host waits for it.  For the sweeps of a refined cell array
// (ftte_sweeps.cpp, ftte_hybrid.cpp): a blocking fill, the device's properties, event times, and stream capture that reports failure.
// tests/host/ only.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

typedef enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorHostMemoryNotRegistered = 713, hipErrorStreamCaptureUnsupported = 900 } hipError_t;
typedef struct stub_event *hipEvent_t;
typedef struct stub_stream *hipStream_t;
typedef struct stub_graph *hipGraph_t;
typedef struct stub_graph_exec *hipGraphExec_t;
typedef enum { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 } hipMemcpyKind;
enum { hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamDefault = 0, hipStreamNonBlocking = 1, hipHostMallocDefault = 0, hipHostRegisterPortable = 1 };

struct stub_state {
    long live = 0, released = 0;
    long live_at_last_request = -1; // objects alive when the last allocation was asked for
    bool fail_next = false;
    int fail_countdown = 0;         // k > 0: the k-th allocation or creation from now fails
    long copies = 0;                // hipMemcpy / hipMemcpyAsync calls so far
    size_t free_bytes = (size_t)1 << 30; // what hipMemGetInfo reports
    std::set<const void *> pinned;  // bases of the ranges hipHostRegister has pinned and hipHostUnregister has not released
    long pin_calls = 0;             // hipHostRegister calls so far
    bool fail_pin_next = false;
    // The laziest legal schedule: hipMemcpyAsync, hipEventRecord and hipStreamWaitEvent only queue on their stream; the queue is
    // carried out, in order, as far as the host waits for it (hipEventSynchronize: up to that event's last record;
    // hipStreamSynchronize and hipStreamDestroy: all of it)
    bool lazy = false;
    struct queued { long id; void *dst; const void *src; size_t bytes; bool wait; hipStream_t on; long upto; }; // a copy, or wait: stream `on` has run up to id `upto`
    std::map<hipStream_t, std::vector<queued>> queue;
    struct recorded { hipStream_t on; long id; };
    std::map<hipEvent_t, recorded> last_record; // where an event's last record is queued
    long next_id = 1;
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
inline hipError_t hipEventDestroy(hipEvent_t e) { stub().last_record.erase(e); return stub_release(e); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return stub_make((void **)s, 1); }
inline void stub_run(hipStream_t s, long upto);
inline hipError_t hipStreamDestroy(hipStream_t s) { stub_run(s, stub().next_id); stub().queue.erase(s); return stub_release(s); }
inline hipError_t hipGraphDestroy(hipGraph_t g) { return stub_release(g); }
inline hipError_t hipGraphExecDestroy(hipGraphExec_t g) { return stub_release(g); }
// what hipStreamEndCapture / hipGraphInstantiate hand out
inline hipGraph_t stub_new_graph() { void *p; stub_make(&p, 1); return (hipGraph_t)p; }
inline hipGraphExec_t stub_new_graph_exec() { void *p; stub_make(&p, 1); return (hipGraphExec_t)p; }
// "device" memory is host memory here: a copy is a copy, and the streams run everything at once
inline hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { std::memcpy(dst, src, bytes); ++stub().copies; return hipSuccess; }
// carries out what is queued on stream s with an id up to `upto`
inline void stub_run(hipStream_t s, long upto)
{
    auto &Q = stub().queue[s];
    size_t done = 0;
    while (done < Q.size() && Q[done].id <= upto) {
        const stub_state::queued op = Q[done++];
        if (!op.wait) std::memcpy(op.dst, op.src, op.bytes);
        else if (op.on != s) stub_run(op.on, op.upto);
    }
    Q.erase(Q.begin(), Q.begin() + (long)done);
}
inline hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s)
{
    if (!stub().lazy) return hipMemcpy(dst, src, bytes, kind);
    ++stub().copies;
    stub().queue[s].push_back({stub().next_id++, dst, src, bytes, false, nullptr, 0});
    return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    if (stub().lazy) stub().last_record[e] = {s, stub().next_id++}; // (nothing to queue: the id says how far the stream has to run)
    return hipSuccess;
}
inline hipError_t hipEventSynchronize(hipEvent_t e)
{
    const auto r = stub().last_record.find(e);
    if (r != stub().last_record.end()) { stub_run(r->second.on, r->second.id); stub().last_record.erase(r); }
    return hipSuccess;
}
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned)
{
    const auto r = stub().last_record.find(e);
    if (r != stub().last_record.end()) stub().queue[s].push_back({stub().next_id++, nullptr, nullptr, 0, true, r->second.on, r->second.id});
    return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t s) { stub_run(s, stub().next_id); return hipSuccess; }
inline hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t) { std::memset(dst, value, bytes); return hipSuccess; }
inline hipError_t hipMemGetInfo(size_t *free_b, size_t *total_b) { *free_b = stub().free_bytes; *total_b = 2 * stub().free_bytes; return hipSuccess; }
inline hipError_t hipHostRegister(void *p, size_t, unsigned)
{
    ++stub().pin_calls;
    if (stub().fail_pin_next) { stub().fail_pin_next = false; return hipErrorOutOfMemory; }
    stub().pinned.insert(p);
    return hipSuccess;
}
inline hipError_t hipHostUnregister(void *p) { return stub().pinned.erase(p) ? hipSuccess : hipErrorHostMemoryNotRegistered; }
// what the sweeps of ftte_sweeps.cpp and ftte_hybrid.cpp call beside the above: a blocking fill, the device's properties, the
// time between two events (none passes here), and stream capture, which this runtime refuses: the hybrid sweep then issues its
// launches one by one
inline hipError_t hipMemset(void *dst, int value, size_t bytes) { std::memset(dst, value, bytes); return hipSuccess; }
struct hipDeviceProp_t { char gcnArchName[256]; int multiProcessorCount; };
inline hipError_t hipGetDeviceProperties(hipDeviceProp_t *prop, int) { std::memset(prop, 0, sizeof *prop); std::strcpy(prop->gcnArchName, "gfx950"); prop->multiProcessorCount = 256; return hipSuccess; }
inline hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
typedef enum { hipStreamCaptureModeGlobal = 0, hipStreamCaptureModeThreadLocal = 1, hipStreamCaptureModeRelaxed = 2 } hipStreamCaptureMode;
typedef struct stub_graph_node *hipGraphNode_t;
inline hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) { return hipErrorStreamCaptureUnsupported; }
inline hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t *graph) { *graph = nullptr; return hipErrorStreamCaptureUnsupported; }
inline hipError_t hipGraphInstantiate(hipGraphExec_t *exec, hipGraph_t, hipGraphNode_t *, char *, size_t) { *exec = nullptr; return hipErrorStreamCaptureUnsupported; }
inline hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { return hipErrorStreamCaptureUnsupported; }
inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipSetDevice(int) { return hipSuccess; } // (one device: the per-leaf updates of ftte_leaf_pass.cpp select theirs)
inline const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "error"; }
