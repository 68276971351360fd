// lpg_host.h — the host scaffold of the batch families (lpg_assign, lpg_binary,
// lpg_transport; lpg_batch uses the error part only). Host code only: nothing
// here is __device__ or __global__, every kernel stays in the file that
// launches it.
//
// A family's handle derives from BatchHost, lists its device arrays once
// (`allocs`, at create) and supplies its own validation and kernels. The
// header owns what is the same for all of them: the error buffers, the device
// side made by the first call that needs it and taken down whole, the loaded
// bookkeeping, the LDS raise and the timed launch.
#pragma once
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/lpg.h"
#include "lpg_internal.h"

namespace lpg {

constexpr size_t kErrLen = 512;

// The message of the last failed call without a handle, per thread and per
// handle type H: a failing lpg_transport_create leaves lpg_assign_last_error(NULL) alone.
template <class H>
char *thread_err() {
    static thread_local char buf[kErrLen];
    return buf;
}

// The message to h->err (h may be null: fail<H>(nullptr, ...)) and to H's thread buffer; returns code.
template <class H>
int fail(H *h, int code, const char *fmt, ...) {
    char buf[kErrLen];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) snprintf(h->err, sizeof h->err, "%s", buf);
    snprintf(thread_err<H>(), kErrLen, "%s", buf);
    return code;
}

#define LPG_HIPCHK(h, x)                                                                  \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            (void)hipGetLastError();                                                      \
            return lpg::fail((h), LPG_ERR_DEVICE, "%s: %s", #x, hipGetErrorString(e_));   \
        }                                                                                 \
    } while (0)

inline bool env_is(const char *name, const char *value) {
    const char *e = getenv(name);
    return e && !strcmp(e, value);
}

struct DevAlloc {
    void **slot;           // a device pointer of the handle
    size_t bytes;          // 0: not needed, the slot stays null
};

template <class T>
DevAlloc dev_array(T *&p, int64_t n) {
    return {(void **)&p, (size_t)n * sizeof(T)};
}

// What every handle of a batch family carries.
struct BatchHost {
    int device = 0;
    int64_t count = 0;
    int64_t lds = 0;              // dynamic LDS of the solve kernel
    bool on_device = false;       // the device side exists (made by the first call that needs it)
    bool loaded = false;          // every problem has data (a load of the whole range, or generate)
    std::vector<uint8_t> have;    // per problem: loaded
    bool solved = false;
    bool lds_raised = false;
    std::vector<DevAlloc> allocs; // the device arrays, in the order they are made (set once, at create)
    char oom_what[96] = {0};      // what the out-of-memory message says was asked for
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;     // around each solve launch
    double kernel_ms = 0.0;
    int64_t launches = 0;
    char err[kErrLen] = {0};
};

// everything ensure_device made, whole or in part
inline void release_device(BatchHost *h) {
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (const DevAlloc &a : h->allocs) {
        if (*a.slot) (void)hipFree(*a.slot);
        *a.slot = nullptr;
    }
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    h->ev0 = h->ev1 = nullptr;
    h->stream = nullptr;
    h->on_device = false;
}

// Device memory, stream, events: made by the first call that moves data or
// launches, so that every refusal of create, load, generate and solve is
// answered before the library touches a device. A setup that fails is taken
// down again, and the next call starts it afresh.
template <class H>
int ensure_device(H *h, const char *call) {
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, LPG_ERR_DEVICE, "%s: hipSetDevice(%d): %s", call, h->device, hipGetErrorString(e));
    }
    if (h->on_device) return 0;
    for (const DevAlloc &a : h->allocs)
        if (a.bytes && hipMalloc(a.slot, a.bytes) != hipSuccess) {
            (void)hipGetLastError();
            release_device(h);
            return fail(h, LPG_ERR_OOM, "%s: hipMalloc(%s) failed", call, h->oom_what);
        }
    if ((e = hipStreamCreate(&h->stream)) != hipSuccess || (e = hipEventCreate(&h->ev0)) != hipSuccess ||
        (e = hipEventCreate(&h->ev1)) != hipSuccess) {
        (void)hipGetLastError();
        release_device(h);
        return fail(h, LPG_ERR_DEVICE, "%s: stream and events: %s", call, hipGetErrorString(e));
    }
    h->on_device = true;
    return 0;
}

template <class H>
void destroy(H *h) {
    if (!h) return;
    if (h->on_device) {
        (void)hipSetDevice(h->device);
        release_device(h);
    }
    delete h;
}

// problems [first, first + n) of a load or a get
template <class H>
int range_ok(H *h, const char *call, int64_t first, int64_t n) {
    if (first < 0 || n < 1 || first > h->count || n > h->count - first)
        return fail(h, LPG_ERR_ARG, "%s: problems [%lld, %lld) outside the batch of %lld (need n >= 1)", call,
                    (long long)first, (long long)(first + n), (long long)h->count);
    return 0;
}

inline void mark_loaded(BatchHost *h, int64_t first, int64_t n) {
    for (int64_t p = 0; p < n; p++) h->have[(size_t)(first + p)] = 1;
    h->loaded = true;
    for (uint8_t v : h->have) h->loaded = h->loaded && v;
}

inline void mark_all_loaded(BatchHost *h) {
    h->have.assign((size_t)h->count, 1);
    h->loaded = true;
}

// the first problem without data (count: none)
inline int64_t first_unloaded(const BatchHost *h) {
    int64_t q = 0;
    while (q < h->count && h->have[(size_t)q]) q++;
    return q;
}

// The solve kernel may use `bytes` of dynamic LDS; asked of the runtime once per handle.
template <class H>
int raise_lds_once(H *h, const void *kernel, int bytes, const char *call) {
    if (h->lds_raised) return 0;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, LPG_ERR_DEVICE, "%s: hipFuncSetAttribute(%d bytes of LDS) failed", call, bytes);
    }
    h->lds_raised = true;
    return 0;
}

// kernel(geo) on `grid` workgroups of kBlock threads with h->lds bytes of LDS, between the handle's two events
template <class Geo>
hipError_t timed_launch(BatchHost *h, const void *kernel, unsigned grid, Geo &geo) {
    void *args[] = {&geo};
    (void)hipEventRecord(h->ev0, h->stream);
    const hipError_t e = hipLaunchKernel(kernel, dim3(grid), dim3(kBlock), args, (size_t)h->lds, h->stream);
    (void)hipEventRecord(h->ev1, h->stream);
    return e;
}

}  // namespace lpg
