// wost_host.h -- the host-side helpers every translation unit of libwost_hip.so shares (host code only, not part of the
// C-ABI): the error macro, device scratch, uploads, environment switches and the skeleton of a batch entry point.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/wost.h"

namespace wost {

// records the message returned by wost_last_error() on this thread; returns `code`
int set_error(int code, const std::string &msg);

// a failed HIP call as the library reports it: WOST_ERR_DEVICE, "<expression text>: <hip error string>"
inline int hip_failed(const char *what, hipError_t e) { return set_error(WOST_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }

// an environment switch as an integer clamped to lo..hi; `fallback` when it is not set
inline int env_int(const char *name, int fallback, int lo = INT_MIN, int hi = INT_MAX)
{
    const char *w = std::getenv(name);
    return w ? std::min(hi, std::max(lo, std::atoi(w))) : fallback;
}

// `count` elements of src in a device array of their own, owned by `allocs` (synchronous: the mesh uploads)
template <class T>
hipError_t upload(std::vector<void *> &allocs, const T *src, size_t count, const T **dst)
{
    *dst = nullptr;
    if (count == 0) return hipSuccess;
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess) return e;
    allocs.push_back(p);
    *dst = reinterpret_cast<const T *>(p);
    return hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
}

// device scratch of the batch entry points, freed on every return path
struct Scratch {
    std::vector<void *> ptrs;
    ~Scratch()
    {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <class T>
    hipError_t alloc(T **p, size_t count)
    {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, count * sizeof(T) + 16);
        if (e == hipSuccess) ptrs.push_back(q);
        *p = reinterpret_cast<T *>(q);
        return e;
    }
};

// solve_ms of a host call is the host wall time of the whole call (include/wost.h): stamped after the download, in 2-D and 3-D
using HostClock = std::chrono::high_resolution_clock;
inline void stamp_solve_ms(wost_stats *stats, HostClock::time_point t0)
{
    if (stats) stats->solve_ms = std::chrono::duration<double, std::milli>(HostClock::now() - t0).count();
}

}  // namespace wost

// `return`s the recorded error from the enclosing function when a HIP call fails.  WOST_TRY_AS is the one definition, `text`
// what the message names; WOST_BUILD_TRY is the mesh builders' form, with "mesh build: " in front
#define WOST_TRY_AS(text, expr)                                                                         \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return wost::hip_failed(text, e_);                                        \
    } while (0)
#define WOST_TRY(expr) WOST_TRY_AS(#expr, expr)
#define WOST_BUILD_TRY(expr) WOST_TRY_AS("mesh build: " #expr, expr)

namespace wost {

// Host arrays in, a launch, host arrays out: the allocations and copies of a batch entry point, all on one stream.  The
// entry point checks its arguments, sets the device and launches; nothing here synchronises before finish().
struct Batch {
    hipStream_t stream;
    Scratch scratch;
    // a device array of `count` elements, filled from the host (the copy is issued, not waited for) ...
    template <class T>
    hipError_t in(const T *host, size_t count, T **dev)
    {
        const hipError_t e = scratch.alloc(dev, count);
        return e != hipSuccess ? e : hipMemcpyAsync(*dev, host, count * sizeof(T), hipMemcpyHostToDevice, stream);
    }
    // ... and one left as it is for the launch to fill
    template <class T>
    hipError_t out(T **dev, size_t count) { return scratch.alloc(dev, count); }
    // `count` elements of a device array on their way to the host; a null host array is an output the caller left out
    template <class T>
    hipError_t fetch(T *host, const T *dev, size_t count)
    {
        return host ? hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, stream) : hipSuccess;
    }
    int finish()
    {
        WOST_TRY(hipStreamSynchronize(stream));
        return WOST_OK;
    }
};

}  // namespace wost
