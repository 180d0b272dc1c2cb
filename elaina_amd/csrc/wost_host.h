// wost_host.h -- the host-side helpers every translation unit of libwost_hip.so shares (host code only, not part of the
// C-ABI): the error macro, device scratch, uploads, environment switches, the LDS of a query kernel's stack columns, the sum of two
// wost_stats, the byte comparison of the mesh build checks and the skeleton of a batch entry point.
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

// (hidden: the dynamic symbol table of the library stays the C-ABI and what it held before; nothing here joins it)
#pragma GCC visibility push(hidden)

// LDS bytes of the traversal stacks of a 256-lane block of a query kernel over a tree of `levels` levels: a column of
// 3 * levels + 1 entries per lane (pushes on the inner levels, at most 3 each; the Neumann tree queries push up to 4 and pop 1)
inline size_t stack_lds(int levels) { return (size_t)(3 * levels + 1) * 256 * sizeof(uint32_t); }

// the counters and kernel times of `st` added to `total`, for a call that makes several passes of a solve driver (reserved, the
// deepest stack, is a maximum; solve_ms is the whole call's and left to the caller)
inline void add_stats(wost_stats &total, const wost_stats &st)
{
    total.walk_steps += st.walk_steps; total.walks_started += st.walks_started; total.walks_absorbed += st.walks_absorbed;
    total.walks_truncated += st.walks_truncated; total.neumann_hits += st.neumann_hits; total.inner_visits += st.inner_visits;
    total.leaf_visits += st.leaf_visits; total.trav_trips += st.trav_trips; total.step_trips += st.step_trips;
    total.kernel_ms += st.kernel_ms; total.kernel_launches += st.kernel_launches; total.reserved = std::max(total.reserved, st.reserved);
}

// the mesh build checks: the bytes in which two device arrays of `count` elements differ (all of them when one is missing or a
// copy fails); *compared grows by the bytes looked at
template <class T>
int64_t differing_bytes(const T *a, const T *b, size_t count, int64_t *compared)
{
    if (count == 0) return 0;
    const size_t bytes = count * sizeof(T);
    if (!a || !b) return (a || b) ? (int64_t)bytes : 0;
    std::vector<unsigned char> ha(bytes), hb(bytes);
    if (hipMemcpy(ha.data(), a, bytes, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hb.data(), b, bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return (int64_t)bytes;
    int64_t diff = 0;
    for (size_t i = 0; i < bytes; ++i) diff += ha[i] != hb[i];
    *compared += (int64_t)bytes;
    return diff;
}

#pragma GCC visibility pop

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
