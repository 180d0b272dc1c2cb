// wost_order_probe.hip -- TEST INFRASTRUCTURE ONLY: runs the product's walk orders (csrc/wost_order.h) on keys a test chose
// (tests/test_walk_order.py).  Second unit of elaina_amd/lib/libwost_probe.so; build_probe() links it with a second compile
// of the product's own csrc/wost_order.hip, so the key kernels and the sort are the product's: no body is restated here.
// One open handle serves many runs, as in the product: the scratch is sized once for `cap` walkers and reused.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <new>

#include "../../elaina_amd/csrc/wost_order.h"

namespace {

struct OrderProbe {
    wost::WalkOrder order;
    float *in = nullptr;       // the keys of a run on the device, grown when a run brings more
    size_t in_cap = 0;
    int device = 0;
};

constexpr int kProbeBadOrderPointer = -2;     // *order_out points at neither of the handle's value buffers

}  // namespace

// A WalkOrder for `cap` walkers on `device`.  Returns a hipError_t as int; *out is the handle, or null.
extern "C" int wost_order_probe_open(int device, uint64_t cap, void **out)
{
    if (!out) return (int)hipErrorInvalidValue;
    *out = nullptr;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return (int)e;
    OrderProbe *p = new (std::nothrow) OrderProbe;
    if (!p) return (int)hipErrorOutOfMemory;
    p->device = device;
    const int rc = wost::order_alloc(p->order, (size_t)cap);
    if (rc != (int)hipSuccess) {
        delete p;
        return rc;
    }
    *out = p;
    return (int)hipSuccess;
}

extern "C" uint64_t wost_order_probe_cap(void *handle) { return handle ? (uint64_t)((OrderProbe *)handle)->order.cap : 0; }

// One run: both value buffers of the handle are filled with 0xFFFFFFFF, the n floats of `in` go to the device, and
// order_by_distance (which = 0) or order_by_estimate (which = 1) runs on them.  *rc_out is what that function returned.
// `out` receives all cap entries of the buffer *order_out points into (of the second value buffer when the function left
// *order_out alone), `out_other` (may be null) those of the other buffer.  Returns the hipError_t of the probe's own calls.
extern "C" int wost_order_probe_run(void *handle, int32_t which, const float *in, uint32_t n, int32_t *rc_out, uint32_t *out, uint32_t *out_other)
{
    OrderProbe *p = (OrderProbe *)handle;
    if (!p || (which != 0 && which != 1) || (n > 0 && !in) || !rc_out) return (int)hipErrorInvalidValue;
    const size_t cap = p->order.cap;
    if (cap > 0 && !out) return (int)hipErrorInvalidValue;
    hipError_t e = hipSetDevice(p->device);
    if (e != hipSuccess) return (int)e;
    if (n > p->in_cap) {
        if (p->in) (void)hipFree(p->in);
        p->in = nullptr;
        p->in_cap = 0;
        e = hipMalloc((void **)&p->in, (size_t)n * sizeof(float));
        if (e != hipSuccess) return (int)e;
        p->in_cap = n;
    }
    if (n > 0) e = hipMemcpy(p->in, in, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
    for (int k = 0; k < 2 && e == hipSuccess && cap > 0; ++k) e = hipMemset(p->order.vals[k], 0xff, cap * sizeof(uint32_t));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return (int)e;
    const uint32_t *ord = nullptr;
    *rc_out = which == 0 ? wost::order_by_distance(p->order, p->in, n, (hipStream_t)0, &ord)
                         : wost::order_by_estimate(p->order, p->in, n, (hipStream_t)0, &ord);
    e = hipDeviceSynchronize();
    if (e != hipSuccess) return (int)e;
    if (cap == 0) return (int)hipSuccess;
    int k = 1;
    if (ord) {
        if (ord == p->order.vals[0]) k = 0;
        else if (ord != p->order.vals[1]) return kProbeBadOrderPointer;
    }
    e = hipMemcpy(out, p->order.vals[k], cap * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_other) e = hipMemcpy(out_other, p->order.vals[k ^ 1], cap * sizeof(uint32_t), hipMemcpyDeviceToHost);
    return (int)e;
}

extern "C" int wost_order_probe_close(void *handle)
{
    OrderProbe *p = (OrderProbe *)handle;
    if (!p) return (int)hipSuccess;
    (void)hipSetDevice(p->device);
    wost::order_free(p->order);
    if (p->in) (void)hipFree(p->in);
    delete p;
    return (int)hipSuccess;
}
