// wost_probe.hip -- TEST INFRASTRUCTURE ONLY: evaluates the product's deterministic math functions
// at arguments a test chose (tests/test_device_math.py).  Not part of libwost_hip.so; built into
// elaina_amd/lib/libwost_probe.so by elaina_amd.build.build_probe() with the flags of the product
// library, so that what runs here is what the walk kernels inline.  Every function comes from
// the product's own headers; no body is restated.  gfx950 only.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../elaina_amd/csrc/wost_math.h"
#include "../../elaina_amd/csrc/wost_device3.h"        // cbrt01
#include "../../elaina_amd/csrc/wost_vmm_device.h"     // pcg_next_double, vm_proposal_r

namespace {

using namespace wost;

// function numbers: tests/device_probe.py and oracle/wost_probe.c use the same table
enum {
    FN_SINCOS_2PI = 0,   // f32 -> 2 f32 (cos, sin)
    FN_LOGF = 1,         // f32 -> f32
    FN_EXPF = 2,         // f32 -> f32
    FN_SINCOSF = 3,      // f32 -> 2 f32 (cos, sin)
    FN_CBRT01 = 4,       // f32 -> f32
    FN_COSPI_D = 5,      // f64 -> f64
    FN_ACOS_D = 6,       // f64 -> f64
    FN_LOG_D = 7,        // f64 -> f64
    FN_PCG = 8,          // 3 u64 (initstate, initseq, delta) -> 8 u64
    FN_PROPOSAL_R = 9,   // f32 -> f64
    FN_COUNT = 10
};

__host__ __device__ inline int in_bytes(int fn) { return fn == FN_PCG ? 24 : (fn >= FN_COSPI_D && fn <= FN_LOG_D) ? 8 : 4; }
__host__ __device__ inline int out_bytes(int fn)
{
    if (fn == FN_PCG) return 64;
    if (fn == FN_SINCOS_2PI || fn == FN_SINCOSF) return 8;
    if (fn == FN_LOGF || fn == FN_EXPF || fn == FN_CBRT01) return 4;
    return 8;
}

__global__ void __launch_bounds__(256) probe_kernel(int fn, const void *in, long long n, void *out)
{
    const float *fi = (const float *)in;
    const double *di = (const double *)in;
    const uint64_t *ui = (const uint64_t *)in;
    float *fo = (float *)out;
    double *dout = (double *)out;
    uint64_t *uo = (uint64_t *)out;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        switch (fn) {
        case FN_SINCOS_2PI: {
            float c, s;
            sincos_2pi(fi[i], c, s);
            fo[2 * i] = c;
            fo[2 * i + 1] = s;
            break;
        }
        case FN_LOGF: fo[i] = det_logf(fi[i]); break;
        case FN_EXPF: fo[i] = det_expf(fi[i]); break;
        case FN_SINCOSF: {
            float c, s;
            det_sincosf(fi[i], &c, &s);
            fo[2 * i] = c;
            fo[2 * i + 1] = s;
            break;
        }
        case FN_CBRT01: fo[i] = cbrt01(fi[i]); break;
        case FN_COSPI_D: dout[i] = det_cospi_d(di[i]); break;
        case FN_ACOS_D: dout[i] = det_acos_d(di[i]); break;
        case FN_LOG_D: dout[i] = det_log_d(di[i]); break;
        case FN_PCG: {
            Pcg r;
            pcg_set_seed(r, ui[3 * i], ui[3 * i + 1]);
            uo[8 * i + 0] = r.state;
            uo[8 * i + 1] = r.inc;
            uo[8 * i + 2] = pcg_next_uint(r);
            uo[8 * i + 3] = __float_as_uint(pcg_next_float(r));
            uo[8 * i + 4] = (uint64_t)__double_as_longlong(pcg_next_double(r));
            uo[8 * i + 5] = r.state;
            pcg_advance(r, (int64_t)ui[3 * i + 2]);
            uo[8 * i + 6] = r.state;
            pcg_skip2(r);
            uo[8 * i + 7] = r.state;
            break;
        }
        case FN_PROPOSAL_R: dout[i] = vm_proposal_r(fi[i]); break;
        default: break;
        }
    }
}

}  // namespace

// Copies n arguments of function fn to the device, evaluates them, copies the results back.
// Returns the hipError_t of the first call that failed (hipErrorInvalidValue for a bad argument).
extern "C" int wost_probe_run(int device, int32_t fn, const void *in, int64_t n, void *out)
{
    if (fn < 0 || fn >= FN_COUNT || n < 0 || (n > 0 && (!in || !out))) return (int)hipErrorInvalidValue;
    if (n == 0) return (int)hipSuccess;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return (int)e;
    const size_t nin = (size_t)n * in_bytes(fn), nout = (size_t)n * out_bytes(fn);
    void *din = nullptr, *dout = nullptr;
    e = hipMalloc(&din, nin);
    if (e == hipSuccess) e = hipMalloc(&dout, nout);
    if (e == hipSuccess) e = hipMemcpy(din, in, nin, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const long long blocks = (n + 255) / 256;
        hipLaunchKernelGGL(probe_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, 0, (int)fn, din,
                           (long long)n, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, nout, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return (int)e;
}
