// wost_train.hip -- the training path that GuidedIntegrator<2> and GuidedIntegrator<3> share (wost_train.h): the ordered training
// set of a sample's records, the batch rule and the Adam steps.  gfx950 only.
//
// The reference fills its training set through atomics, in whatever order the threads arrive; here it is ordered by
// (pixel, record) through a prefix sum -- count, scan, scatter -- so two runs, and the CPU restatement the tests compare
// against, see the same batches.
#include <hip/hip_runtime.h>

#include <string>

#include "wost_train.h"
#include "wost_internal3.h"

namespace wost {

// One record of a pixel into registers; false when the training set does not take it: outside scene.aabb, or a NaN in the
// normalised input, the direction, the pdf or the solution, or pdf == 0.  On return out[kSol ..] = |solution / thp| per channel
// (0 where the throughput vanished) and out[kPos ..] = the normalised input.
template <int D>
__device__ __forceinline__ bool record_valid(const TrainSetParams<D> &T, int slot, uint32_t pid, float out[Rec<D>::kFields])
{
    using R = Rec<D>;
#pragma unroll
    for (int f = 0; f < R::kFields; ++f) out[f] = T.rec[((size_t)slot * R::kFields + f) * T.rec_ld + pid];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < D; ++a) inside = inside && T.min[a] <= out[R::kPos + a] && out[R::kPos + a] <= T.max[a];
    if (!inside) return false;
    bool bad = isnan(out[R::kPdf]) || out[R::kPdf] == 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = 0.0f;
        if (fabsf(out[R::kThp]) > 1e-5f) v = out[R::kSol + c] / out[R::kThp];
        out[R::kSol + c] = fabsf(v);
        bad = bad || isnan(out[R::kSol + c]);
    }
#pragma unroll
    for (int a = 0; a < D; ++a) {
        out[R::kPos + a] = 0.5f + (out[R::kPos + a] - T.c[a]) / T.e[a];
        bad = bad || isnan(out[R::kPos + a]) || isnan(out[R::kDir + a]);
    }
    return !bad;
}

// pass 1: samples per training pixel -> per-block sums; pass 3: scatter at the scanned offsets
template <int D, bool SCATTER>
__global__ __launch_bounds__(256) void train_set_kernel(TrainSetParams<D> T)
{
    using R = Rec<D>;
    __shared__ uint32_t sh[256];
    const int t = blockIdx.x * 256 + threadIdx.x;
    uint32_t cnt = 0;
    uint32_t pid = 0, depth = 0;
    if (t < T.n_train_pixels) {
        pid = T.train_offset + (uint32_t)t * T.train_stride;
        depth = min(T.cur_depth[pid], (uint32_t)kMaxTrainDepth);
    }
    float r[kMaxTrainDepth][R::kFields];
    bool ok[kMaxTrainDepth];
#pragma unroll
    for (int k = 0; k < kMaxTrainDepth; ++k) {
        ok[k] = (uint32_t)k < depth && record_valid<D>(T, k, pid, r[k]);
        cnt += ok[k] ? 1u : 0u;
    }
    // block-level exclusive scan of cnt
    sh[threadIdx.x] = cnt;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        uint32_t v = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0u;
        __syncthreads();
        sh[threadIdx.x] += v;
        __syncthreads();
    }
    if (!SCATTER) {
        if (threadIdx.x == 255) T.block_sums[blockIdx.x] = sh[255];
        return;
    }
    size_t o = (size_t)T.block_sums[blockIdx.x] + (sh[threadIdx.x] - cnt);
#pragma unroll
    for (int k = 0; k < kMaxTrainDepth; ++k) {
        if (!ok[k]) continue;
        const float *q = r[k];
#pragma unroll
        for (int a = 0; a < D; ++a) {
            T.ts.x[D * o + a] = q[R::kPos + a];
            T.ts.dir[D * o + a] = q[R::kDir + a];
            T.ts.nrm[D * o + a] = q[R::kNrm + a];
        }
        T.ts.sol[3 * o] = q[0]; T.ts.sol[3 * o + 1] = q[1]; T.ts.sol[3 * o + 2] = q[2];
        T.ts.li[o] = (q[0] + q[1] + q[2]) / 3.0f;      // Color::mean() (train.h:519)
        T.ts.pdf[o] = q[R::kPdf];
        T.ts.onn[o] = q[R::kOnN] != 0.0f ? 1 : 0;
        ++o;
    }
}

// pass 2: exclusive scan of the block sums by one block; block_sums[n_blocks] = total
__global__ __launch_bounds__(256) void train_scan_kernel(uint32_t *block_sums, int n_blocks)
{
    __shared__ uint32_t sh[256];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n_blocks; base += 256) {
        const int i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? block_sums[i] : 0u;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            uint32_t a = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0u;
            __syncthreads();
            sh[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < n_blocks) block_sums[i] = carry + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 0) carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sums[n_blocks] = carry;
}

__global__ void resolve_kernel(const float *sol, int n, float spp, float *field)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * n) field[i] = sol[i] / spp;
}

__global__ void resolve_points_kernel(const float *sol, const float *points, int dim, int n, float spp, float *field)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool finite = true;
    for (int a = 0; a < dim; ++a) finite = finite && isfinite(points[(size_t)dim * i + a]);
    for (int k = 0; k < 3; ++k) field[3 * (size_t)i + k] = finite ? sol[3 * (size_t)i + k] / spp : __builtin_nanf("");
}

template <int D>
int enqueue_train_set(const TrainSetParams<D> &T, int n_blocks, hipStream_t st, uint32_t *host_total)
{
    hipLaunchKernelGGL((train_set_kernel<D, false>), dim3(n_blocks), dim3(256), 0, st, T);
    hipLaunchKernelGGL(train_scan_kernel, dim3(1), dim3(256), 0, st, T.block_sums, n_blocks);
    hipLaunchKernelGGL((train_set_kernel<D, true>), dim3(n_blocks), dim3(256), 0, st, T);
    WOST_TRY(hipGetLastError());
    WOST_TRY(hipMemcpyAsync(host_total, T.block_sums + n_blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return WOST_OK;
}

size_t batch_len(size_t n, size_t it, const TrainSchedule &s)
{
    const size_t bs = (size_t)s.batch_size;
    if (it * bs > n) return 0;
    const size_t local = std::min(n - it * bs, bs) / 128 * 128;
    return local < (size_t)s.min_batch_size ? 0 : local;
}

template <int D>
int train_passes(wost_net_handle net, const TrainSet &ts, size_t n, const TrainSchedule &s, const TrainSync &sync, hipStream_t st,
                 uint32_t &launches)
{
    const size_t bs = (size_t)s.batch_size;
    size_t n_batches = std::min<size_t>(n / bs + 1, (size_t)s.batches_per_spp);
    if (sync.fn) {
        // shared network: every rank must take the same number of steps -- the smallest number of full batches any rank has
        int64_t vmin = 0;
        while ((size_t)vmin < n_batches && batch_len(n, (size_t)vmin, s)) ++vmin;
        if (sync.fn(sync.user, WOST_SYNC_MIN_I64_HOST, &vmin, 1) != 0) return set_error(WOST_ERR_DEVICE, "sync callback failed (batch count)");
        n_batches = (size_t)std::max<int64_t>(vmin, 0);
    }
    for (size_t it = 0; it < n_batches; ++it) {
        const size_t local = batch_len(n, it, s), o = it * bs;
        if (!local) break;
        float *raw = nullptr, *dl = nullptr;
        int rc = net_forward_train_dev(net, ts.x + D * o, (int)local, st, &raw, &dl);
        if (rc != WOST_OK) return rc;
        if constexpr (D == 2) launch_vmm_loss_gradients(st, raw, ts.dir + D * o, ts.li + o, ts.pdf + o, ts.onn + o, ts.nrm + D * o, (int)local, s.loss_scale, dl, nullptr);
        else launch_vmm3_loss_gradients(st, raw, ts.dir + D * o, ts.li + o, ts.pdf + o, ts.onn + o, ts.nrm + D * o, (int)local, s.loss_scale, dl, nullptr);
        ++launches;      // the loss-gradient kernel; the network's own launches are counted by the network
        rc = net_backward_update_dev(net, ts.x + D * o, (int)local, s.loss_scale, sync.fn ? 0 : 1, st);
        if (rc != WOST_OK) return rc;
        if (!sync.fn) continue;
        // sum the fixed-point gradients of all ranks (integer sums: the same network everywhere, bit for bit), then step
        WOST_TRY(hipStreamSynchronize(st));
        uint64_t count = 0;
        void *gbuf = net_gradient_buffer(net, &count);
        if (sync.fn(sync.user, WOST_SYNC_SUM_I64_DEVICE, gbuf, count) != 0)
            return set_error(WOST_ERR_DEVICE, "sync callback failed (gradient all-reduce)");
        rc = net_apply_update_dev(net, s.loss_scale, st);
        if (rc != WOST_OK) return rc;
    }
    return WOST_OK;
}

template int enqueue_train_set<2>(const TrainSetParams<2> &, int, hipStream_t, uint32_t *);
template int enqueue_train_set<3>(const TrainSetParams<3> &, int, hipStream_t, uint32_t *);
template int train_passes<2>(wost_net_handle, const TrainSet &, size_t, const TrainSchedule &, const TrainSync &, hipStream_t, uint32_t &);
template int train_passes<3>(wost_net_handle, const TrainSet &, size_t, const TrainSchedule &, const TrainSync &, hipStream_t, uint32_t &);

void launch_resolve(const float *sol, int n, float spp, float *field, hipStream_t st)
{
    hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)((3 * (size_t)n + 255) / 256)), dim3(256), 0, st, sol, n, spp, field);
}

void launch_resolve_points(const float *sol, const float *points, int dim, int n, float spp, float *field, hipStream_t st)
{
    hipLaunchKernelGGL(resolve_points_kernel, dim3((unsigned)(((size_t)n + 255) / 256)), dim3(256), 0, st, sol, points, dim, n, spp, field);
}

hipError_t alloc_train_set(std::vector<void *> &allocs, TrainSet &ts, int dim, size_t capacity)
{
    const size_t M = capacity, d = (size_t)dim;
    hipError_t e = device_alloc(allocs, &ts.x, d * M);
    if (e == hipSuccess) e = device_alloc(allocs, &ts.dir, d * M);
    if (e == hipSuccess) e = device_alloc(allocs, &ts.sol, 3 * M);
    if (e == hipSuccess) e = device_alloc(allocs, &ts.li, M);
    if (e == hipSuccess) e = device_alloc(allocs, &ts.pdf, M);
    if (e == hipSuccess) e = device_alloc(allocs, &ts.nrm, d * M);
    if (e == hipSuccess) e = device_alloc(allocs, &ts.onn, M);
    return e;
}

int copy_train_set(const TrainSet &ts, int dim, size_t m, float *x, float *dir, float *solution, float *dir_pdf, float *normal,
                   uint8_t *on_neumann)
{
    const size_t d = (size_t)dim;
    if (m == 0) return WOST_OK;
    if (x) WOST_TRY(hipMemcpy(x, ts.x, m * d * sizeof(float), hipMemcpyDeviceToHost));
    if (dir) WOST_TRY(hipMemcpy(dir, ts.dir, m * d * sizeof(float), hipMemcpyDeviceToHost));
    if (solution) WOST_TRY(hipMemcpy(solution, ts.sol, m * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (dir_pdf) WOST_TRY(hipMemcpy(dir_pdf, ts.pdf, m * sizeof(float), hipMemcpyDeviceToHost));
    if (normal) WOST_TRY(hipMemcpy(normal, ts.nrm, m * d * sizeof(float), hipMemcpyDeviceToHost));
    if (on_neumann) WOST_TRY(hipMemcpy(on_neumann, ts.onn, m, hipMemcpyDeviceToHost));
    return WOST_OK;
}

}  // namespace wost
