// wost_exits_index.hip -- the index of an exit list by vertex (wost_exits.h; include/wost.h "Exit lists: the index and the ordered
// adjoint"): the transpose of the list, built once per walk of the list so that the adjoints become gathers
// (exits_adjoint_ordered_kernel & co., wost_exits.hip).  An incidence w * DIM + j -- corner j of the primitive of absorbed walk w
// -- belongs to bin 2 v + (side < 0), v the corner's vertex.  One pass counts the absorbed walks in front of each walk (a prefix
// sum: the place of a pair is a function of the records, not of arrival), one writes the (bin, incidence) pairs in ascending
// order of incidence, a stable radix sort by bin keeps that order inside a bin, and the bins' offsets are read off the sorted
// keys.  For a list of the gradient, the mean direction of every point, summed as exits_adjoint_gradient_kernel sums it.  No
// floating-point atomic anywhere: the index is a function of the records alone.  Cold path: once per geometry.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "wost_exits.h"
#include "wost_grad.h"

namespace wost {

namespace {
struct Absorbed {
    __host__ __device__ uint32_t operator()(int32_t slot) const { return slot >= 0 ? 1u : 0u; }
};

// One lane per walk: absorbed walk w, the `before[w]`-th of them, writes its DIM pairs at DIM * before[w].
template <int DIM>
__global__ __launch_bounds__(256) void index_pairs_kernel(ExitRecords rec, const int32_t *verts, const uint32_t *before, size_t N, uint32_t *keys,
                                                          int32_t *vals)
{
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= N) return;
    const int32_t slot = rec.slot()[w];
    if (slot < 0) return;
    const uint32_t minus = rec.side()[w] < 0 ? 1u : 0u;
    const size_t at = (size_t)DIM * before[w];
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
        keys[at + j] = 2u * (uint32_t)verts[(size_t)DIM * slot + j] + minus;
        vals[at + j] = (int32_t)(w * DIM + j);
    }
}

// One lane per offset: bin_begin[b] is the first place of the sorted keys that holds a key >= b (b = 0 .. bins, both ends).
__global__ __launch_bounds__(256) void index_bins_kernel(const uint32_t *keys, int64_t count, int64_t bins, int64_t *bin_begin)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > bins) return;
    int64_t lo = 0, hi = count;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)keys[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    bin_begin[b] = lo;
}

// One wave per point: nbar_a = sum_s n_sa / S, the lanes over s = lane, lane + 64, ..., then the butterfly of wave_sum -- the
// very operations of exits_adjoint_gradient_kernel, so the ordered adjoint centres the directions by the same numbers.
template <int DIM>
__global__ __launch_bounds__(256) void index_nbar_kernel(const float *dirs, int32_t n, int32_t S, double *nbar_out)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= n) return;      // (the whole wave)
    const size_t w0 = (size_t)i * S;
    double nbar[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) nbar[a] = 0.0;
    for (int s = lane; s < S; s += 64) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) nbar[a] += (double)dirs[DIM * (w0 + s) + a];
    }
#pragma unroll
    for (int a = 0; a < DIM; ++a) nbar[a] = wave_sum(nbar[a]) / (double)S;
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) nbar_out[(size_t)DIM * i + a] = nbar[a];
    }
}

// the new index until it stands whole: freed on every other return path
struct IndexGuard {
    ExitIndex x;
    ~IndexGuard() { exits_index_free(x); }
};

int scratch_alloc(Scratch &s, void **p, size_t bytes, const char *what)
{
    const int rc = exits_alloc(p, bytes + 16, what);
    if (rc == WOST_OK) s.ptrs.push_back(*p);
    return rc;
}
}  // namespace

int exits_index_build(const ExitCall &c)
{
    WOST_TRY(hipSetDevice(c.device));
    ExitList &l = *c.list;
    const hipStream_t stream = nullptr;      // the default stream
    const size_t N = (size_t)l.n * l.S, dim = (size_t)c.dim;
    const int64_t bins = 2 * (int64_t)c.n_verts;
    Scratch tmp;
    int rc;
    // the absorbed walks in front of each walk
    uint32_t *before = nullptr;
    void *scan_tmp = nullptr;
    size_t scan_bytes = 0;
    const auto absorbed = rocprim::make_transform_iterator(static_cast<const int32_t *>(l.rec.slot()), Absorbed{});
    WOST_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, absorbed, before, 0u, N, rocprim::plus<uint32_t>(), stream));
    if ((rc = scratch_alloc(tmp, (void **)&before, N * sizeof(uint32_t), "the prefix counts of the index")) != WOST_OK) return rc;
    if ((rc = scratch_alloc(tmp, &scan_tmp, scan_bytes, "the prefix counts of the index")) != WOST_OK) return rc;
    WOST_TRY(rocprim::exclusive_scan(scan_tmp, scan_bytes, absorbed, before, 0u, N, rocprim::plus<uint32_t>(), stream));
    uint32_t before_last = 0;
    int32_t slot_last = -1;
    WOST_TRY(hipMemcpyAsync(&before_last, before + (N - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipMemcpyAsync(&slot_last, l.rec.slot() + (N - 1), sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipStreamSynchronize(stream));
    const size_t count = dim * ((size_t)before_last + (slot_last >= 0 ? 1u : 0u));
    // the index itself: the offsets, the mean directions (eight-byte entries first), the incidences
    IndexGuard fresh;
    ExitIndex &x = fresh.x;
    const size_t n_begin = (size_t)bins + 1, n_nbar = l.dirs ? (size_t)l.n * dim : 0;
    if ((rc = exits_alloc(&x.mem, (n_begin + n_nbar) * 8 + count * 4 + 16, "the index of the exit list")) != WOST_OK) return rc;
    x.bin_begin = static_cast<int64_t *>(x.mem);
    x.nbar = n_nbar ? reinterpret_cast<double *>(x.bin_begin + n_begin) : nullptr;
    x.inc = reinterpret_cast<int32_t *>(x.bin_begin + n_begin + n_nbar);
    x.n_inc = (int64_t)count;
    uint32_t *keys_sorted = nullptr;
    if (count > 0) {
        uint32_t *keys = nullptr;
        int32_t *vals = nullptr;
        void *sort_tmp = nullptr;
        size_t sort_bytes = 0;
        unsigned bits = 1;
        while (bits < 32 && ((uint64_t)1 << bits) < (uint64_t)bins) ++bits;
        WOST_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys, keys_sorted, vals, x.inc, count, 0u, bits, stream));
        if ((rc = scratch_alloc(tmp, (void **)&keys, count * sizeof(uint32_t), "the pairs of the index")) != WOST_OK) return rc;
        if ((rc = scratch_alloc(tmp, (void **)&keys_sorted, count * sizeof(uint32_t), "the pairs of the index")) != WOST_OK) return rc;
        if ((rc = scratch_alloc(tmp, (void **)&vals, count * sizeof(int32_t), "the pairs of the index")) != WOST_OK) return rc;
        if ((rc = scratch_alloc(tmp, &sort_tmp, sort_bytes, "the sort of the index")) != WOST_OK) return rc;
        const dim3 grid((unsigned)((N + 255) / 256));
        if (c.dim == 2) hipLaunchKernelGGL(index_pairs_kernel<2>, grid, dim3(256), 0, stream, l.rec, c.verts, before, N, keys, vals);
        else hipLaunchKernelGGL(index_pairs_kernel<3>, grid, dim3(256), 0, stream, l.rec, c.verts, before, N, keys, vals);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = rocprim::radix_sort_pairs(sort_tmp, sort_bytes, keys, keys_sorted, vals, x.inc, count, 0u, bits, stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(stream);      // (the scratch arrays are freed on return)
            return hip_failed("the pairs of the index and their sort", e);
        }
    }
    hipLaunchKernelGGL(index_bins_kernel, dim3((unsigned)((n_begin + 255) / 256)), dim3(256), 0, stream, keys_sorted, (int64_t)count, bins, x.bin_begin);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && x.nbar) {
        const dim3 grid((unsigned)((l.n + 3) / 4));
        if (c.dim == 2) hipLaunchKernelGGL(index_nbar_kernel<2>, grid, dim3(256), 0, stream, l.dirs, l.n, l.S, x.nbar);
        else hipLaunchKernelGGL(index_nbar_kernel<3>, grid, dim3(256), 0, stream, l.dirs, l.n, l.S, x.nbar);
        e = hipGetLastError();
    }
    std::vector<int64_t> begin(n_begin);
    if (e == hipSuccess) e = hipMemcpyAsync(begin.data(), x.bin_begin, n_begin * sizeof(int64_t), hipMemcpyDeviceToHost, stream);
    const hipError_t done = hipStreamSynchronize(stream);      // (the scratch arrays are freed on return)
    if (e != hipSuccess) return hip_failed("the offsets of the index", e);
    WOST_TRY_AS("hipStreamSynchronize", done);
    for (size_t b = 0; b + 1 < n_begin; ++b) x.longest_bin = std::max(x.longest_bin, begin[b + 1] - begin[b]);
    exits_index_free(l.index);
    l.index = x;
    x = ExitIndex{};
    return WOST_OK;
}

int exits_index_records(const ExitCall &c, int64_t *bin_begin, int32_t *inc)
{
    WOST_TRY(hipSetDevice(c.device));
    const ExitIndex &x = c.list->index;
    const hipStream_t stream = nullptr;
    if (bin_begin) WOST_TRY(hipMemcpyAsync(bin_begin, x.bin_begin, (2 * (size_t)c.n_verts + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    if (inc && x.n_inc > 0) WOST_TRY(hipMemcpyAsync(inc, x.inc, (size_t)x.n_inc * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipStreamSynchronize(stream));
    return WOST_OK;
}

}  // namespace wost
