// wost_carry.hip -- the kernel that closes a continued call of a carried frame solve, and the drivers built on it
// (wost_carry.h; include/wost.h "The continued frame solve").  Cold path: one thread per pixel of the
// frame, once per call; the walk kernels do not know of it.  At the end: the bind of a carried point list, whose
// calls the same kernel closes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>

#include "wost_carry.h"

namespace wost {

enum { CARRY_PICK_NONE = 0, CARRY_PICK_MAP = 1, CARRY_PICK_TOLERANCE = 2 };

struct CarryParams {
    const float *sum;
    uint32_t *n, *batches;
    float *prev, *q;
    const uint8_t *mask;
    int32_t nan_masked;        // a point list: the field of a masked entry (a point that is not finite) is NaN
    int32_t width, n_pixels, shard_index, shard_count;
    // the call that has just walked: m samples (0: none, the kernel only reports and selects) on the pixels of `walked`
    // (nullptr: every pixel)
    int32_t m;
    const uint8_t *walked;
    float *field;              // every owned pixel's sum / n (0 where n is 0); nullptr: not wanted
    float *se;                 // every pixel's three standard errors; nullptr: not wanted
    // the selection for the next call: none, the caller's map `want` (nullptr: every pixel), or the pixels that have not
    // converged and have room for another batch
    int32_t pick;
    const uint8_t *want;
    int32_t batch_spp, min_batches, max_spp;
    float abs_tol, rel_tol;
    uint8_t *sel;              // the selection as a map over the frame
    int32_t *ids;              // ... and as a list of pixel ids (nullptr: not wanted), *count of them
    uint32_t *count;
};

// `walked` and `sel` may be one buffer: a thread reads its pixel's byte before it writes it.
__global__ __launch_bounds__(256) void carry_kernel(CarryParams P)
{
    const int pid = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool picked = false;
    if (pid < P.n_pixels) {
        // ownership: the tile formula of init_kernel and walk3_kernel
        const int px = pid % P.width, py = pid / P.width;
        const int tile = (py >> 3) * ((P.width + 7) >> 3) + (px >> 3);
        const bool owned = (tile % P.shard_count) == P.shard_index;
        const bool live = owned && (P.mask == nullptr || P.mask[pid] != 0);
        uint32_t n = P.n[pid], K = P.batches[pid];
        float s[3], q[3];
        for (int ch = 0; ch < 3; ++ch) {
            s[ch] = P.sum[3 * (size_t)pid + ch];
            q[ch] = P.q[3 * (size_t)pid + ch];
        }
        if (live && P.m > 0 && (P.walked == nullptr || P.walked[pid] != 0)) {
            for (int ch = 0; ch < 3; ++ch) {
                const float b = s[ch] - P.prev[3 * (size_t)pid + ch];
                q[ch] = q[ch] + (b * b) / (float)P.m;
                P.q[3 * (size_t)pid + ch] = q[ch];
                P.prev[3 * (size_t)pid + ch] = s[ch];
            }
            K += 1u;
            n += (uint32_t)P.m;
            P.batches[pid] = K;
            P.n[pid] = n;
        }
        const float N = (float)n;
        if (owned && P.field) {
            // the division of the resolve: a pixel that every call walked keeps the bits of the single solve
            float *f = P.field + 3 * (size_t)pid;
            const float unwalked = P.nan_masked && !live ? __int_as_float(0x7fc00000) : 0.0f;
            for (int ch = 0; ch < 3; ++ch) f[ch] = n > 0u ? s[ch] / N : unwalked;
        }
        if (P.se || P.pick == CARRY_PICK_TOLERANCE) {
            bool converged = K >= (uint32_t)P.min_batches;
            for (int ch = 0; ch < 3; ++ch) {
                float v = q[ch] - (s[ch] * s[ch]) / N;
                v = v < 0.0f ? 0.0f : v;      // (NaN stays NaN)
                const float se = K < 2u ? __int_as_float(0x7f800000) : sqrtf(v / ((float)(K - 1u) * N));
                if (P.se) P.se[3 * (size_t)pid + ch] = se;
                const float tol = fmaxf(P.abs_tol, P.rel_tol * fabsf(s[ch] / N));
                converged = converged && (se <= tol);      // (false for a NaN)
            }
            if (P.pick == CARRY_PICK_TOLERANCE) picked = live && !converged && (int64_t)n + P.batch_spp <= (int64_t)P.max_spp;
        }
        if (P.pick == CARRY_PICK_MAP) picked = live && (P.want == nullptr || P.want[pid] != 0);
        if (P.pick != CARRY_PICK_NONE) P.sel[pid] = picked ? 1 : 0;
    }
    if (P.pick == CARRY_PICK_NONE) return;      // (the whole grid: P is uniform)
    // compaction of the selected ids: ballot + popcount prefix in the wave, the waves' counts through LDS, one atomic per
    // workgroup (with one returning atomic per wave on the one counter a selection of a 1024^2 frame took 190 us, ten times the
    // kernel without a selection: EXPERIMENTS 38)
    __shared__ uint32_t wave_count[4];
    __shared__ uint32_t block_base;
    const int wave = threadIdx.x >> 6;
    const unsigned long long votes = __ballot(picked);
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(votes);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
        block_base = total > 0u ? atomicAdd(P.count, total) : 0u;
    }
    __syncthreads();
    if (picked && P.ids) {
        uint32_t base = block_base;
        for (int k = 0; k < wave; ++k) base += wave_count[k];
        P.ids[base + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull))] = pid;
    }
}

static size_t n_pixels_of(const CarryFrame &f) { return (size_t)f.width * (size_t)f.height; }

void carry_free(CarryState &s)
{
    if (s.mem) (void)hipFree(s.mem);
    if (s.work) (void)hipFree(s.work);
    s = CarryState{};
}

void carry_restart(CarryState &s)
{
    s.done = 0; s.shard_index = 0; s.shard_count = 0;
    s.stale = s.mem != nullptr;
}

// the carried state ready for a call on `stream`: allocated, and zeroed when it is new or stale
static int carry_ready(CarryState &s, const CarryFrame &f, hipStream_t stream)
{
    const size_t n = n_pixels_of(f), bytes = n * 52;
    if (!s.mem) {
        WOST_TRY(hipMalloc(&s.mem, bytes));
        s.rng = static_cast<uint64_t *>(s.mem);
        s.sum = reinterpret_cast<float *>(s.rng + n);
        s.prev = s.sum + 3 * n;
        s.q = s.prev + 3 * n;
        s.n = reinterpret_cast<uint32_t *>(s.q + 3 * n);
        s.batches = s.n + n;
        s.stale = true;
    }
    if (s.stale) {
        WOST_TRY(hipMemsetAsync(s.mem, 0, bytes, stream));
        s.stale = false;
    }
    return WOST_OK;
}

static int carry_work_ready(CarryState &s, const CarryFrame &f)
{
    if (s.work) return WOST_OK;
    const size_t n = n_pixels_of(f), n4 = (n + 3) & ~(size_t)3;
    WOST_TRY(hipMalloc(&s.work, 3 * n * sizeof(float) + n * sizeof(int32_t) + sizeof(uint32_t) + 2 * n4));
    s.se = static_cast<float *>(s.work);
    s.ids = reinterpret_cast<int32_t *>(s.se + 3 * n);
    s.count = reinterpret_cast<uint32_t *>(s.ids + n);
    s.sel = reinterpret_cast<uint8_t *>(s.count + 1);
    s.want = s.sel + n4;
    return WOST_OK;
}

static CarryParams carry_params(const CarryState &s, const CarryFrame &f, int32_t shard_index, int32_t shard_count)
{
    CarryParams P{};
    P.sum = s.sum; P.n = s.n; P.batches = s.batches; P.prev = s.prev; P.q = s.q;
    P.mask = f.mask; P.nan_masked = f.nan_masked ? 1 : 0; P.width = f.width; P.n_pixels = (int32_t)n_pixels_of(f);
    P.shard_index = shard_index; P.shard_count = shard_count;
    P.sel = s.sel; P.ids = s.ids; P.count = s.count;
    return P;
}

// The kernel on `stream`, which is idle again when this returns; *count (not nullptr: P.pick is set) receives the pixels selected.
static int carry_launch(const CarryParams &P, hipStream_t stream, uint32_t *count)
{
    if (P.pick != CARRY_PICK_NONE) WOST_TRY(hipMemsetAsync(P.count, 0, sizeof(uint32_t), stream));
    // (256 threads: the kernel's LDS holds the counts of four waves)
    hipLaunchKernelGGL(carry_kernel, dim3((unsigned)((P.n_pixels + 255) / 256)), dim3(256), 0, stream, P);
    WOST_TRY(hipGetLastError());
    if (count) WOST_TRY(hipMemcpyAsync(count, P.count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipStreamSynchronize(stream));
    return WOST_OK;
}

int carry_check_more(const void *h, const void *field, int32_t more_spp)
{
    if (!h || !field) return set_error(WOST_ERR_INVALID, "null argument");
    if (more_spp < 1 || more_spp > (1 << 20) - 1) return set_error(WOST_ERR_INVALID, "more_spp must be in 1..2^20-1");
    return WOST_OK;
}

int carry_check_shard(int32_t shard_index, int32_t shard_count)
{
    if (shard_count <= 0 || shard_index < 0 || shard_index >= shard_count) return set_error(WOST_ERR_INVALID, "bad shard");
    return WOST_OK;
}

int carry_check_adaptive(const void *h, const wost_adaptive *a, const void *field)
{
    if (!h || !a || !field) return set_error(WOST_ERR_INVALID, "null argument");
    if (a->batch_spp < 1 || a->batch_spp > (1 << 20) - 1) return set_error(WOST_ERR_INVALID, "batch_spp must be in 1..2^20-1");
    if (a->min_batches < 2) return set_error(WOST_ERR_INVALID, "min_batches must be at least 2 (one batch has no variance)");
    if (a->max_spp < a->batch_spp) return set_error(WOST_ERR_INVALID, "max_spp must be at least batch_spp");
    if (!std::isfinite(a->abs_tol) || !std::isfinite(a->rel_tol) || a->abs_tol < 0.0f || a->rel_tol < 0.0f)
        return set_error(WOST_ERR_INVALID, "abs_tol and rel_tol must be finite and not negative");
    return WOST_OK;
}

// what a call checks on the handle before any device work: the shard of the carried solve, the room left under the cap
static int carry_check_call(const CarryState &s, int32_t shard_index, int32_t shard_count, int32_t more_spp, const char *prefix)
{
    if (s.shard_count > 0 && (s.shard_index != shard_index || s.shard_count != shard_count))
        return set_error(WOST_ERR_INVALID, "the carried solve belongs to shard " + std::to_string(s.shard_index) + " of " + std::to_string(s.shard_count) +
                                               " (" + prefix + "solve_restart releases it)");
    if ((int64_t)s.done + more_spp > (1 << 20) - 1)
        return set_error(WOST_ERR_INVALID, "spp_done + more_spp must be at most 2^20-1 (spp_done is " + std::to_string(s.done) + ")");
    return WOST_OK;
}

// a call failed after device work had begun: some pixels' state may be written and others' not -- the carried solve is gone
static int carry_drop(CarryState &s, hipStream_t stream, int rc)
{
    const std::string msg = wost_last_error();
    (void)hipStreamSynchronize(stream);
    carry_restart(s);
    return set_error(rc, msg + " (the carried solve was dropped: spp_done is 0)");
}

static double ms_since(std::chrono::high_resolution_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
}

// one walk and the kernel that closes it; `pick` and the tolerances of P select for the next call
static int carry_walk_and_close(CarryState &s, CarryParams P, int32_t more_spp, const uint8_t *sel, uint32_t n_sel, float *field_dev,
                                hipStream_t stream, wost_stats *st, const CarryWalk &walk, uint32_t *count)
{
    int rc = walk(more_spp, sel, sel ? s.ids : nullptr, n_sel, field_dev, stream, st);
    if (rc != WOST_OK) return carry_drop(s, stream, rc);
    ++s.walks;
    P.m = more_spp; P.walked = sel; P.field = field_dev;
    rc = carry_launch(P, stream, count);
    if (rc != WOST_OK) return carry_drop(s, stream, rc);
    return WOST_OK;
}

int carry_more_where(CarryState &s, const CarryFrame &f, int32_t shard_index, int32_t shard_count, int32_t more_spp, const uint8_t *select,
                     bool select_on_host, float *field_dev, hipStream_t stream, wost_stats *stats, const CarryWalk &walk, const char *prefix)
{
    const auto t0 = std::chrono::high_resolution_clock::now();
    int rc = carry_check_call(s, shard_index, shard_count, more_spp, prefix);
    if (rc != WOST_OK) return rc;
    s.walks = 0;
    WOST_TRY(hipSetDevice(f.device));
    if ((rc = carry_ready(s, f, stream)) != WOST_OK) return rc;
    if (select && (rc = carry_work_ready(s, f)) != WOST_OK) return rc;
    wost_stats st{};
    const CarryParams P = carry_params(s, f, shard_index, shard_count);
    if (!select) {
        // every pixel: wost_solve_more
        if ((rc = carry_walk_and_close(s, P, more_spp, nullptr, 0, field_dev, stream, &st, walk, nullptr)) != WOST_OK) return rc;
    } else {
        if (select_on_host) {
            WOST_TRY(hipMemcpyAsync(s.want, select, n_pixels_of(f), hipMemcpyHostToDevice, stream));
            select = s.want;
        }
        // the selection as the walk wants it -- owned, unmasked pixels only, counted -- and the field of the carried state
        CarryParams S = P;
        S.pick = CARRY_PICK_MAP; S.want = select; S.field = field_dev;
        uint32_t n_sel = 0;
        if ((rc = carry_launch(S, stream, &n_sel)) != WOST_OK) return rc;
        if (n_sel > 0 && (rc = carry_walk_and_close(s, P, more_spp, s.sel, n_sel, field_dev, stream, &st, walk, nullptr)) != WOST_OK) return rc;
    }
    // (every call counts, one with an empty selection too: done is the sum of more_spp since the restart)
    s.done += more_spp; s.shard_index = shard_index; s.shard_count = shard_count;
    st.solve_ms = ms_since(t0);
    if (stats) *stats = st;
    return WOST_OK;
}

int carry_adaptive(CarryState &s, const CarryFrame &f, int32_t shard_index, int32_t shard_count, const wost_adaptive &a, float *field_dev,
                   hipStream_t stream, wost_stats *stats, const CarryWalk &walk, const char *prefix)
{
    const auto t0 = std::chrono::high_resolution_clock::now();
    int rc = carry_check_call(s, shard_index, shard_count, 0, prefix);
    if (rc != WOST_OK) return rc;
    s.walks = 0;
    WOST_TRY(hipSetDevice(f.device));
    if ((rc = carry_ready(s, f, stream)) != WOST_OK) return rc;
    if ((rc = carry_work_ready(s, f)) != WOST_OK) return rc;
    CarryParams P = carry_params(s, f, shard_index, shard_count);
    P.pick = CARRY_PICK_TOLERANCE;
    P.batch_spp = a.batch_spp; P.min_batches = a.min_batches; P.max_spp = a.max_spp; P.abs_tol = a.abs_tol; P.rel_tol = a.rel_tol;
    // the first selection, from the carried state as it stands (a resumed solve starts here), and its field
    CarryParams S = P;
    S.field = field_dev;
    uint32_t n_sel = 0;
    if ((rc = carry_launch(S, stream, &n_sel)) != WOST_OK) return rc;
    s.shard_index = shard_index; s.shard_count = shard_count;
    wost_stats total{};
    while (n_sel > 0) {
        if ((rc = carry_check_call(s, shard_index, shard_count, a.batch_spp, prefix)) != WOST_OK) return rc;
        wost_stats st{};
        if ((rc = carry_walk_and_close(s, P, a.batch_spp, s.sel, n_sel, field_dev, stream, &st, walk, &n_sel)) != WOST_OK) return rc;
        s.done += a.batch_spp;
        add_stats(total, st);
    }
    total.solve_ms = ms_since(t0);
    if (stats) *stats = total;
    return WOST_OK;
}

int carry_read(CarryState &s, const CarryFrame &f, int32_t *spp, int32_t *batches, float *sum_rgb, float *stderr_rgb, hipStream_t stream)
{
    const size_t n = n_pixels_of(f);
    if (!s.mem || s.stale) {
        // nothing carried: no pixel was ever walked
        if (spp) std::memset(spp, 0, n * sizeof(int32_t));
        if (batches) std::memset(batches, 0, n * sizeof(int32_t));
        if (sum_rgb) std::memset(sum_rgb, 0, 3 * n * sizeof(float));
        if (stderr_rgb) std::fill(stderr_rgb, stderr_rgb + 3 * n, INFINITY);
        return WOST_OK;
    }
    WOST_TRY(hipSetDevice(f.device));
    if (stderr_rgb) {
        int rc = carry_work_ready(s, f);
        if (rc != WOST_OK) return rc;
        CarryParams P = carry_params(s, f, 0, 1);
        P.se = s.se;
        if ((rc = carry_launch(P, stream, nullptr)) != WOST_OK) return rc;
        WOST_TRY(hipMemcpyAsync(stderr_rgb, s.se, 3 * n * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
    if (spp) WOST_TRY(hipMemcpyAsync(spp, s.n, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (batches) WOST_TRY(hipMemcpyAsync(batches, s.batches, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (sum_rgb) WOST_TRY(hipMemcpyAsync(sum_rgb, s.sum, 3 * n * sizeof(float), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipStreamSynchronize(stream));
    return WOST_OK;
}

// ---- the carried point list (wost_points_carry & co., wost_carry.h) ----
// the map of the finite points of a list, built once when the list is bound: one thread per point
__global__ __launch_bounds__(256) void points_finite_kernel(const float *pts, int32_t n, int32_t dim, uint8_t *finite)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool ok = true;
    for (int k = 0; k < dim; ++k) ok = ok && isfinite(pts[(size_t)i * dim + k]);
    finite[i] = ok ? 1 : 0;
}

void points_free(PointList &l)
{
    if (l.pts) (void)hipFree(l.pts);      // (one allocation: the points, the field, the map)
    carry_free(l.carry);
    l = PointList{};
}

int points_check_bind(const void *h, const float *pts, int32_t n, int32_t seed_base, int32_t seed_width)
{
    if (!h) return set_error(WOST_ERR_INVALID, "null argument");
    if (n < 0) return set_error(WOST_ERR_INVALID, "negative number of points");
    if (n > 0 && !pts) return set_error(WOST_ERR_INVALID, "null argument");
    if (seed_width <= 0) return set_error(WOST_ERR_INVALID, "seed_width must be positive");
    if (seed_base < 0 || (int64_t)seed_base + n > ((int64_t)1 << 28))
        return set_error(WOST_ERR_INVALID, "seed_base must be >= 0 and seed_base + n at most 2^28");
    return WOST_OK;
}

int points_bind(PointList &l, int device, int dim, const float *pts, bool pts_on_host, int32_t n, int32_t seed_base, int32_t seed_width,
                hipStream_t stream)
{
    if (n == 0) {
        if (l.pts || l.carry.mem || l.carry.work) {
            WOST_TRY(hipSetDevice(device));
            points_free(l);
        }
        l = PointList{};
        return WOST_OK;
    }
    WOST_TRY(hipSetDevice(device));
    // the new list first, whole; the old one goes only when the new one stands
    const size_t n_pts = (size_t)n * (size_t)dim, n_field = (size_t)n * 3;
    void *mem = nullptr;
    WOST_TRY(hipMalloc(&mem, (n_pts + n_field) * sizeof(float) + (size_t)n));
    PointList fresh;
    fresh.pts = static_cast<float *>(mem);
    fresh.field = fresh.pts + n_pts;
    fresh.finite = reinterpret_cast<uint8_t *>(fresh.field + n_field);
    fresh.n = n; fresh.seed_base = seed_base; fresh.seed_width = seed_width;
    hipError_t e = hipMemcpyAsync(fresh.pts, pts, n_pts * sizeof(float), pts_on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(fresh.field, 0, n_field * sizeof(float), stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(points_finite_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, fresh.pts, n, (int32_t)dim, fresh.finite);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        (void)hipFree(mem);
        return hip_failed("binding the point list", e);
    }
    points_free(l);
    l = fresh;
    return WOST_OK;
}

}  // namespace wost
