// wost_grad_carry.hip -- the carried gradient list (wost_grad.h; include/wost.h "The carried gradient list"): the
// accumulate step behind the walks of a block -- per selected point the reduction of wost_solve_gradient_points, rounded as the
// single call rounds it and added to the point's fp64 sums --, the kernel that closes a call -- outputs, convergence and room
// tests, the selection of the next round as a map and as counts per block --, and the drivers of the bind and of the calls.
// Cold path: one wave per point behind the walks, one thread per point at the close; the walk kernels do not know of it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "wost_grad.h"

namespace wost {

#define WOST_NAN __int_as_float(0x7fc00000)

// ---- the kernels -------------------------------------------------------------------------------------------------------------
// the map of the walkable points, built once when the list is bound: one thread per point
__global__ __launch_bounds__(256) void gradlist_walkable_kernel(const float *radius, int32_t n, float eps, uint8_t *walkable)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) walkable[i] = ball_degenerate(radius[i], eps) ? 0 : 1;
}

struct GradAccumParams {
    // the block: count points of spp walks each from point `first` of the list on -- results and directions per walk, radii per point
    const float *w, *dirs, *radius;
    const float *ball;         // the in-ball samples of a list bound to take them (nullptr: none), ball_stride floats apart
    size_t ball_stride;
    const uint8_t *sel;        // over the list: the points this round walks
    int32_t first, count, spp;
    int32_t *K;
    double *G, *Q, *F;
};

// One wave per point of the block; a selected point's batch is reduced by the passes of grad_reduce_kernel (grad_point_sums_from
// over GradWalkArrays and, with in-ball samples, grad_ball_sums), so its fp32 gradient and mean have the bits of the single
// call, and lane 0 adds them to the point's sums.
template <int DIM>
__global__ __launch_bounds__(256) void gradlist_accumulate_kernel(GradAccumParams P)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (j >= P.count) return;      // (the whole wave)
    const size_t i = (size_t)P.first + (size_t)j;
    if (P.sel[i] == 0) return;     // (the whole wave)
    const int S = P.spp;
    double mean[3], t[DIM * 3];
    grad_point_sums_from<DIM>(GradWalkArrays<DIM>{P.w + 3 * (size_t)j * S, P.dirs + DIM * (size_t)j * S}, S, lane, mean, t);
    double a[DIM * 3], u[3];
    if (P.ball) grad_ball_sums<DIM>(P.ball + (size_t)j * S, P.ball_stride, S, lane, a, u);      // (the whole grid: P is uniform)
    if (lane != 0) return;
    const float R = P.radius[j];
    const double scale = grad_scale<DIM>(R, S);
#pragma unroll
    for (int e = 0; e < DIM * 3; ++e) {
        double g = scale * t[e];
        if (P.ball) g += ball_grad_term(R, S, a[e]);
        g = (double)(float)g;
        P.G[(size_t)(DIM * 3) * i + e] += g;
        P.Q[(size_t)(DIM * 3) * i + e] += g * g;
    }
    for (int c = 0; c < 3; ++c) P.F[3 * i + c] += (double)(float)(P.ball ? mean[c] + ball_field_term(R, S, u[c]) : mean[c]);
    P.K[i] += 1;
}

enum { GRAD_PICK_NONE = 0, GRAD_PICK_MAP = 1, GRAD_PICK_TOLERANCE = 2 };

struct GradCloseParams {
    int32_t n, entries, per_block;      // entries = DIM * 3
    const int32_t *K;
    const double *G, *Q, *F;
    const float *radius;
    const uint8_t *walkable;
    // the outputs, nullptr: not wanted
    float *grad, *se, *field, *radius_out;
    int32_t *batches;
    // the selection of the next round: none, the caller's map `want` (nullptr: every point), or the points that have not
    // converged and have room for another batch -- walkable points only
    int32_t pick;
    const uint8_t *want;
    int32_t min_batches, max_batches;
    float abs_tol, rel_tol;
    uint8_t *sel;              // the selection as a map over the list
    uint32_t *counts;          // ... and counted per block of per_block points (zeroed before the launch)
};

// One thread per point: the outputs from the sums, the tests in fp32 on the rounded outputs, the selection.  The counts: a
// ballot per block of the list that has a selected point in the wave, one atomic per wave and such block.
__global__ __launch_bounds__(256) void gradlist_close_kernel(GradCloseParams P)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool picked = false;
    if (i < P.n) {
        const int32_t K = P.K[i];
        const bool walkable = P.walkable[i] != 0;
        const double dK = (double)K;
        bool converged = K >= P.min_batches;
        for (int e = 0; e < P.entries; ++e) {
            const double G = P.G[(size_t)P.entries * i + e], Q = P.Q[(size_t)P.entries * i + e];
            const float g = K > 0 ? (float)(G / dK) : WOST_NAN;
            double v = Q - G * G / dK;
            v = v < 0.0 ? 0.0 : v;
            const float se = !walkable ? WOST_NAN : K < 2 ? __int_as_float(0x7f800000) : (float)sqrt(v / ((dK - 1.0) * dK));
            if (P.grad) P.grad[(size_t)P.entries * i + e] = g;
            if (P.se) P.se[(size_t)P.entries * i + e] = se;
            converged = converged && (se <= fmaxf(P.abs_tol, P.rel_tol * fabsf(g)));      // (false for a NaN)
        }
        if (P.field)
            for (int c = 0; c < 3; ++c) P.field[3 * (size_t)i + c] = K > 0 ? (float)(P.F[3 * (size_t)i + c] / dK) : WOST_NAN;
        if (P.radius_out) P.radius_out[i] = P.radius[i];
        if (P.batches) P.batches[i] = K;
        if (P.pick == GRAD_PICK_TOLERANCE) picked = walkable && !converged && (int64_t)K + 1 <= (int64_t)P.max_batches;
        if (P.pick == GRAD_PICK_MAP) picked = walkable && (P.want == nullptr || P.want[i] != 0);
        if (P.pick != GRAD_PICK_NONE) P.sel[i] = picked ? 1 : 0;
    }
    if (P.pick == GRAD_PICK_NONE) return;      // (the whole grid: P is uniform)
    const int block = i < P.n ? i / P.per_block : 0;
    unsigned long long rest = __ballot(picked);
    while (rest) {
        const int src = __builtin_ctzll(rest);
        const int b = __shfl(block, src);
        const unsigned long long votes = __ballot(picked && block == b);
        if (lane == src) atomicAdd(P.counts + b, (uint32_t)__popcll(votes));
        rest &= ~votes;
    }
}

// ---- the list ----------------------------------------------------------------------------------------------------------------
void gradlist_free(GradList &l)
{
    if (l.mem) (void)hipFree(l.mem);
    for (hipEvent_t e : l.ev)
        if (e) (void)hipEventDestroy(e);
    l = GradList{};
}

void gradlist_restart(GradList &l)
{
    l.rounds = 0;
    l.stale = l.mem != nullptr;
}

static size_t up8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

// the arrays of a list of n points carved from one allocation (mem == nullptr: the bytes it takes)
static size_t gradlist_carve(GradList &l, void *mem)
{
    const size_t n = (size_t)l.n, ne = n * (size_t)l.dim * 3, nb = (size_t)l.n_blocks;
    char *p = static_cast<char *>(mem);
    size_t at = 0;
    auto take = [&](auto *&a, size_t count) {
        if (mem) a = reinterpret_cast<std::remove_reference_t<decltype(a)>>(p + at);
        at += up8(count * sizeof(*a));
    };
    take(l.G, ne); take(l.Q, ne); take(l.F, n * 3);
    take(l.pts, n * (size_t)l.dim); take(l.radius, n); take(l.o_grad, ne); take(l.o_se, ne); take(l.o_field, n * 3);
    take(l.K, n); take(l.counts, nb);
    take(l.walkable, n); take(l.sel, n); take(l.want, n);
    return at;
}

// K and the sums zeroed when the list is new or restarted (G, Q and F are one stretch of the allocation)
static int gradlist_ready(GradList &l, hipStream_t stream)
{
    if (!l.stale) return WOST_OK;
    const size_t n = (size_t)l.n, ne = n * (size_t)l.dim * 3;
    WOST_TRY(hipMemsetAsync(l.G, 0, 2 * up8(ne * sizeof(double)) + up8(n * 3 * sizeof(double)), stream));
    WOST_TRY(hipMemsetAsync(l.K, 0, n * sizeof(int32_t), stream));
    l.stale = false;
    return WOST_OK;
}

int gradlist_check_bind(const void *h, const float *pts, int32_t n, int32_t batch_walks, int32_t round_stride, int32_t max_rounds,
                        int32_t seed_base, int32_t walk_seed_base, int32_t seed_width)
{
    if (!h) return set_error(WOST_ERR_INVALID, "null argument");
    if (n < 0) return set_error(WOST_ERR_INVALID, "negative number of points");
    if (n > 0 && !pts) return set_error(WOST_ERR_INVALID, "null argument");
    if (seed_width <= 0) return set_error(WOST_ERR_INVALID, "seed_width must be positive");
    if (seed_base < 0 || walk_seed_base < 0) return set_error(WOST_ERR_INVALID, "seed_base and walk_seed_base must be >= 0");
    if (batch_walks < 2) return set_error(WOST_ERR_INVALID, "batch_walks must be at least 2 (the estimator needs two walks per point)");
    if (round_stride < n) return set_error(WOST_ERR_INVALID, "round_stride must be at least n (the seeds of two rounds must not meet)");
    if (max_rounds < 1) return set_error(WOST_ERR_INVALID, "max_rounds must be at least 1");
    const int64_t limit = (int64_t)1 << 28, span = ((int64_t)max_rounds - 1) * (int64_t)round_stride + n;
    if ((int64_t)seed_base + span > limit)
        return set_error(WOST_ERR_INVALID, "seed_base + (max_rounds - 1) * round_stride + n (" + std::to_string((int64_t)seed_base + span) +
                                               ") must be at most 2^28");
    // (span <= 2^28 here, so the product stays far inside 64 bits)
    const int64_t walks = span * (int64_t)batch_walks;
    if ((int64_t)walk_seed_base + walks > limit)
        return set_error(WOST_ERR_INVALID, "walk_seed_base + ((max_rounds - 1) * round_stride + n) * batch_walks (" +
                                               std::to_string((int64_t)walk_seed_base + walks) + ") must be at most 2^28");
    if ((int64_t)seed_base < (int64_t)walk_seed_base + walks && (int64_t)walk_seed_base < (int64_t)seed_base + span)
        return set_error(WOST_ERR_INVALID, "the seeds of the directions [seed_base, seed_base + (max_rounds - 1) * round_stride + n) overlap those "
                                           "of the walks, which start at walk_seed_base");
    return WOST_OK;
}

int gradlist_check_out(const void *h, const wost_gradient_carried_out *out)
{
    if (!h || !out || !out->grad) return set_error(WOST_ERR_INVALID, "null argument");
    return WOST_OK;
}

int gradlist_check_adaptive(const void *h, const wost_gradient_adaptive *a, const wost_gradient_carried_out *out)
{
    if (!h || !a || !out || !out->grad) return set_error(WOST_ERR_INVALID, "null argument");
    if (a->min_batches < 2) return set_error(WOST_ERR_INVALID, "min_batches must be at least 2 (one batch has no variance)");
    if (a->max_batches < 1) return set_error(WOST_ERR_INVALID, "max_batches must be at least 1");
    if (!std::isfinite(a->abs_tol) || !std::isfinite(a->rel_tol) || a->abs_tol < 0.0f || a->rel_tol < 0.0f)
        return set_error(WOST_ERR_INVALID, "abs_tol and rel_tol must be finite and not negative");
    return WOST_OK;
}

int gradlist_bind(GradList &l, const GradCall &c, const float *pts, bool pts_on_host, int32_t n, int32_t batch_walks, int32_t round_stride,
                  int32_t max_rounds, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width, hipStream_t stream)
{
    const std::string name = std::string(c.prefix) + "gradient_points_carry: ";
    if ((uint64_t)batch_walks > (uint64_t)c.n_pixels)
        return set_error(WOST_ERR_INVALID, name + "batch_walks (" + std::to_string(batch_walks) + ") exceeds n_pixels (" + std::to_string(c.n_pixels) +
                                               "): a point's walks must fit one point step");
    if (c.has_source && !c.source_term)
        return set_error(WOST_ERR_UNSUPPORTED, name + "a scene with a source term is not covered (the in-ball term of the gradient is not built)");
    WOST_TRY(hipSetDevice(c.device));
    // the new list first, whole; the old one goes only when the new one stands
    GradList fresh;
    fresh.dim = c.dim; fresh.n = n; fresh.S = batch_walks; fresh.round_stride = round_stride; fresh.max_rounds = max_rounds;
    fresh.seed_base = seed_base; fresh.walk_seed_base = walk_seed_base; fresh.seed_width = seed_width;
    fresh.per_block = (int32_t)std::min<size_t>(c.n_pixels / (size_t)batch_walks, (size_t)INT32_MAX);
    fresh.n_blocks = (n + fresh.per_block - 1) / fresh.per_block;
    fresh.stale = true;
    fresh.in_ball = c.in_ball();
    void *mem = nullptr;
    WOST_TRY(hipMalloc(&mem, gradlist_carve(fresh, nullptr)));
    fresh.mem = mem;
    (void)gradlist_carve(fresh, mem);
    hipError_t e = hipSuccess;
    for (hipEvent_t &ev : fresh.ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e == hipSuccess)
        e = hipMemcpyAsync(fresh.pts, pts, (size_t)n * (size_t)c.dim * sizeof(float), pts_on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream);
    int rc = WOST_OK;
    if (e == hipSuccess) {
        // the radius part of the kernel in front, once for the whole list: no walks, no directions
        rc = c.prep(GradPrep{fresh.pts, 0, n, 0, 0, seed_width, c.eps, fresh.radius, nullptr, nullptr, nullptr}, stream);
        if (rc == WOST_OK) {
            hipLaunchKernelGGL(gradlist_walkable_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, fresh.radius, n, c.eps, fresh.walkable);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    else (void)hipStreamSynchronize(stream);
    if (e != hipSuccess || rc != WOST_OK) {
        gradlist_free(fresh);
        return rc != WOST_OK ? rc : hip_failed("binding the gradient list", e);
    }
    gradlist_free(l);
    l = fresh;
    return WOST_OK;
}

// ---- the calls ---------------------------------------------------------------------------------------------------------------
// a call failed after device work had begun: some points' sums may be written and others' not -- the samples are gone
static int gradlist_drop(GradList &l, hipStream_t stream, int rc)
{
    const std::string msg = wost_last_error();
    (void)hipStreamSynchronize(stream);
    gradlist_restart(l);
    return set_error(rc, msg + " (the samples of the gradient list were dropped: rounds_done is 0)");
}

// where the close kernel writes the outputs of a call: a host call's go to the list's own arrays (radius and batches are
// fetched from the state itself), a device call's to the caller's
static GradCloseParams close_params(const GradList &l, bool on_host, const wost_gradient_carried_out &out)
{
    GradCloseParams P{};
    P.n = l.n; P.entries = l.dim * 3; P.per_block = l.per_block;
    P.K = l.K; P.G = l.G; P.Q = l.Q; P.F = l.F; P.radius = l.radius; P.walkable = l.walkable;
    if (on_host) {
        P.grad = l.o_grad; P.se = out.grad_stderr ? l.o_se : nullptr; P.field = out.field_rgb ? l.o_field : nullptr;
    } else {
        P.grad = out.grad; P.se = out.grad_stderr; P.field = out.field_rgb; P.radius_out = out.radius; P.batches = out.batches;
    }
    P.min_batches = 2; P.max_batches = 0;
    P.sel = l.sel; P.counts = l.counts;
    return P;
}

// The kernel on `stream`, which is idle again when this returns; with a selection, counts receives the selected points of
// every block and *total their sum.  kernel_ms grows by the kernel's time.
static int close_launch(GradList &l, const GradCloseParams &P, hipStream_t stream, std::vector<uint32_t> *counts, uint32_t *total, double &kernel_ms)
{
    if (P.pick != GRAD_PICK_NONE) WOST_TRY(hipMemsetAsync(l.counts, 0, (size_t)l.n_blocks * sizeof(uint32_t), stream));
    WOST_TRY(hipEventRecord(l.ev[0], stream));
    hipLaunchKernelGGL(gradlist_close_kernel, dim3((unsigned)((P.n + 255) / 256)), dim3(256), 0, stream, P);
    WOST_TRY(hipGetLastError());
    WOST_TRY(hipEventRecord(l.ev[1], stream));
    if (P.pick != GRAD_PICK_NONE) {
        counts->resize((size_t)l.n_blocks);
        WOST_TRY(hipMemcpyAsync(counts->data(), l.counts, (size_t)l.n_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    WOST_TRY(hipStreamSynchronize(stream));
    float ms = 0.0f;
    WOST_TRY(hipEventElapsedTime(&ms, l.ev[0], l.ev[1]));
    kernel_ms += (double)ms;
    if (P.pick != GRAD_PICK_NONE) {
        *total = 0;
        for (uint32_t k : *counts) *total += k;
    }
    return WOST_OK;
}

// Round r = l.rounds on the selection l.sel: every block that has a selected point runs the kernel in front (the unselected
// points get NaN first points), the point step of one sample per walk, and the accumulate step.
static int gradlist_round(GradList &l, const GradCall &c, const std::vector<uint32_t> &counts, hipStream_t stream, wost_stats &total)
{
    GradScratch &s = *c.scratch;
    const int32_t S = l.S, at = l.rounds * l.round_stride;      // (at + n <= 2^28: the bind checked it)
    for (int32_t b = 0; b < l.n_blocks; ++b) {
        if (counts[(size_t)b] == 0) continue;
        const int32_t a = b * l.per_block, m = std::min(l.per_block, l.n - a), walks = m * S;
        int rc;
        WOST_TRY(hipEventRecord(s.ev[0], stream));
        if ((rc = c.prep(GradPrep{l.pts, a, m, S, l.seed_base + at, l.seed_width, c.eps, s.radius, s.dirs, s.first, l.sel}, stream)) != WOST_OK) return rc;
        if (l.in_ball && (rc = grad_ball_block(c, l.pts, a, m, S, l.seed_base + at, l.seed_width, stream)) != WOST_OK) return rc;
        WOST_TRY(hipEventRecord(s.ev[1], stream));
        WOST_TRY(hipMemsetAsync(s.w, 0, (size_t)walks * 3 * sizeof(float), stream));
        wost_stats st{};
        if ((rc = c.walk(s.first, walks, l.walk_seed_base + (at + a) * S, l.seed_width, s.w, stream, &st)) != WOST_OK) return rc;
        const GradAccumParams ap{s.w, s.dirs, s.radius, l.in_ball ? s.ball : nullptr, s.ball_stride, l.sel, a, m, S, l.K, l.G, l.Q, l.F};
        WOST_TRY(hipEventRecord(s.ev[2], stream));
        if (c.dim == 2) hipLaunchKernelGGL(gradlist_accumulate_kernel<2>, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, stream, ap);
        else hipLaunchKernelGGL(gradlist_accumulate_kernel<3>, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, stream, ap);
        WOST_TRY(hipGetLastError());
        WOST_TRY(hipEventRecord(s.ev[3], stream));
        WOST_TRY(hipEventSynchronize(s.ev[3]));
        float ms_front = 0.0f, ms_behind = 0.0f;
        WOST_TRY(hipEventElapsedTime(&ms_front, s.ev[0], s.ev[1]));
        WOST_TRY(hipEventElapsedTime(&ms_behind, s.ev[2], s.ev[3]));
        add_stats(total, st);
        total.kernel_ms += (double)ms_front + (double)ms_behind;
    }
    ++l.rounds;
    return WOST_OK;
}

// the outputs of a host call, after the close kernel that wrote them (the stream is idle)
static int fetch_outputs(const GradList &l, const wost_gradient_carried_out &out, hipStream_t stream)
{
    const size_t n = (size_t)l.n, ne = n * (size_t)l.dim * 3;
    WOST_TRY(hipMemcpyAsync(out.grad, l.o_grad, ne * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (out.grad_stderr) WOST_TRY(hipMemcpyAsync(out.grad_stderr, l.o_se, ne * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (out.field_rgb) WOST_TRY(hipMemcpyAsync(out.field_rgb, l.o_field, n * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (out.radius) WOST_TRY(hipMemcpyAsync(out.radius, l.radius, n * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (out.batches) WOST_TRY(hipMemcpyAsync(out.batches, l.K, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipStreamSynchronize(stream));
    return WOST_OK;
}

// what every call does before its first kernel
static int gradlist_begin(GradList &l, const GradCall &c, hipStream_t stream)
{
    WOST_TRY(hipSetDevice(c.device));
    int rc = grad_ready(*c.scratch, c.n_pixels, c.dim);
    if (rc == WOST_OK && l.in_ball) rc = grad_ball_ready(*c.scratch, c.n_pixels, c.dim);
    return rc != WOST_OK ? rc : gradlist_ready(l, stream);
}

int gradlist_more(GradList &l, const GradCall &c, const uint8_t *select, bool on_host, const wost_gradient_carried_out &out, hipStream_t stream,
                  wost_stats *stats)
{
    const auto t0 = HostClock::now();
    if (l.rounds >= l.max_rounds)
        return set_error(WOST_ERR_INVALID, std::string(c.prefix) + "gradient_points_more: the list has run its max_rounds (" +
                                               std::to_string(l.max_rounds) + ") rounds");
    int rc = gradlist_begin(l, c, stream);
    if (rc != WOST_OK) return rc;
    if (select && on_host) {
        WOST_TRY(hipMemcpyAsync(l.want, select, (size_t)l.n, hipMemcpyHostToDevice, stream));
        select = l.want;
    }
    wost_stats total{};
    GradCloseParams P = close_params(l, on_host, out);
    P.pick = GRAD_PICK_MAP; P.want = select;
    std::vector<uint32_t> counts;
    uint32_t n_sel = 0;
    if ((rc = close_launch(l, P, stream, &counts, &n_sel, total.kernel_ms)) != WOST_OK) return rc;
    if (n_sel > 0) {
        if ((rc = gradlist_round(l, c, counts, stream, total)) != WOST_OK) return gradlist_drop(l, stream, rc);
        P.pick = GRAD_PICK_NONE;
        if ((rc = close_launch(l, P, stream, nullptr, nullptr, total.kernel_ms)) != WOST_OK) return gradlist_drop(l, stream, rc);
    } else {
        total = wost_stats{};      // an empty selection: zeroed stats
    }
    if (on_host && (rc = fetch_outputs(l, out, stream)) != WOST_OK) return rc;
    if (stats) {
        *stats = total;
        if (n_sel > 0) stamp_solve_ms(stats, t0);
    }
    return WOST_OK;
}

int gradlist_adaptive(GradList &l, const GradCall &c, const wost_gradient_adaptive &a, bool on_host, const wost_gradient_carried_out &out,
                      hipStream_t stream, wost_stats *stats)
{
    const auto t0 = HostClock::now();
    int rc = gradlist_begin(l, c, stream);
    if (rc != WOST_OK) return rc;
    wost_stats total{};
    GradCloseParams P = close_params(l, on_host, out);
    P.pick = GRAD_PICK_TOLERANCE;
    P.min_batches = a.min_batches; P.max_batches = a.max_batches; P.abs_tol = a.abs_tol; P.rel_tol = a.rel_tol;
    // the first selection, from the state as it stands (a resumed call starts here), and its outputs
    std::vector<uint32_t> counts;
    uint32_t n_sel = 0;
    if ((rc = close_launch(l, P, stream, &counts, &n_sel, total.kernel_ms)) != WOST_OK) return rc;
    while (n_sel > 0 && l.rounds < l.max_rounds) {
        if ((rc = gradlist_round(l, c, counts, stream, total)) != WOST_OK) return gradlist_drop(l, stream, rc);
        if ((rc = close_launch(l, P, stream, &counts, &n_sel, total.kernel_ms)) != WOST_OK) return gradlist_drop(l, stream, rc);
    }
    if (on_host && (rc = fetch_outputs(l, out, stream)) != WOST_OK) return rc;
    if (stats) {
        *stats = total;
        stamp_solve_ms(stats, t0);
    }
    return WOST_OK;
}

int gradlist_read(GradList &l, const GradCall &c, const wost_gradient_carried_out &out)
{
    int rc = gradlist_begin(l, c, c.stream);
    if (rc != WOST_OK) return rc;
    GradCloseParams P = close_params(l, true, out);
    double ms = 0.0;
    if ((rc = close_launch(l, P, c.stream, nullptr, nullptr, ms)) != WOST_OK) return rc;
    return fetch_outputs(l, out, c.stream);
}

}  // namespace wost
