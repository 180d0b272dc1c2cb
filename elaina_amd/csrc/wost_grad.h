// wost_grad.h -- the gradient of the solution at a caller's points (wost_solve_gradient_points & co., include/wost.h; DESIGN
// 4.3f), shared by the 2-D and the 3-D context: a kernel in front of the point solve (ball radii, directions, first points), the
// point solve of one sample per walk as it is, and a kernel behind it (the weighted reduction and its error estimate).  Cold
// path beside the walk kernels, which do not know of it.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <functional>

#include "../../include/wost.h"
#include "wost_internal.h"

namespace wost {

struct DevMesh3;      // wost_device3.h
struct DevSource3;

// the first ball stays clear of the Neumann boundary: R = min(dD, kGradNeumannShrink * dN).  Exact in binary; a design constant
constexpr float kGradNeumannShrink = 0.875f;

// The scratch of a handle's gradient calls, sized by the handle (n_pixels walks, what one point step takes), allocated on the
// first call and freed with the handle: per walk its first point and direction (dim floats each) and its result (RGB), per
// point of a block its radius; two pairs of events around the two kernels of a block.  A second allocation, made on the first
// call that takes in-ball samples (a scene with a source term and the handle's "grad_source" on) and on no other: per sample
// its direction, its two weights and the odd and even part of the source at its pair of points -- dim + 8 arrays of n_pixels
// floats (kBall*), so that the samples of a block lie side by side in each.
struct GradScratch {
    void *mem = nullptr;
    float *first = nullptr, *dirs = nullptr, *w = nullptr, *radius = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float *ball = nullptr;
    size_t ball_stride = 0;      // n_pixels
};
void grad_free(GradScratch &s);
// the scratch allocated (the first call of a handle) for blocks of a frame of n_pixels
int grad_ready(GradScratch &s, size_t n_pixels, int dim);
// ... and its in-ball part (the first call of a handle that takes in-ball samples)
int grad_ball_ready(GradScratch &s, size_t n_pixels, int dim);

// ---- what the kernel behind the walks and the accumulate step of the carried list share -------------------------------------
// a point is degenerate -- its walks start at the point itself, its gradient is NaN -- when R is not finite or within the shell
__device__ __forceinline__ bool ball_degenerate(float R, float eps) { return !(R > eps) || !isfinite(R); }

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The first two passes over a point's S walks by the lanes of one wave (all of them call): load(s, W, n) gives the result W
// (RGB) and the direction n of walk s of the point;  mean_c = sum_s W_sc / S  and  t_kc = sum_s n_sk (W_sc - mean_c), in fp64,
// the same on every lane.  Every kernel that reduces a point's walks -- grad_reduce_kernel, gradlist_accumulate_kernel,
// exits_apply_gradient_kernel -- goes through these passes and the third one below, so they agree bit for bit: a lane adds its
// walks s = lane, lane + 64, ... in that order, then the butterfly of wave_sum.
template <int DIM, class LOAD>
__device__ __forceinline__ void grad_point_sums_from(const LOAD &load, int S, int lane, double (&mean)[3], double (&t)[DIM * 3])
{
    const double dS = (double)S;
    for (int c = 0; c < 3; ++c) mean[c] = 0.0;
    for (int s = lane; s < S; s += 64) {
        float W[3], n[DIM];
        load(s, W, n);
        for (int c = 0; c < 3; ++c) mean[c] += (double)W[c];
    }
    for (int c = 0; c < 3; ++c) mean[c] = wave_sum(mean[c]) / dS;
#pragma unroll
    for (int e = 0; e < DIM * 3; ++e) t[e] = 0.0;
    for (int s = lane; s < S; s += 64) {
        float W[3], n[DIM];
        load(s, W, n);
#pragma unroll
        for (int e = 0; e < DIM * 3; ++e) t[e] += (double)n[e / 3] * ((double)W[e % 3] - mean[e % 3]);
    }
#pragma unroll
    for (int e = 0; e < DIM * 3; ++e) t[e] = wave_sum(t[e]);
}
// the third pass,  v_kc = sum_s (n_sk (W_sc - mean_c) - t_kc / S)^2
template <int DIM, class LOAD>
__device__ __forceinline__ void grad_point_variance_from(const LOAD &load, int S, int lane, const double (&mean)[3], const double (&t)[DIM * 3],
                                                         double (&v)[DIM * 3])
{
    const double dS = (double)S;
#pragma unroll
    for (int e = 0; e < DIM * 3; ++e) v[e] = 0.0;
    for (int s = lane; s < S; s += 64) {
        float W[3], n[DIM];
        load(s, W, n);
#pragma unroll
        for (int e = 0; e < DIM * 3; ++e) {
            const double dev = (double)n[e / 3] * ((double)W[e % 3] - mean[e % 3]) - t[e] / dS;
            v[e] += dev * dev;
        }
    }
#pragma unroll
    for (int e = 0; e < DIM * 3; ++e) v[e] = wave_sum(v[e]);
}
// the loader of walks held in arrays: w their results (RGB), d their directions (DIM each), both interleaved per walk
template <int DIM>
struct GradWalkArrays {
    const float *w, *d;
    __device__ __forceinline__ void operator()(int s, float (&W)[3], float (&n)[DIM]) const
    {
        for (int c = 0; c < 3; ++c) W[c] = w[3 * s + c];
        for (int k = 0; k < DIM; ++k) n[k] = d[DIM * s + k];
    }
};
// grad_kc = grad_scale * t_kc, rounded to fp32 once
template <int DIM>
__device__ __forceinline__ double grad_scale(float R, int S) { return (double)DIM / ((double)R * ((double)S - 1.0)); }

// The in-ball samples of a block as grad_ball_kernel leaves them (include/wost.h "In-ball samples"): array a of sample t at
// ball[a * stride + t], t = j * S + s for sample s of point j of the block.  The arrays: the direction m (DIM), then
enum { kBallWg = 0, kBallWu = 1, kBallDs = 2, kBallMs = 5, kBallArrays = 8 };      // ... these, behind the DIM of m
// The pass over a point's S in-ball samples by the lanes of one wave (all of them call; `ball` points at the point's sample 0):
//   a_kc = sum_s wg_s m_sk ds_sc   and   u_c = sum_s wu_s ms_sc,   in fp64, the same on every lane.
// A point that took no samples has zeros there and gets zeros here.
template <int DIM>
__device__ __forceinline__ void grad_ball_sums(const float *ball, size_t stride, int S, int lane, double (&a)[DIM * 3], double (&u)[3])
{
    const float *wg = ball + (DIM + kBallWg) * stride, *wu = ball + (DIM + kBallWu) * stride;
    const float *ds = ball + (DIM + kBallDs) * stride, *ms = ball + (DIM + kBallMs) * stride;
#pragma unroll
    for (int e = 0; e < DIM * 3; ++e) a[e] = 0.0;
    for (int c = 0; c < 3; ++c) u[c] = 0.0;
    for (int s = lane; s < S; s += 64) {
#pragma unroll
        for (int e = 0; e < DIM * 3; ++e) a[e] += (double)wg[s] * (double)ball[(e / 3) * stride + s] * (double)ds[(e % 3) * stride + s];
        for (int c = 0; c < 3; ++c) u[c] += (double)wu[s] * (double)ms[c * stride + s];
    }
#pragma unroll
    for (int e = 0; e < DIM * 3; ++e) a[e] = wave_sum(a[e]);
    for (int c = 0; c < 3; ++c) u[c] = wave_sum(u[c]);
}
// ... and the second pass over them,  va_kc = sum_s (wg_s m_sk ds_sc - a_kc / S)^2
template <int DIM>
__device__ __forceinline__ void grad_ball_variance(const float *ball, size_t stride, int S, int lane, const double (&a)[DIM * 3], double (&va)[DIM * 3])
{
    const double dS = (double)S;
#pragma unroll
    for (int e = 0; e < DIM * 3; ++e) va[e] = 0.0;
    for (int s = lane; s < S; s += 64) {
#pragma unroll
        for (int e = 0; e < DIM * 3; ++e) {
            const double dev = (double)ball[(DIM + kBallWg) * stride + s] * (double)ball[(e / 3) * stride + s] * (double)ball[(DIM + kBallDs + e % 3) * stride + s] -
                               a[e] / dS;
            va[e] += dev * dev;
        }
    }
#pragma unroll
    for (int e = 0; e < DIM * 3; ++e) va[e] = wave_sum(va[e]);
}
// T_kc = (R / S) a_kc joins the walk part of grad, U_c = (R^2 / S) u_c the mean, before the one rounding to fp32
__device__ __forceinline__ double ball_grad_term(float R, int S, double a) { return (double)R / (double)S * a; }
__device__ __forceinline__ double ball_field_term(float R, int S, double u) { return (double)R * (double)R / (double)S * u; }

// The kernel in front of the walks, for `count` points of the caller's list from point `first` on, `spp` walks each: point j of
// the block draws its directions from the stream of pixel seed_base + first + j of a frame seed_width wide.  All pointers on
// the device; radius, dirs and first_pts are the block's (indexed from 0).  sel (a round of the carried gradient list; nullptr:
// every point) is a map over the caller's list: a point whose byte is 0 makes no query and draws nothing, its radius and first
// points are NaN, so the point step never queues its walks.  spp == 0 (the bind of a list): the radii alone.
struct GradPrep {
    const float *pts;
    int32_t first, count, spp, seed_base, seed_width;
    float eps;
    float *radius, *dirs, *first_pts;
    const uint8_t *sel = nullptr;
};
int grad_prep2(const DevMesh &dm, const DevMesh &nm, const GradPrep &p, hipStream_t stream);
int grad_prep3(const DevMesh3 &dm, const DevMesh3 &nm, const GradPrep &p, hipStream_t stream);

// The kernel between the one in front and the walks, on a scene with a source term when the handle's "grad_source" is on: for
// the same `count` points, `spp` in-ball samples each from the same streams, behind the direction draws.  It reads the block's
// radii (a point whose radius is degenerate -- an unselected or a non-finite point's is NaN -- takes no samples and draws
// none: zeros) and writes the block's part of the in-ball arrays (GradScratch::ball, stride floats apart).
struct GradBall {
    const float *pts;
    int32_t first, count, spp, seed_base, seed_width;
    float eps;
    const float *radius;
    float *ball;
    size_t stride;
};
int grad_ball2(const DevSource &src, const GradBall &p, hipStream_t stream);
int grad_ball3(const DevSource3 &src, const GradBall &p, hipStream_t stream);

// What the driver reads of a context, and what a dimension adds: its kernel in front (grad_prep2 / grad_prep3 on its meshes),
// its point step -- one sample at each of the n_walks device points, walk w on the stream of pixel seed_base + w, into w_rgb --
// and the in-ball kernel on its source grid (grad_ball2 / grad_ball3).  source_term: the handle's option "grad_source"; a scene
// with a source term is refused without it and takes in-ball samples with it (in_ball).
struct GradCall {
    const char *prefix;
    int dim, device;
    int32_t spp;
    size_t n_pixels;
    float eps;
    bool has_source, source_term;
    hipStream_t stream;      // the handle's own: where a host call runs
    GradScratch *scratch;
    std::function<int(const GradPrep &, hipStream_t)> prep;
    std::function<int(const float *first_pts, int32_t n_walks, int32_t seed_base, int32_t seed_width, float *w_rgb, hipStream_t stream,
                      wost_stats *stats)>
        walk;
    std::function<int(const GradBall &, hipStream_t)> ball;
    bool in_ball() const { return has_source && source_term; }
};
// the block's in-ball samples behind the kernel in front (the scratch has its in-ball part): sel as in GradPrep, through the radii
int grad_ball_block(const GradCall &c, const float *pts, int32_t first, int32_t count, int32_t spp, int32_t seed_base, int32_t seed_width,
                    hipStream_t stream);

// the option "grad_source" of a handle (wost_set_option, wost3_set_option): exactly 0 or 1
int grad_source_option(double value, bool *option);

// the argument rules that need no look at the handle (include/wost.h), in the order of the header
int grad_check(const void *h, const float *pts, int32_t n, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width,
               const wost_gradient_out *out);
// ... and those that need the handle: its spp setting, its frame, its source term
int grad_check_handle(const GradCall &c, int32_t n, int32_t seed_base, int32_t walk_seed_base);
// the call on device arrays, after both: the blocks
int grad_solve_dev(const GradCall &c, const float *pts_dev, int32_t n, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width,
                   const wost_gradient_out &out_dev, hipStream_t stream, wost_stats *stats);
// ... and on host arrays: the same on the handle's stream, the wanted outputs fetched
int grad_solve_host(const GradCall &c, const float *pts, int32_t n, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width,
                    const wost_gradient_out &out, wost_stats *stats);

// the bodies of the four entry points, written once: H is the context, `call` what it adds (read after the handle-free rules)
template <class H>
int grad_entry(H *h, GradCall (*call)(H *), int dim, const float *pts, bool on_host, int32_t n, int32_t seed_base, int32_t walk_seed_base,
               int32_t seed_width, const wost_gradient_out *out, void *stream, wost_stats *stats)
{
    int rc = grad_check(h, pts, n, seed_base, walk_seed_base, seed_width, out);
    if (rc == WOST_OK && on_host) rc = check_points_finite(pts, n, dim);
    if (rc != WOST_OK) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return WOST_OK;
    const GradCall c = call(h);
    if ((rc = grad_check_handle(c, n, seed_base, walk_seed_base)) != WOST_OK) return rc;
    if (on_host) return grad_solve_host(c, pts, n, seed_base, walk_seed_base, seed_width, *out, stats);
    return grad_solve_dev(c, pts, n, seed_base, walk_seed_base, seed_width, *out, reinterpret_cast<hipStream_t>(stream), stats);
}

// ---- the carried gradient list behind wost_gradient_points_carry & co. (wost_grad_carry.hip) --------------------
// What a handle carries beside the carried frame solve and the carried point list: the library's copy of the caller's points,
// their radii and the map of the walkable ones (both from the bind), per point the batches K and the fp64 sums of the batches'
// fp32 results -- G and Q = sum g, sum g^2 per entry of the gradient, F = sum of the batch means per channel --, the work
// arrays of a call (the selection, a caller's map on its way to the device, the selected points per block, the outputs of a
// host call) and the rounds done.  One allocation; zeroed sums are a fresh list.
struct GradList {
    void *mem = nullptr;
    double *G = nullptr, *Q = nullptr, *F = nullptr;
    float *pts = nullptr, *radius = nullptr, *o_grad = nullptr, *o_se = nullptr, *o_field = nullptr;
    int32_t *K = nullptr;
    uint32_t *counts = nullptr;                  // n_blocks: the selected points of each block of floor(n_pixels / S) points
    uint8_t *walkable = nullptr, *sel = nullptr, *want = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};       // around the close / select kernel
    int dim = 0;
    int32_t n = 0, S = 0, round_stride = 0, max_rounds = 0, seed_base = 0, walk_seed_base = 0, seed_width = 1;
    int32_t per_block = 0, n_blocks = 0, rounds = 0;
    bool stale = false;                          // restarted: K and the sums are zeroed before their next use
    bool in_ball = false;                        // GradCall::in_ball() at the bind: every round takes in-ball samples, or none does
};
void gradlist_free(GradList &l);
void gradlist_restart(GradList &l);

// the argument rules that need no look at the handle (include/wost.h), in the order of the header
int gradlist_check_bind(const void *h, const float *pts, int32_t n, int32_t batch_walks, int32_t round_stride, int32_t max_rounds,
                        int32_t seed_base, int32_t walk_seed_base, int32_t seed_width);
int gradlist_check_out(const void *h, const wost_gradient_carried_out *out);
int gradlist_check_adaptive(const void *h, const wost_gradient_adaptive *a, const wost_gradient_carried_out *out);
// the bind after them (n > 0): the rules that need the handle, then the new list, which replaces the old one when it stands whole
int gradlist_bind(GradList &l, const GradCall &c, const float *pts, bool pts_on_host, int32_t n, int32_t batch_walks, int32_t round_stride,
                  int32_t max_rounds, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width, hipStream_t stream);
// one batch on a selection (select: n bytes on the host or the device, nullptr: every walkable point); out on the same side
int gradlist_more(GradList &l, const GradCall &c, const uint8_t *select, bool on_host, const wost_gradient_carried_out &out, hipStream_t stream,
                  wost_stats *stats);
// batches on the points that have not converged and have room, until none is left or the rounds run out
int gradlist_adaptive(GradList &l, const GradCall &c, const wost_gradient_adaptive &a, bool on_host, const wost_gradient_carried_out &out,
                      hipStream_t stream, wost_stats *stats);
// the state into host arrays
int gradlist_read(GradList &l, const GradCall &c, const wost_gradient_carried_out &out);

// the bodies of the nine entry points, written once: H is the context (device, stream, glist), `call` what a dimension adds
template <class H>
struct GradListCalls {
    GradCall (*call)(H *);
    int dim;

    static int bound(const H *h)
    {
        if (h->glist.n <= 0) return set_error(WOST_ERR_INVALID, "no gradient list is bound to the handle (gradient_points_carry binds one)");
        return WOST_OK;
    }
    // host points travel on the handle's stream, device points on the caller's
    int bind(H *h, const float *pts, bool pts_on_host, int32_t n, int32_t batch_walks, int32_t round_stride, int32_t max_rounds, int32_t seed_base,
             int32_t walk_seed_base, int32_t seed_width, void *stream) const
    {
        int rc = gradlist_check_bind(h, pts, n, batch_walks, round_stride, max_rounds, seed_base, walk_seed_base, seed_width);
        if (rc == WOST_OK && pts_on_host) rc = check_points_finite(pts, n, dim);
        if (rc != WOST_OK) return rc;
        if (n == 0) {
            if (h->glist.mem) {
                WOST_TRY(hipSetDevice(h->device));
                gradlist_free(h->glist);
            }
            return WOST_OK;
        }
        return gradlist_bind(h->glist, call(h), pts, pts_on_host, n, batch_walks, round_stride, max_rounds, seed_base, walk_seed_base, seed_width,
                             pts_on_host ? h->stream : reinterpret_cast<hipStream_t>(stream));
    }
    int more(H *h, const uint8_t *select, bool on_host, const wost_gradient_carried_out *out, void *stream, wost_stats *stats) const
    {
        int rc = gradlist_check_out(h, out);
        if (rc == WOST_OK) rc = bound(h);
        if (rc != WOST_OK) return rc;
        return gradlist_more(h->glist, call(h), select, on_host, *out, on_host ? h->stream : reinterpret_cast<hipStream_t>(stream), stats);
    }
    int adaptive(H *h, const wost_gradient_adaptive *a, bool on_host, const wost_gradient_carried_out *out, void *stream, wost_stats *stats) const
    {
        int rc = gradlist_check_adaptive(h, a, out);
        if (rc == WOST_OK) rc = bound(h);
        if (rc != WOST_OK) return rc;
        return gradlist_adaptive(h->glist, call(h), *a, on_host, *out, on_host ? h->stream : reinterpret_cast<hipStream_t>(stream), stats);
    }
    int carried(H *h, const wost_gradient_carried_out *out) const
    {
        int rc = gradlist_check_out(h, out);
        if (rc == WOST_OK) rc = bound(h);
        if (rc != WOST_OK) return rc;
        return gradlist_read(h->glist, call(h), *out);
    }
    int restart(H *h) const
    {
        if (!h) return set_error(WOST_ERR_INVALID, "null argument");
        const int rc = bound(h);
        if (rc != WOST_OK) return rc;
        gradlist_restart(h->glist);
        return WOST_OK;
    }
    int progress(H *h, int32_t *n_points, int32_t *rounds_done) const
    {
        if (!h || !n_points || !rounds_done) return set_error(WOST_ERR_INVALID, "null argument");
        *n_points = h->glist.n;
        *rounds_done = h->glist.rounds;
        return WOST_OK;
    }
};

}  // namespace wost
