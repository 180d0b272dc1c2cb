// wost_grad.hip -- the gradient of the solution at a caller's points (wost_grad.h; include/wost.h "The gradient at the caller's
// points"): the kernel in front of the point solve -- per point the radius of its first ball, per walk a direction
// and the first point on that ball -- in 2-D and 3-D, the kernel behind it -- per point the weighted reduction of its walks'
// results and the standard error of that estimate --, and the driver that cuts a call into blocks of floor(n_pixels / spp)
// points.  Cold path: one thread per point in front, one wave per point behind; the walk kernels do not know of it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>

#include "wost_device3.h"
#include "wost_grad.h"
#include "wost_walk.h"

namespace wost {

#define WOST_NAN __int_as_float(0x7fc00000)

// ---- the kernel in front ------------------------------------------------------------------------------------------------------
constexpr int kPrepThreads = 256;

// What a dimension adds to the kernel in front and the in-ball kernel.  The distance of a point to a mesh as wost_closest_point /
// wost3_closest_point answers it, at any distance from the mesh (closest_point_lockstep, closest_triangle_lockstep: all lanes
// of the wave call; an empty mesh: +inf); col is the thread's stack column in a block of kPrepThreads.
__device__ __forceinline__ float mesh_distance(const DevMesh &m, const float (&x)[2], bool active, uint32_t *col)
{
    return sqrtf(closest_point_lockstep(m, x[0], x[1], active, col, kPrepThreads).d2);
}
__device__ __forceinline__ float mesh_distance(const DevMesh3 &m, const float (&x)[3], bool active, uint32_t *col)
{
    return sqrtf(closest_triangle_lockstep(m, v3(x[0], x[1], x[2]), active, LdsColumn(col, kPrepThreads)).d2);
}
// A uniform direction from the stream: in 2-D one draw, (cos, sin) of sincos_2pi(u); in 3-D two, u1 then u2, the walk's own
// uniform direction (step3_b0).
template <int DIM>
__device__ __forceinline__ void draw_direction(Pcg &rng, float (&n)[DIM])
{
    float c, sn;
    if (DIM == 2) {
        sincos_2pi(pcg_next_float(rng), c, sn);
        n[0] = c; n[1] = sn;
    } else {
        const float u1 = pcg_next_float(rng), u2 = pcg_next_float(rng);
        sincos_2pi(u2, c, sn);
        const float z = 1 - 2 * u1, r = sqrtf(1 - z * z);
        n[0] = r * c; n[1] = r * sn; n[DIM - 1] = z;
    }
}

// R = min(dD, 0.875 dN) (degenerate or not: ball_degenerate, wost_grad.h)
__device__ __forceinline__ float ball_radius(float dD, float dN) { return fminf(dD, kGradNeumannShrink * dN); }

template <class MESH>
struct GradPrepParams {
    MESH dm, nm;
    GradPrep p;
};

// Thread j takes point first + j of the call: its radius, then spp draws from the stream of pixel seed_base + first + j --
// walk s of the point gets the direction n of draw_direction and the first point fmaf(R, n, x) (madd3 in 3-D).  A point with a
// non-finite coordinate makes no query; its radius and first points are NaN, so the point step never queues its walks.  The
// same holds for a point that the map of a carried list's round (GradPrep::sel) leaves out; it draws nothing either.
template <int DIM, class MESH>
__global__ __launch_bounds__(kPrepThreads) void grad_prep_kernel(GradPrepParams<MESH> P)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t *col = lds_stack + threadIdx.x;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool owned = j < P.p.count;
    float x[DIM];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        x[k] = owned ? P.p.pts[DIM * (size_t)(P.p.first + j) + k] : 0.0f;
        finite = finite && isfinite(x[k]);
    }
    const bool chosen = owned && (P.p.sel == nullptr || P.p.sel[P.p.first + j] != 0);
    const float dD = mesh_distance(P.dm, x, chosen && finite, col);
    const float dN = mesh_distance(P.nm, x, chosen && finite, col);
    if (!owned) return;
    float *dirs = P.p.dirs + DIM * (size_t)j * P.p.spp, *fp = P.p.first_pts + DIM * (size_t)j * P.p.spp;
    if (!chosen) {
        P.p.radius[j] = WOST_NAN;
        for (int s = 0; s < DIM * P.p.spp; ++s) fp[s] = WOST_NAN;
        return;
    }
    const float R = finite ? ball_radius(dD, dN) : WOST_NAN;
    const bool degenerate = ball_degenerate(R, P.p.eps);
    P.p.radius[j] = R;
    Pcg rng{0, 1};
    pcg_seed_pixel(rng, P.p.seed_base + P.p.first + j, P.p.seed_width);
    for (int s = 0; s < P.p.spp; ++s) {
        float n[DIM];
        draw_direction<DIM>(rng, n);
        float f[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) f[k] = !finite ? WOST_NAN : degenerate ? x[k] : __builtin_fmaf(R, n[k], x[k]);
        // (the direction whole, then the first point whole: stores to the two arrays in turn are not merged into wide ones)
#pragma unroll
        for (int k = 0; k < DIM; ++k) dirs[DIM * s + k] = n[k];
#pragma unroll
        for (int k = 0; k < DIM; ++k) fp[DIM * s + k] = f[k];
    }
}

// the launch, with the stack columns of a block for the deeper of the two trees (levels of an empty mesh: 1)
template <int DIM, class MESH>
static int grad_prep_launch(const MESH &dm, int32_t levels_d, const MESH &nm, int32_t levels_n, const GradPrep &p, hipStream_t stream)
{
    const GradPrepParams<MESH> P{dm, nm, p};
    hipLaunchKernelGGL((grad_prep_kernel<DIM, MESH>), dim3((unsigned)((p.count + kPrepThreads - 1) / kPrepThreads)), dim3(kPrepThreads),
                       stack_lds(std::max(levels_d, levels_n)), stream, P);
    WOST_TRY(hipGetLastError());
    return WOST_OK;
}

int grad_prep2(const DevMesh &dm, const DevMesh &nm, const GradPrep &p, hipStream_t stream)
{
    return grad_prep_launch<2>(dm, dm.n_segs > 0 ? dm.levels : 1, nm, nm.n_segs > 0 ? nm.levels : 1, p, stream);
}

int grad_prep3(const DevMesh3 &dm, const DevMesh3 &nm, const GradPrep &p, hipStream_t stream)
{
    return grad_prep_launch<3>(dm, dm.n_tris > 0 ? dm.levels : 1, nm, nm.n_tris > 0 ? nm.levels : 1, p, stream);
}

// ---- the in-ball kernel --------------------------------------------------------------------------------------------------------
// the source at a point, intensity included, by the walk step's own functions
__device__ __forceinline__ void ball_source(const DevSource &src, const float (&y)[2], float (&f)[3]) { source_eval(src, y[0], y[1], f[0], f[1], f[2]); }
__device__ __forceinline__ void ball_source(const DevSource3 &src, const float (&y)[3], float (&f)[3]) { source3_eval(src, v3(y[0], y[1], y[2]), f); }

template <class SRC>
struct GradBallParams {
    SRC src;
    GradBall p;
};

// Thread t takes in-ball sample s = t % spp of point j = t / spp of the block.  It jumps to its place in the stream of pixel
// seed_base + first + j -- behind the spp direction draws of the kernel in front, DIM - 1 floats each, and the s samples before
// its own, DIM floats each --, draws a direction m by that kernel's draw_direction and rho, and evaluates the source at the pair
// x +- rho R m: every operation a single fp32 one in the order of include/wost.h ("In-ball samples"), no fused multiply-add.
// A point whose radius is degenerate (NaN for an unselected and for a non-finite point) draws nothing: zeros.
template <int DIM, class SRC>
__global__ __launch_bounds__(256) void grad_ball_kernel(GradBallParams<SRC> P)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)P.p.count * P.p.spp) return;
    const int j = (int)(t / P.p.spp), s = (int)(t % P.p.spp);
    float *out = P.p.ball + t;
    const size_t stride = P.p.stride;
    const float R = P.p.radius[j];
    float m[DIM], wg = 0.0f, wu = 0.0f, ds[3] = {0.0f, 0.0f, 0.0f}, ms[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < DIM; ++k) m[k] = 0.0f;
    if (!ball_degenerate(R, P.p.eps)) {
        Pcg rng{0, 1};
        pcg_seed_pixel(rng, P.p.seed_base + P.p.first + j, P.p.seed_width);
        pcg_advance(rng, (int64_t)(DIM - 1) * P.p.spp + (int64_t)DIM * s);
        draw_direction<DIM>(rng, m);
        const float rho = pcg_next_float(rng);
        const float r = rho * R;
        float yp[DIM], ym[DIM], fp[3], fm[3];
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            const float x = P.p.pts[(size_t)DIM * (size_t)(P.p.first + j) + k], p = r * m[k];
            yp[k] = x + p;
            ym[k] = x - p;
        }
        ball_source(P.src, yp, fp);
        ball_source(P.src, ym, fm);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            ds[ch] = 0.5f * (fp[ch] - fm[ch]);
            ms[ch] = 0.5f * (fp[ch] + fm[ch]);
        }
        if (DIM == 2) {
            wg = 1.0f - rho * rho;
            wu = rho > 0.0f ? -(rho * det_logf(rho)) : 0.0f;
        } else {
            wg = 1.0f - (rho * rho) * rho;
            wu = rho - rho * rho;
        }
    }
#pragma unroll
    for (int k = 0; k < DIM; ++k) out[k * stride] = m[k];
    out[(DIM + kBallWg) * stride] = wg;
    out[(DIM + kBallWu) * stride] = wu;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        out[(DIM + kBallDs + ch) * stride] = ds[ch];
        out[(DIM + kBallMs + ch) * stride] = ms[ch];
    }
}

template <int DIM, class SRC>
static int grad_ball_launch(const SRC &src, const GradBall &p, hipStream_t stream)
{
    const GradBallParams<SRC> P{src, p};
    const int64_t threads = (int64_t)p.count * p.spp;
    hipLaunchKernelGGL((grad_ball_kernel<DIM, SRC>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, P);
    WOST_TRY(hipGetLastError());
    return WOST_OK;
}

int grad_ball2(const DevSource &src, const GradBall &p, hipStream_t stream) { return grad_ball_launch<2>(src, p, stream); }
int grad_ball3(const DevSource3 &src, const GradBall &p, hipStream_t stream) { return grad_ball_launch<3>(src, p, stream); }

int grad_ball_block(const GradCall &c, const float *pts, int32_t first, int32_t count, int32_t spp, int32_t seed_base, int32_t seed_width,
                    hipStream_t stream)
{
    const GradScratch &s = *c.scratch;
    return c.ball(GradBall{pts, first, count, spp, seed_base, seed_width, c.eps, s.radius, s.ball, s.ball_stride}, stream);
}

int grad_source_option(double value, bool *option)
{
    if (value != 0 && value != 1) return set_error(WOST_ERR_INVALID, "grad_source must be 0 or 1");
    *option = value == 1;
    return WOST_OK;
}

// ---- the kernel behind ---------------------------------------------------------------------------------------------------------
struct GradReduceParams {
    // the block: count points of spp walks each -- results (RGB), directions and first points per walk, radii per point
    const float *w, *dirs, *first_pts, *radius;
    // ... and with in-ball samples (nullptr: none) their arrays, ball_stride floats apart
    const float *ball;
    size_t ball_stride;
    int32_t first, count, spp;
    float eps;
    // the call's outputs, indexed by the point's index in the call; nullptr: not wanted (grad always is)
    float *grad, *grad_stderr, *field, *radius_out, *first_out;
};

// One wave per point, its lanes over the point's walks, three passes (the mean, the estimate, its two-pass variance:
// grad_point_sums_from, grad_point_variance_from; with in-ball samples grad_ball_sums, grad_ball_variance -- wost_grad.h):
//   mean_c = sum_s W_sc / S,   t_s = n_sk (W_sc - mean_c),   grad_kc = DIM / (R (S - 1)) sum_s t_s,
//   stderr_kc = DIM / R sqrt(sum_s (t_s - mean t)^2 / (S - 1) / S);   a degenerate point: NaN, NaN and its mean.
// The sums run in fp64 and the results are rounded once.  The control variate subtracts numbers of the size of u and leaves
// differences of the size of R |grad u|: a mean rounded to fp32 would sit in t_s with |u| / (R |grad u|) ulps, and the standard
// error of a point close to the boundary would lose that factor of its precision.
// With in-ball samples (include/wost.h "The gradient on a scene with a source term"): a_s = wg_s m_sk ds_sc,
//   T_kc = (R / S) sum_s a_s,   seT_kc = R sqrt(sum_s (a_s - mean a)^2 / (S - 1) / S),   U_c = (R^2 / S) sum_s wu_s ms_sc,
//   grad = walk part + T,   stderr = sqrt(walk part^2 + seT^2),   field = mean + U,   each still rounded once.
template <int DIM>
__global__ __launch_bounds__(256) void grad_reduce_kernel(GradReduceParams P)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (j >= P.count) return;      // (the whole wave)
    const int S = P.spp;
    const size_t i = (size_t)P.first + (size_t)j;
    const GradWalkArrays<DIM> load{P.w + 3 * (size_t)j * S, P.dirs + DIM * (size_t)j * S};
    const double dS = (double)S;
    double mean[3], t[DIM * 3], v[DIM * 3];
    grad_point_sums_from<DIM>(load, S, lane, mean, t);
    grad_point_variance_from<DIM>(load, S, lane, mean, t, v);
    const float R = P.radius[j];
    const bool degenerate = ball_degenerate(R, P.eps);
    double a[DIM * 3], u[3], va[DIM * 3];
    if (P.ball) {      // (the whole grid: P is uniform)
        grad_ball_sums<DIM>(P.ball + (size_t)j * S, P.ball_stride, S, lane, a, u);
        grad_ball_variance<DIM>(P.ball + (size_t)j * S, P.ball_stride, S, lane, a, va);
    }
    if (lane == 0) {
        const double scale = grad_scale<DIM>(R, S), scale_se = (double)DIM / (double)R;
#pragma unroll
        for (int e = 0; e < DIM * 3; ++e) {
            double g = scale * t[e], se = scale_se * sqrt(v[e] / (dS - 1.0) / dS);
            if (P.ball) {
                const double se_t = (double)R * sqrt(va[e] / (dS - 1.0) / dS);
                g += ball_grad_term(R, S, a[e]);
                se = sqrt(se * se + se_t * se_t);
            }
            P.grad[(size_t)(DIM * 3) * i + e] = degenerate ? WOST_NAN : (float)g;
            if (P.grad_stderr) P.grad_stderr[(size_t)(DIM * 3) * i + e] = degenerate ? WOST_NAN : (float)se;
        }
        if (P.field)
            for (int c = 0; c < 3; ++c) P.field[3 * i + c] = (float)(P.ball && !degenerate ? mean[c] + ball_field_term(R, S, u[c]) : mean[c]);
        if (P.radius_out) P.radius_out[i] = R;
    }
    if (P.first_out)
        for (int s = lane; s < DIM * S; s += 64) P.first_out[(size_t)DIM * S * i + s] = P.first_pts[(size_t)DIM * S * j + s];
}

// ---- the driver ----------------------------------------------------------------------------------------------------------------
void grad_free(GradScratch &s)
{
    if (s.mem) (void)hipFree(s.mem);
    if (s.ball) (void)hipFree(s.ball);
    for (hipEvent_t e : s.ev)
        if (e) (void)hipEventDestroy(e);
    s = GradScratch{};
}

int grad_ready(GradScratch &s, size_t n_pixels, int dim)
{
    if (s.mem) return WOST_OK;
    const size_t floats = n_pixels * (size_t)(2 * dim + 3) + n_pixels / 2 + 1;
    for (hipEvent_t &e : s.ev)
        if (!e) WOST_TRY(hipEventCreate(&e));
    WOST_TRY(hipMalloc(&s.mem, floats * sizeof(float)));
    s.first = static_cast<float *>(s.mem);
    s.dirs = s.first + n_pixels * dim;
    s.w = s.dirs + n_pixels * dim;
    s.radius = s.w + n_pixels * 3;
    return WOST_OK;
}

int grad_ball_ready(GradScratch &s, size_t n_pixels, int dim)
{
    if (s.ball) return WOST_OK;
    WOST_TRY(hipMalloc((void **)&s.ball, n_pixels * (size_t)(dim + kBallArrays) * sizeof(float)));
    s.ball_stride = n_pixels;
    return WOST_OK;
}

int grad_check(const void *h, const float *pts, int32_t n, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width,
               const wost_gradient_out *out)
{
    if (!h || !pts || !out || !out->grad) return set_error(WOST_ERR_INVALID, "null argument");
    if (n < 0) return set_error(WOST_ERR_INVALID, "negative number of points");
    if (seed_width <= 0) return set_error(WOST_ERR_INVALID, "seed_width must be positive");
    if (seed_base < 0 || walk_seed_base < 0) return set_error(WOST_ERR_INVALID, "seed_base and walk_seed_base must be >= 0");
    if ((int64_t)seed_base + n > ((int64_t)1 << 28)) return set_error(WOST_ERR_INVALID, "seed_base + n must be at most 2^28");
    return WOST_OK;
}

// the rules that need the handle: its spp setting S and its frame
int grad_check_handle(const GradCall &c, int32_t n, int32_t seed_base, int32_t walk_seed_base)
{
    const std::string name = std::string(c.prefix) + "solve_gradient_points: ";
    if (c.has_source && !c.source_term)
        return set_error(WOST_ERR_UNSUPPORTED, name + "a scene with a source term is not covered (the in-ball term of the gradient is not built)");
    const int64_t S = c.spp, walks = S * (int64_t)n;
    if (S < 2) return set_error(WOST_ERR_INVALID, name + "the handle's spp is " + std::to_string(S) + ", the estimator needs spp >= 2 walks per point");
    if ((uint64_t)S > (uint64_t)c.n_pixels)
        return set_error(WOST_ERR_INVALID, name + "the handle's spp (" + std::to_string(S) + ") exceeds n_pixels (" + std::to_string(c.n_pixels) +
                                               "): a point's walks must fit one point step");
    if ((int64_t)walk_seed_base + walks > ((int64_t)1 << 28))
        return set_error(WOST_ERR_INVALID, name + "walk_seed_base + n * spp (" + std::to_string((int64_t)walk_seed_base + walks) + ") must be at most 2^28");
    if ((int64_t)seed_base < (int64_t)walk_seed_base + walks && (int64_t)walk_seed_base < (int64_t)seed_base + n)
        return set_error(WOST_ERR_INVALID, name + "the seeds of the directions [seed_base, seed_base + n) overlap those of the walks [walk_seed_base, "
                                                  "walk_seed_base + n * spp)");
    return WOST_OK;
}

int grad_solve_dev(const GradCall &c, const float *pts_dev, int32_t n, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width,
                   const wost_gradient_out &out, hipStream_t stream, wost_stats *stats)
{
    const auto t0 = HostClock::now();
    WOST_TRY(hipSetDevice(c.device));
    GradScratch &s = *c.scratch;
    int rc = grad_ready(s, c.n_pixels, c.dim);
    if (rc == WOST_OK && c.in_ball()) rc = grad_ball_ready(s, c.n_pixels, c.dim);
    if (rc != WOST_OK) return rc;
    const int32_t S = c.spp, per_block = (int32_t)(c.n_pixels / (size_t)S);
    wost_stats total{};
    for (int32_t a = 0; a < n; a += per_block) {
        const int32_t m = std::min(per_block, n - a), walks = m * S;
        WOST_TRY(hipEventRecord(s.ev[0], stream));
        if ((rc = c.prep(GradPrep{pts_dev, a, m, S, seed_base, seed_width, c.eps, s.radius, s.dirs, s.first}, stream)) != WOST_OK) return rc;
        if (c.in_ball() && (rc = grad_ball_block(c, pts_dev, a, m, S, seed_base, seed_width, stream)) != WOST_OK) return rc;
        WOST_TRY(hipEventRecord(s.ev[1], stream));
        WOST_TRY(hipMemsetAsync(s.w, 0, (size_t)walks * 3 * sizeof(float), stream));
        wost_stats st{};
        if ((rc = c.walk(s.first, walks, walk_seed_base + a * S, seed_width, s.w, stream, &st)) != WOST_OK) return rc;
        const GradReduceParams rp{s.w, s.dirs, s.first, s.radius, c.in_ball() ? s.ball : nullptr, s.ball_stride, a, m, S, c.eps,
                                  out.grad, out.grad_stderr, out.field_rgb, out.radius, out.first_pts};
        WOST_TRY(hipEventRecord(s.ev[2], stream));
        if (c.dim == 2) hipLaunchKernelGGL(grad_reduce_kernel<2>, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, stream, rp);
        else hipLaunchKernelGGL(grad_reduce_kernel<3>, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, stream, rp);
        WOST_TRY(hipGetLastError());
        WOST_TRY(hipEventRecord(s.ev[3], stream));
        WOST_TRY(hipEventSynchronize(s.ev[3]));
        float ms_front = 0.0f, ms_behind = 0.0f;
        WOST_TRY(hipEventElapsedTime(&ms_front, s.ev[0], s.ev[1]));
        WOST_TRY(hipEventElapsedTime(&ms_behind, s.ev[2], s.ev[3]));
        add_stats(total, st);
        total.kernel_ms += (double)ms_front + (double)ms_behind;
    }
    if (stats) {
        *stats = total;
        stamp_solve_ms(stats, t0);
    }
    return WOST_OK;
}

int grad_solve_host(const GradCall &c, const float *pts, int32_t n, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width,
                    const wost_gradient_out &out, wost_stats *stats)
{
    const auto t0 = HostClock::now();
    WOST_TRY(hipSetDevice(c.device));
    const size_t N = (size_t)n, dim = (size_t)c.dim, S = (size_t)c.spp;
    Batch b{c.stream};
    float *d_pts = nullptr;
    wost_gradient_out d{};
    WOST_TRY(b.in(pts, N * dim, &d_pts));
    WOST_TRY(b.out(&d.grad, N * dim * 3));
    if (out.grad_stderr) WOST_TRY(b.out(&d.grad_stderr, N * dim * 3));
    if (out.field_rgb) WOST_TRY(b.out(&d.field_rgb, N * 3));
    if (out.radius) WOST_TRY(b.out(&d.radius, N));
    if (out.first_pts) WOST_TRY(b.out(&d.first_pts, N * S * dim));
    int rc = grad_solve_dev(c, d_pts, n, seed_base, walk_seed_base, seed_width, d, c.stream, stats);
    if (rc != WOST_OK) {
        (void)hipStreamSynchronize(c.stream);      // (the scratch arrays are freed on return)
        return rc;
    }
    WOST_TRY(b.fetch(out.grad, d.grad, N * dim * 3));
    WOST_TRY(b.fetch(out.grad_stderr, d.grad_stderr, N * dim * 3));
    WOST_TRY(b.fetch(out.field_rgb, d.field_rgb, N * 3));
    WOST_TRY(b.fetch(out.radius, d.radius, N));
    WOST_TRY(b.fetch(out.first_pts, d.first_pts, N * S * dim));
    if ((rc = b.finish()) == WOST_OK) stamp_solve_ms(stats, t0);
    return rc;
}

}  // namespace wost
