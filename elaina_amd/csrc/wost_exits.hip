// wost_exits.hip -- the exit list of a handle (wost_exits.h; include/wost.h "Exit lists"): the two kernels behind
// the walks -- apply, one wave per point over its records for K sets of Dirichlet colours, and the adjoint, a scatter of fp64
// atomic adds over the same records -- and the driver: the list in chunks of n_pixels walks, the records into host arrays, the
// host and device forms of apply and adjoint.  Cold path beside the walk kernels, which do not know of it.  And the list of the
// gradient (include/wost.h "Exit lists of the gradient"): the same list walked from the first points of the
// gradient's estimator, kept with their directions and radii, and the two kernels that are its hot path -- grad u, its standard
// error and the mean for K sets of colours, one wave per point, and the transpose of that map.  On a scene with a source term
// (the option "exits_grad_source") the walk also reduces the in-ball samples of the gradient's estimator to three fp64 terms per
// point, which the list keeps and apply joins to every set (exits_ball_terms_kernel; DESIGN 4.3i "The in-ball term").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "wost_exits.h"
#include "wost_grad.h"

namespace wost {

#define WOST_NAN __int_as_float(0x7fc00000)

// ---- one record against one set of colours ----------------------------------------------------------------------------------
// A record as a lane holds it: slot < 0 is a walk that was not absorbed (W = base).
template <int DIM>
struct ExitRec {
    int32_t slot, side;
    float uv[DIM - 1], thp, base[3];
    int32_t v[DIM];
};

template <int DIM>
__device__ __forceinline__ ExitRec<DIM> exit_load(const ExitRecords &r, const int32_t *verts, size_t w)
{
    ExitRec<DIM> e;
    e.slot = r.slot()[w];
    e.side = r.side()[w];
#pragma unroll
    for (int k = 0; k < DIM - 1; ++k) e.uv[k] = r.uv(k)[w];
    e.thp = r.thp()[w];
#pragma unroll
    for (int c = 0; c < 3; ++c) e.base[c] = r.base(DIM, c)[w];
#pragma unroll
    for (int k = 0; k < DIM; ++k) e.v[k] = e.slot >= 0 ? verts[(size_t)DIM * e.slot + k] : 0;
    return e;
}

// the weights of the primitive's vertices, with the operations of surface_color (1 - uv, uv) and surface_color3 (1 - u - v, u, v)
template <int DIM>
__device__ __forceinline__ void exit_weights(const ExitRec<DIM> &e, float (&wgt)[DIM])
{
    if (DIM == 2) {
        wgt[0] = 1 - e.uv[0];
        wgt[1] = e.uv[0];
    } else {
        wgt[0] = 1 - e.uv[0] - e.uv[DIM - 2];
        wgt[1] = e.uv[0];
        wgt[DIM - 1] = e.uv[DIM - 2];
    }
}

// W of the walk for one set of colours (n_verts * 6), channel by channel: the colour of surface_color / surface_color3, times
// the intensity, times the throughput, plus base -- every line one fp32 operation, as the walk step has them
template <int DIM>
__device__ __forceinline__ void exit_value(const ExitRec<DIM> &e, const float *colors, float intensity, float (&W)[3])
{
    if (e.slot < 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) W[c] = e.base[c];
        return;
    }
    float wgt[DIM];
    exit_weights<DIM>(e, wgt);
    const int off = (e.side >= 0) ? 0 : 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = colors[6 * (size_t)e.v[0] + off + c], b = colors[6 * (size_t)e.v[1] + off + c];
        float col;
        if (DIM == 2) {
            col = a * wgt[0] + b * wgt[1];
        } else {
            const float cc = colors[6 * (size_t)e.v[DIM - 1] + off + c];
            col = (a * wgt[0] + b * wgt[1]) + cc * wgt[DIM - 1];
        }
        col *= intensity;
        col *= e.thp;
        W[c] = col + e.base[c];
    }
}

// ---- apply ------------------------------------------------------------------------------------------------------------------
struct ExitApplyParams {
    ExitRecords rec;
    const int32_t *verts;
    const float *colors;     // K sets of n_verts * 6
    int32_t n, S, K, n_verts;
    float intensity;
    float *field, *se;       // K * n * 3 each; se may be nullptr
};

// One wave per point, its lanes over the point's S walks, per set two passes in fp64 over the fp32 W (the mean, the two-pass
// variance), rounded once.  A lane keeps the record of its first walk in registers for all K sets -- with S <= 64 every record
// is read once --; the walks beyond the first 64 of a point are read again per set (from the cache: a point's records are
// S * 36 bytes).
template <int DIM>
__global__ __launch_bounds__(256) void exits_apply_kernel(ExitApplyParams P)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= P.n) return;      // (the whole wave)
    const int S = P.S;
    const size_t w0 = (size_t)i * S;
    ExitRec<DIM> first{};
    first.slot = -1;
    if (lane < S) first = exit_load<DIM>(P.rec, P.verts, w0 + lane);
    const double dS = (double)S;
    for (int k = 0; k < P.K; ++k) {
        const float *colors = P.colors + (size_t)k * P.n_verts * 6;
        double mean[3] = {0.0, 0.0, 0.0}, var[3] = {0.0, 0.0, 0.0};
        for (int s = lane; s < S; s += 64) {
            float W[3];
            exit_value<DIM>(s == lane ? first : exit_load<DIM>(P.rec, P.verts, w0 + s), colors, P.intensity, W);
            for (int c = 0; c < 3; ++c) mean[c] += (double)W[c];
        }
        for (int c = 0; c < 3; ++c) mean[c] = wave_sum(mean[c]) / dS;
        if (P.se) {
            for (int s = lane; s < S; s += 64) {
                float W[3];
                exit_value<DIM>(s == lane ? first : exit_load<DIM>(P.rec, P.verts, w0 + s), colors, P.intensity, W);
                for (int c = 0; c < 3; ++c) {
                    const double dev = (double)W[c] - mean[c];
                    var[c] += dev * dev;
                }
            }
            for (int c = 0; c < 3; ++c) var[c] = wave_sum(var[c]);
        }
        if (lane == 0) {
            const size_t o = ((size_t)k * P.n + i) * 3;
            for (int c = 0; c < 3; ++c) {
                P.field[o + c] = (float)mean[c];
                if (P.se) P.se[o + c] = S > 1 ? (float)sqrt(var[c] / (dS - 1.0) / dS) : __builtin_inff();
            }
        }
    }
}

// ---- adjoint ----------------------------------------------------------------------------------------------------------------
struct ExitAdjointParams {
    ExitRecords rec;
    const int32_t *verts;
    const float *dfield;     // K * n * 3
    int32_t n, S, K, n_verts;
    float intensity;
    double *acc;             // K * n_verts * 6, zeroed
};

// One lane per walk.  An absorbed walk (i, s) adds, per set, channel and vertex of its primitive, the term
// (dfield[k][i][c] / S) * intensity * thp * w_v -- fp64 from the fp32 operands, multiplied in this order -- to the entry of that
// vertex and side, by an fp64 atomic add: the order of the sum is the arrival order.
template <int DIM>
__global__ __launch_bounds__(256) void exits_adjoint_kernel(ExitAdjointParams P)
{
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= (size_t)P.n * P.S) return;
    const ExitRec<DIM> e = exit_load<DIM>(P.rec, P.verts, w);
    if (e.slot < 0) return;
    float wgt[DIM];
    exit_weights<DIM>(e, wgt);
    const int off = (e.side >= 0) ? 0 : 3;
    const size_t i = w / (size_t)P.S;
    for (int k = 0; k < P.K; ++k) {
        double *acc = P.acc + (size_t)k * P.n_verts * 6;
        for (int c = 0; c < 3; ++c) {
            const double g = (double)P.dfield[((size_t)k * P.n + i) * 3 + c] / (double)P.S * (double)P.intensity * (double)e.thp;
#pragma unroll
            for (int v = 0; v < DIM; ++v) atomicAdd(acc + 6 * (size_t)e.v[v] + off + c, g * (double)wgt[v]);
        }
    }
}

__global__ __launch_bounds__(256) void exits_round_kernel(const double *acc, float *out, size_t count)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < count) out[j] = (float)acc[j];
}

// ---- the list of the gradient: the in-ball term at walk time -----------------------------------------------------------------
struct ExitBallTermsParams {
    const float *ball;               // a block's in-ball samples as grad_ball_kernel leaves them, `stride` floats apart
    size_t stride;
    const float *radius;             // the block's radii
    double *terms;                   // the block's part of the list's terms
    int32_t count, S;
    float eps;
};

// One wave per point of a block behind grad_ball_kernel: the two passes of grad_reduce_kernel over the point's S in-ball samples
// (grad_ball_sums, grad_ball_variance, with its arguments) and, by lane 0, the three terms that kernel joins to the walk part,
// kept in fp64 as it forms them:  T_e = (R / S) a_e,  seT_e = R sqrt(va_e / (S - 1) / S),  U_c = (R^2 / S) u_c  -- T (DIM * 3),
// seT (DIM * 3), U (3) per point.  A degenerate point took no samples and has +0.0 in all of them.
template <int DIM>
__global__ __launch_bounds__(256) void exits_ball_terms_kernel(ExitBallTermsParams P)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (j >= P.count) return;      // (the whole wave)
    const int S = P.S;
    const double dS = (double)S;
    double a[DIM * 3], u[3], va[DIM * 3];
    grad_ball_sums<DIM>(P.ball + (size_t)j * S, P.stride, S, lane, a, u);
    grad_ball_variance<DIM>(P.ball + (size_t)j * S, P.stride, S, lane, a, va);
    if (lane == 0) {
        const float R = P.radius[j];
        const bool degenerate = ball_degenerate(R, P.eps);
        double *out = P.terms + (size_t)(6 * DIM + 3) * j;
#pragma unroll
        for (int e = 0; e < DIM * 3; ++e) {
            out[e] = degenerate ? 0.0 : ball_grad_term(R, S, a[e]);
            out[DIM * 3 + e] = degenerate ? 0.0 : (double)R * sqrt(va[e] / (dS - 1.0) / dS);
        }
        for (int c = 0; c < 3; ++c) out[6 * DIM + c] = degenerate ? 0.0 : ball_field_term(R, S, u[c]);
    }
}

// ---- the list of the gradient: apply -----------------------------------------------------------------------------------------
struct ExitApplyGradParams {
    ExitRecords rec;
    const int32_t *verts;
    const float *colors;             // K sets of n_verts * 6
    const float *radius, *dirs;      // the list's: n, and DIM per walk
    int32_t n, S, K, n_verts;
    float intensity, eps;
    float *grad, *se, *field;        // K * n * DIM * 3, the same, K * n * 3; se and field may be nullptr
    const double *terms;             // the list's in-ball term, 6 * DIM + 3 per point (BALL; nullptr without)
};

// One wave per point, its lanes over the point's S walks, per set the three passes of grad_reduce_kernel (the mean, the
// estimate, its two-pass variance) in fp64 over W as exit_value forms it: the same functions (grad_point_sums_from,
// grad_point_variance_from) with another loader, so with the handle's own colours the bits of wost_solve_gradient_points.  A lane keeps the record, the weights' operands and the direction of its first
// walk in registers for all K sets and that walk's W for the three passes of a set: with S <= 64 every record and direction is
// read once, and W is formed once per set.  The walks beyond the first 64 of a point are read again per pass (from the cache).
// W never passes through memory.  Lane 0 writes the DIM * 3 + DIM * 3 + 3 results of a set.
// BALL (a list that carries the in-ball term): lane 0 joins the point's T, seT and U to every set as grad_reduce_kernel joins
// them -- grad = walk part + T, stderr = sqrt(walk part^2 + seT^2), field = mean + U unless the point is degenerate, each still
// rounded once --, and loads them where it uses them: nothing of them is live across the three passes.
template <int DIM, bool BALL>
__global__ __launch_bounds__(256) void exits_apply_gradient_kernel(ExitApplyGradParams P)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= P.n) return;      // (the whole wave)
    const int S = P.S;
    const size_t w0 = (size_t)i * S;
    ExitRec<DIM> first{};
    first.slot = -1;
    float n0[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) n0[a] = 0.0f;
    if (lane < S) {
        first = exit_load<DIM>(P.rec, P.verts, w0 + lane);
#pragma unroll
        for (int a = 0; a < DIM; ++a) n0[a] = P.dirs[DIM * (w0 + lane) + a];
    }
    const float R = P.radius[i];
    const bool degenerate = ball_degenerate(R, P.eps);
    const double dS = (double)S;
    for (int k = 0; k < P.K; ++k) {
        const float *colors = P.colors + (size_t)k * P.n_verts * 6;
        float W0[3];
        exit_value<DIM>(first, colors, P.intensity, W0);
        const auto load = [&](int s, float (&W)[3], float (&n)[DIM]) {
            if (s == lane) {
                for (int c = 0; c < 3; ++c) W[c] = W0[c];
#pragma unroll
                for (int a = 0; a < DIM; ++a) n[a] = n0[a];
            } else {
                exit_value<DIM>(exit_load<DIM>(P.rec, P.verts, w0 + s), colors, P.intensity, W);
#pragma unroll
                for (int a = 0; a < DIM; ++a) n[a] = P.dirs[DIM * (w0 + s) + a];
            }
        };
        double mean[3], t[DIM * 3], v[DIM * 3];
        grad_point_sums_from<DIM>(load, S, lane, mean, t);
        if (P.se) grad_point_variance_from<DIM>(load, S, lane, mean, t, v);      // (the whole grid: P is uniform)
        if (lane == 0) {
            const size_t o = (size_t)k * P.n + i;
            const double scale = grad_scale<DIM>(R, S), scale_se = (double)DIM / (double)R;
            if (BALL) {
                const double *terms = P.terms + (size_t)(6 * DIM + 3) * i;
#pragma unroll
                for (int e = 0; e < DIM * 3; ++e) {
                    double g = scale * t[e];
                    g += terms[e];
                    P.grad[(size_t)(DIM * 3) * o + e] = degenerate ? WOST_NAN : (float)g;
                    if (P.se) {
                        double se = scale_se * sqrt(v[e] / (dS - 1.0) / dS);
                        const double se_t = terms[DIM * 3 + e];
                        se = sqrt(se * se + se_t * se_t);
                        P.se[(size_t)(DIM * 3) * o + e] = degenerate ? WOST_NAN : (float)se;
                    }
                }
                if (P.field)
                    for (int c = 0; c < 3; ++c) P.field[3 * o + c] = (float)(degenerate ? mean[c] : mean[c] + terms[6 * DIM + c]);
            } else {
#pragma unroll
                for (int e = 0; e < DIM * 3; ++e) {
                    P.grad[(size_t)(DIM * 3) * o + e] = degenerate ? WOST_NAN : (float)(scale * t[e]);
                    if (P.se) P.se[(size_t)(DIM * 3) * o + e] = degenerate ? WOST_NAN : (float)(scale_se * sqrt(v[e] / (dS - 1.0) / dS));
                }
                if (P.field)
                    for (int c = 0; c < 3; ++c) P.field[3 * o + c] = (float)mean[c];
            }
        }
    }
}

// ---- the list of the gradient: adjoint ---------------------------------------------------------------------------------------
struct ExitAdjointGradParams {
    ExitRecords rec;
    const int32_t *verts;
    const float *dgrad;              // K * n * DIM * 3
    const float *radius, *dirs;
    int32_t n, S, K, n_verts;
    float intensity, eps;
    double *acc;                     // K * n_verts * 6, zeroed
};

// One wave per point: its walks share R, nbar and the rows of dgrad.  nbar_a = sum_s n_sa / S by one wave_sum per axis; then
// the lanes run over the walks, and an absorbed walk adds, per set, channel and vertex of its primitive, the term
//   q * intensity * thp * w_v,   q = sum_a dgrad[k][i][a][c] * (DIM / (R (S - 1))) * (n_sa - nbar_a)
// -- fp64 from the fp32 operands, multiplied in this order -- to the entry of that vertex and side, by an fp64 atomic add.  A
// degenerate point (a point that is not finite has a NaN radius) adds nothing and its dgrad is not read.
template <int DIM>
__global__ __launch_bounds__(256) void exits_adjoint_gradient_kernel(ExitAdjointGradParams P)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= P.n) return;      // (the whole wave)
    const float R = P.radius[i];
    if (ball_degenerate(R, P.eps)) return;      // (the whole wave)
    const int S = P.S;
    const size_t w0 = (size_t)i * S;
    double nbar[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) nbar[a] = 0.0;
    for (int s = lane; s < S; s += 64) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) nbar[a] += (double)P.dirs[DIM * (w0 + s) + a];
    }
#pragma unroll
    for (int a = 0; a < DIM; ++a) nbar[a] = wave_sum(nbar[a]) / (double)S;
    const double scale = grad_scale<DIM>(R, S);
    for (int s = lane; s < S; s += 64) {
        const ExitRec<DIM> e = exit_load<DIM>(P.rec, P.verts, w0 + s);
        if (e.slot < 0) continue;
        float wgt[DIM];
        exit_weights<DIM>(e, wgt);
        const int off = (e.side >= 0) ? 0 : 3;
        double cen[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) cen[a] = (double)P.dirs[DIM * (w0 + s) + a] - nbar[a];
        for (int k = 0; k < P.K; ++k) {
            double *acc = P.acc + (size_t)k * P.n_verts * 6;
            const float *dg = P.dgrad + ((size_t)k * P.n + i) * (DIM * 3);
            for (int c = 0; c < 3; ++c) {
                double q = (double)dg[c] * scale * cen[0];
#pragma unroll
                for (int a = 1; a < DIM; ++a) q += (double)dg[3 * a + c] * scale * cen[a];
                const double g = q * (double)P.intensity * (double)e.thp;
#pragma unroll
                for (int v = 0; v < DIM; ++v) atomicAdd(acc + 6 * (size_t)e.v[v] + off + c, g * (double)wgt[v]);
            }
        }
    }
}

// ---- the ordered adjoints: gathers over the index of the list -------------------------------------------------
struct ExitOrderedParams {
    ExitRecords rec;
    const int32_t *verts;
    const float *in;                 // dfield (K * n * 3) or dgrad (K * n * DIM * 3)
    const float *radius, *dirs;      // the list's (the gradient form)
    const double *nbar;              // the index's: n * DIM (the gradient form)
    const int64_t *bin_begin;        // 2 * n_verts + 1
    const int32_t *inc;
    int32_t n, S, K, n_verts;
    float intensity, eps;
    float *out;                      // K * n_verts * 6
};

// One wave per (bin, set): the wave of bin b = 2 v + (side < 0) and set k owns the three entries dcolors[k][v][off + c].  Its
// lanes take the bin's incidences at positions lane, lane + 64, ... in that order; for incidence w * DIM + j a lane forms the
// term of walk w and corner j, factor by factor as the scatter kernels do, and adds it to its three fp64 sums, which start at
// +0.0.  Then one wave_sum per channel, one rounding to fp32 and a plain store by lane 0: no scratch array, no atomic, and an
// order that is a function of the list alone.  GRAD: the terms of exits_adjoint_gradient_kernel with nbar from the index; an
// incidence of a degenerate point is skipped and its dgrad is not read.  An empty bin stores +0.0f.
template <int DIM, bool GRAD>
__device__ __forceinline__ void exits_ordered_wave(const ExitOrderedParams &P)
{
    const int lane = threadIdx.x & 63;
    const size_t bins = 2 * (size_t)P.n_verts;
    const size_t g = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= bins * (size_t)P.K) return;      // (the whole wave)
    const size_t k = g / bins, b = g % bins;
    const int64_t begin = P.bin_begin[b], end = P.bin_begin[b + 1];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t p = begin + lane; p < end; p += 64) {
        const int32_t inc = P.inc[p];
        const size_t w = (size_t)(inc / DIM);
        const int j = inc % DIM;
        const size_t i = w / (size_t)P.S;
        const ExitRec<DIM> e = exit_load<DIM>(P.rec, P.verts, w);
        float wgt[DIM];
        exit_weights<DIM>(e, wgt);
        const float w_v = j == 0 ? wgt[0] : (j == 1 ? wgt[1] : wgt[DIM - 1]);
        if (GRAD) {
            const float R = P.radius[i];
            if (ball_degenerate(R, P.eps)) continue;
            const double scale = grad_scale<DIM>(R, P.S);
            double cen[DIM];
#pragma unroll
            for (int a = 0; a < DIM; ++a) cen[a] = (double)P.dirs[DIM * w + a] - P.nbar[DIM * i + a];
            const float *dg = P.in + (k * (size_t)P.n + i) * (DIM * 3);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double q = (double)dg[c] * scale * cen[0];
#pragma unroll
                for (int a = 1; a < DIM; ++a) q += (double)dg[3 * a + c] * scale * cen[a];
                acc[c] += q * (double)P.intensity * (double)e.thp * (double)w_v;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                acc[c] += (double)P.in[(k * (size_t)P.n + i) * 3 + c] / (double)P.S * (double)P.intensity * (double)e.thp * (double)w_v;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = wave_sum(acc[c]);
    if (lane == 0) {
        float *out = P.out + (k * (size_t)P.n_verts + (b >> 1)) * 6 + ((b & 1) ? 3 : 0);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = (float)acc[c];
    }
}

template <int DIM>
__global__ __launch_bounds__(256) void exits_adjoint_ordered_kernel(ExitOrderedParams P)
{
    exits_ordered_wave<DIM, false>(P);
}

template <int DIM>
__global__ __launch_bounds__(256) void exits_adjoint_gradient_ordered_kernel(ExitOrderedParams P)
{
    exits_ordered_wave<DIM, true>(P);
}

// ---- the driver -------------------------------------------------------------------------------------------------------------
void exits_index_free(ExitIndex &x)
{
    if (x.mem) (void)hipFree(x.mem);
    x = ExitIndex{};
}

void exits_free(ExitList &l)
{
    exits_index_free(l.index);
    if (l.mem) (void)hipFree(l.mem);
    l = ExitList{};
}

int exits_alloc(void **p, size_t bytes, const char *what)
{
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return set_error(WOST_ERR_NOMEM, std::string("out of device memory for ") + what + " (" + std::to_string(bytes) + " bytes)");
    }
    WOST_TRY_AS("hipMalloc", e);
    return WOST_OK;
}

// a device array of `count` floats that the batch of a host call owns (never empty: a scene without a Dirichlet mesh has no colours)
static int exits_stage(Batch &b, float **dev, size_t count, const char *what)
{
    void *p = nullptr;
    const int rc = exits_alloc(&p, count * sizeof(float) + 16, what);
    if (rc != WOST_OK) return rc;
    b.scratch.ptrs.push_back(p);
    *dev = static_cast<float *>(p);
    return WOST_OK;
}

// the arrays of a list of N walks, carved from one allocation: prim, slot, side, thp, DIM - 1 of uv and three of base, four
// bytes an entry -- and behind them, for a list of the gradient, the radii (n), the directions and the first points (dim * N each)
// -- and behind those, for one that carries the in-ball term, 6 dim + 3 doubles per point from the next multiple of 8 bytes on
static int exits_carve(ExitList &l, int dim, int32_t n, int32_t S, bool gradient, bool in_ball)
{
    const size_t N = (size_t)n * S, records = N * (size_t)(6 + dim);
    const size_t words = records + (gradient ? (size_t)n + 2 * (size_t)dim * N : 0), terms_at = (words + 1) / 2 * 2;
    const size_t bytes = in_ball ? terms_at * 4 + (size_t)n * (size_t)(6 * dim + 3) * sizeof(double) : words * 4;
    const int rc = exits_alloc(&l.mem, bytes, "the exit list");
    if (rc != WOST_OK) return rc;
    l.rec = ExitRecords{static_cast<int32_t *>(l.mem), N};
    l.dim = dim; l.n = n; l.S = S;
    if (gradient) {
        l.radius = static_cast<float *>(l.mem) + records;
        l.dirs = l.radius + n;
        l.first = l.dirs + (size_t)dim * N;
    }
    if (in_ball) l.terms = reinterpret_cast<double *>(static_cast<float *>(l.mem) + terms_at);
    return WOST_OK;
}

int exits_check_walk(const void *h, const float *pts, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width)
{
    if (!h) return set_error(WOST_ERR_INVALID, "null argument");
    if (n < 0) return set_error(WOST_ERR_INVALID, "negative number of points");
    if (n > 0 && !pts) return set_error(WOST_ERR_INVALID, "null argument");
    if (walks < 1) return set_error(WOST_ERR_INVALID, "walks must be at least 1");
    if (seed_width <= 0) return set_error(WOST_ERR_INVALID, "seed_width must be positive");
    if (walk_seed_base < 0) return set_error(WOST_ERR_INVALID, "walk_seed_base must be >= 0");
    const int64_t end = (int64_t)walk_seed_base + (int64_t)n * walks;
    if (end > ((int64_t)1 << 28))
        return set_error(WOST_ERR_INVALID, "walk_seed_base + n * walks (" + std::to_string(end) + ") must be at most 2^28");
    return WOST_OK;
}

int exits_check_walk_gradient(const void *h, const float *pts, int32_t n, int32_t walks, const ExitSeeds &seeds)
{
    if (!h) return set_error(WOST_ERR_INVALID, "null argument");
    if (n < 0) return set_error(WOST_ERR_INVALID, "negative number of points");
    if (n > 0 && !pts) return set_error(WOST_ERR_INVALID, "null argument");
    if (walks < 2) return set_error(WOST_ERR_INVALID, "walks must be at least 2: the estimator needs two walks per point");
    if (seeds.seed_width <= 0) return set_error(WOST_ERR_INVALID, "seed_width must be positive");
    if (seeds.seed_base < 0 || seeds.walk_seed_base < 0) return set_error(WOST_ERR_INVALID, "seed_base and walk_seed_base must be >= 0");
    if ((int64_t)seeds.seed_base + n > ((int64_t)1 << 28)) return set_error(WOST_ERR_INVALID, "seed_base + n must be at most 2^28");
    const int64_t end = (int64_t)seeds.walk_seed_base + (int64_t)n * walks;
    if (end > ((int64_t)1 << 28))
        return set_error(WOST_ERR_INVALID, "walk_seed_base + n * walks (" + std::to_string(end) + ") must be at most 2^28");
    if ((int64_t)seeds.seed_base < end && (int64_t)seeds.walk_seed_base < (int64_t)seeds.seed_base + n)
        return set_error(WOST_ERR_INVALID, "the seeds of the directions [seed_base, seed_base + n) overlap those of the walks [walk_seed_base, "
                                           "walk_seed_base + n * walks)");
    return WOST_OK;
}

int exits_check_apply(const void *h, const void *in, int32_t K, const void *out, const char *in_name, const char *out_name)
{
    if (!h) return set_error(WOST_ERR_INVALID, "null argument");
    if (!in) return set_error(WOST_ERR_INVALID, std::string("null argument: ") + in_name);
    if (!out) return set_error(WOST_ERR_INVALID, std::string("null argument: ") + out_name);
    if (K < 1) return set_error(WOST_ERR_INVALID, "K must be at least 1");
    return WOST_OK;
}

namespace {
// two events of a call, destroyed on every return path
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};
// the new list of a walk until it stands whole: freed on every other return path
struct ListGuard {
    ExitList l;
    ~ListGuard() { exits_free(l); }
};
}  // namespace

// The walk of a plain list (gradient == false: seeds.seed_base is not read) and of a list of the gradient.  The latter runs the
// kernel in front first, in launches of at most n_pixels points, straight into the new list's radii, directions and first
// points (GradPrep's pointers are the launch's own: offset per launch); then its walks are those of a plain list of the n * S
// first points with one walk each -- walk w reads point w, seeds pixel walk_seed_base + w and writes record w.
// in_ball (a list of the gradient on a scene with a source term, the handle's "exits_grad_source" on): between the kernel in
// front and the walks, the in-ball passes, in blocks of max(1, floor(n_pixels / S)) points as the single call cuts them -- the
// in-ball kernel of the single call (S samples per point from the directions' streams, reading the list's radii) into a
// temporary of this call's own, dim + 8 arrays of max(n_pixels, S) floats, and exits_ball_terms_kernel behind it, which leaves
// the block's terms in the list.  Two launches per block; the samples are no walks and count in none of the five counters.
static int exits_walk_list(const ExitCall &c, const float *pts, bool pts_on_host, int32_t n, int32_t walks, const ExitSeeds &seeds, bool gradient,
                           hipStream_t stream, wost_stats *stats)
{
    const int32_t walk_seed_base = seeds.walk_seed_base, seed_width = seeds.seed_width;
    const auto t0 = HostClock::now();
    WOST_TRY(hipSetDevice(c.device));
    const bool in_ball = gradient && c.in_ball();
    ListGuard fresh;
    int rc = exits_carve(fresh.l, c.dim, n, walks, gradient, in_ball);
    if (rc != WOST_OK) return rc;
    Scratch scratch;
    void *d_pts = nullptr, *d_counters = nullptr, *d_ball = nullptr;
    if ((rc = exits_alloc(&d_counters, 5 * sizeof(unsigned long long), "the counters of the walk")) != WOST_OK) return rc;
    scratch.ptrs.push_back(d_counters);
    const size_t ball_stride = std::max(c.n_pixels, (size_t)walks);
    if (in_ball) {
        if ((rc = exits_alloc(&d_ball, ball_stride * (size_t)(c.dim + kBallArrays) * sizeof(float), "the in-ball samples of the walk")) != WOST_OK) return rc;
        scratch.ptrs.push_back(d_ball);
    }
    if (pts_on_host) {
        const size_t bytes = (size_t)n * c.dim * sizeof(float);
        if ((rc = exits_alloc(&d_pts, bytes, "the points")) != WOST_OK) return rc;
        scratch.ptrs.push_back(d_pts);
        WOST_TRY(hipMemcpyAsync(d_pts, pts, bytes, hipMemcpyHostToDevice, stream));
    }
    EventPair ev;
    WOST_TRY(hipEventCreate(&ev.a));
    WOST_TRY(hipEventCreate(&ev.b));
    WOST_TRY(hipMemsetAsync(d_counters, 0, 5 * sizeof(unsigned long long), stream));
    WOST_TRY(hipEventRecord(ev.a, stream));
    const int64_t N = (int64_t)n * walks, cap = (int64_t)std::min<size_t>(c.n_pixels, (size_t)1 << 28);
    uint32_t launches = 0;
    const float *walk_pts = pts_on_host ? static_cast<const float *>(d_pts) : pts;
    int32_t per_point = walks;
    if (gradient) {
        const ExitList &l = fresh.l;
        for (int64_t a = 0; a < n; a += cap, ++launches) {
            const size_t at = (size_t)c.dim * (size_t)a * (size_t)walks;
            const GradPrep p{walk_pts, (int32_t)a, (int32_t)std::min<int64_t>(cap, n - a), walks, seeds.seed_base, seed_width, c.eps,
                             l.radius + a, l.dirs + at, l.first + at};
            if ((rc = c.prep(p, stream)) != WOST_OK) {
                (void)hipStreamSynchronize(stream);      // (the scratch arrays are freed on return)
                return rc;
            }
        }
        if (in_ball) {
            const int64_t per_block = std::max<int64_t>(1, (int64_t)(c.n_pixels / (size_t)walks));
            const size_t per_point_terms = (size_t)(6 * c.dim + 3);
            for (int64_t a = 0; a < n; a += per_block, launches += 2) {
                const int32_t m = (int32_t)std::min<int64_t>(per_block, n - a);
                rc = c.ball(GradBall{walk_pts, (int32_t)a, m, walks, seeds.seed_base, seed_width, c.eps, l.radius + a, static_cast<float *>(d_ball), ball_stride},
                            stream);
                if (rc == WOST_OK) {
                    const ExitBallTermsParams P{static_cast<const float *>(d_ball), ball_stride, l.radius + a, l.terms + per_point_terms * (size_t)a, m, walks, c.eps};
                    const dim3 grid((unsigned)((m + 3) / 4));
                    if (c.dim == 2) hipLaunchKernelGGL(exits_ball_terms_kernel<2>, grid, dim3(256), 0, stream, P);
                    else hipLaunchKernelGGL(exits_ball_terms_kernel<3>, grid, dim3(256), 0, stream, P);
                    if (hipGetLastError() != hipSuccess) rc = set_error(WOST_ERR_DEVICE, "the kernel of the in-ball terms could not be launched");
                }
                if (rc != WOST_OK) {
                    (void)hipStreamSynchronize(stream);      // (the scratch arrays are freed on return)
                    return rc;
                }
            }
        }
        walk_pts = l.first;
        per_point = 1;
    }
    for (int64_t a = 0; a < N; a += cap, ++launches) {
        const ExitWalk w{walk_pts, (int32_t)a, (int32_t)std::min(cap, N - a), per_point, walk_seed_base, seed_width,
                         fresh.l.rec, static_cast<unsigned long long *>(d_counters)};
        if ((rc = c.walk(w, stream)) != WOST_OK) {
            (void)hipStreamSynchronize(stream);      // (the scratch arrays are freed on return)
            return rc;
        }
    }
    WOST_TRY(hipEventRecord(ev.b, stream));
    unsigned long long counters[5] = {0, 0, 0, 0, 0};
    WOST_TRY(hipMemcpyAsync(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipStreamSynchronize(stream));
    float ms = 0.0f;
    WOST_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    exits_free(*c.list);
    *c.list = fresh.l;
    fresh.l = ExitList{};
    if (stats) {
        stats->walk_steps = counters[0]; stats->walks_started = counters[1]; stats->walks_absorbed = counters[2];
        stats->walks_truncated = counters[3]; stats->neumann_hits = counters[4];
        stats->kernel_ms = ms;
        stats->kernel_launches = launches;
        stamp_solve_ms(stats, t0);
    }
    return WOST_OK;
}

int exits_walk(const ExitCall &c, const float *pts, bool pts_on_host, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width,
               hipStream_t stream, wost_stats *stats)
{
    return exits_walk_list(c, pts, pts_on_host, n, walks, ExitSeeds{0, walk_seed_base, seed_width}, false, stream, stats);
}

int exits_walk_gradient(const ExitCall &c, const float *pts, bool pts_on_host, int32_t n, int32_t walks, const ExitSeeds &seeds, hipStream_t stream,
                        wost_stats *stats)
{
    if (c.has_source && !c.source_term)
        return set_error(WOST_ERR_UNSUPPORTED, std::string(c.prefix) + "exits_walk_gradient: a scene with a source term is not covered without the option "
                                                                        "exits_grad_source (the in-ball term of the gradient does not depend on the Dirichlet "
                                                                        "data; with the option at 1 it is computed at the walk and carried in the list)");
    return exits_walk_list(c, pts, pts_on_host, n, walks, seeds, true, stream, stats);
}

int exits_grad_source_option(double value, bool *option)
{
    if (value != 0 && value != 1) return set_error(WOST_ERR_INVALID, "exits_grad_source must be 0 or 1");
    *option = value == 1;
    return WOST_OK;
}

int exits_gradient_terms(const ExitCall &c, double *T, double *seT, double *U)
{
    WOST_TRY(hipSetDevice(c.device));
    const ExitList &l = *c.list;
    const size_t n = (size_t)l.n, e3 = (size_t)l.dim * 3, per_point = 2 * e3 + 3;
    // T, seT and U are interleaved per point in the list: fetched whole and sorted on the host
    std::vector<double> terms(n * per_point);
    WOST_TRY(hipMemcpyAsync(terms.data(), l.terms, terms.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
    WOST_TRY(hipStreamSynchronize(c.stream));
    for (size_t i = 0; i < n; ++i) {
        const double *t = terms.data() + i * per_point;
        if (T) std::copy(t, t + e3, T + i * e3);
        if (seT) std::copy(t + e3, t + 2 * e3, seT + i * e3);
        if (U) std::copy(t + 2 * e3, t + per_point, U + i * 3);
    }
    return WOST_OK;
}

int exits_gradient_records(const ExitCall &c, const wost_exit_gradient_records &out)
{
    WOST_TRY(hipSetDevice(c.device));
    const ExitList &l = *c.list;
    const size_t n = (size_t)l.n, per_point = (size_t)l.S * (size_t)l.dim;
    // a point that is not finite has a NaN radius (and no other has); the kernel in front drew its directions all the same
    std::vector<float> radius(out.dirs ? n : 0);
    if (out.radius) WOST_TRY(hipMemcpyAsync(out.radius, l.radius, n * 4, hipMemcpyDeviceToHost, c.stream));
    if (out.dirs) {
        WOST_TRY(hipMemcpyAsync(radius.data(), l.radius, n * 4, hipMemcpyDeviceToHost, c.stream));
        WOST_TRY(hipMemcpyAsync(out.dirs, l.dirs, n * per_point * 4, hipMemcpyDeviceToHost, c.stream));
    }
    if (out.first_pts) WOST_TRY(hipMemcpyAsync(out.first_pts, l.first, n * per_point * 4, hipMemcpyDeviceToHost, c.stream));
    WOST_TRY(hipStreamSynchronize(c.stream));
    if (out.dirs)
        for (size_t i = 0; i < n; ++i)
            if (std::isnan(radius[i])) std::fill(out.dirs + i * per_point, out.dirs + (i + 1) * per_point, std::nanf(""));
    return WOST_OK;
}

static int exits_apply_gradient_dev(const ExitCall &c, const float *colors, int32_t K, float *grad, float *se, float *field, hipStream_t stream)
{
    const ExitList &l = *c.list;
    const ExitApplyGradParams P{l.rec, c.verts, colors, l.radius, l.dirs, l.n, l.S, K, c.n_verts, c.dirichlet_intensity, c.eps, grad, se, field, l.terms};
    const dim3 grid((unsigned)((l.n + 3) / 4));
    // (the list's mode, not the handle's option: what the walk recorded)
    if (l.terms) {
        if (c.dim == 2) hipLaunchKernelGGL((exits_apply_gradient_kernel<2, true>), grid, dim3(256), 0, stream, P);
        else hipLaunchKernelGGL((exits_apply_gradient_kernel<3, true>), grid, dim3(256), 0, stream, P);
    } else {
        if (c.dim == 2) hipLaunchKernelGGL((exits_apply_gradient_kernel<2, false>), grid, dim3(256), 0, stream, P);
        else hipLaunchKernelGGL((exits_apply_gradient_kernel<3, false>), grid, dim3(256), 0, stream, P);
    }
    WOST_TRY(hipGetLastError());
    return WOST_OK;
}

int exits_apply_gradient(const ExitCall &c, const float *colors, int32_t K, float *grad, float *se, float *field, bool on_host, hipStream_t stream)
{
    WOST_TRY(hipSetDevice(c.device));
    const size_t n_colors = (size_t)K * c.n_verts * 6, n_field = (size_t)K * c.list->n * 3, n_grad = n_field * (size_t)c.dim;
    if (!on_host) {
        const int rc = exits_apply_gradient_dev(c, colors, K, grad, se, field, stream);
        if (rc != WOST_OK) return rc;
        WOST_TRY(hipStreamSynchronize(stream));
        return WOST_OK;
    }
    Batch b{stream};
    float *d_colors = nullptr, *d_grad = nullptr, *d_se = nullptr, *d_field = nullptr;
    int rc = exits_stage(b, &d_colors, n_colors, "the colours");
    if (rc == WOST_OK) rc = exits_stage(b, &d_grad, n_grad, "the gradient");
    if (rc == WOST_OK && se) rc = exits_stage(b, &d_se, n_grad, "the standard errors");
    if (rc == WOST_OK && field) rc = exits_stage(b, &d_field, n_field, "the field");
    if (rc != WOST_OK) return rc;
    WOST_TRY(hipMemcpyAsync(d_colors, colors, n_colors * sizeof(float), hipMemcpyHostToDevice, stream));
    rc = exits_apply_gradient_dev(c, d_colors, K, d_grad, d_se, d_field, stream);
    if (rc != WOST_OK) {
        (void)hipStreamSynchronize(stream);      // (the scratch arrays are freed on return)
        return rc;
    }
    WOST_TRY(b.fetch(grad, d_grad, n_grad));
    WOST_TRY(b.fetch(se, d_se, n_grad));
    WOST_TRY(b.fetch(field, d_field, n_field));
    return b.finish();
}

// the frame all adjoints share: the input and the output staged for a host call, `launch` (the kernels from the input on the
// device to dcolors on the device; it may hand the batch scratch of its own), the fetch
static int exits_adjoint_frame(const ExitCall &c, const char *name, const float *in, size_t n_in, const char *in_name, int32_t K, float *dcolors, bool on_host,
                               hipStream_t stream, const std::function<int(Batch &b, const float *d_in, float *d_out)> &launch)
{
    if (c.n_verts <= 0)
        return set_error(WOST_ERR_UNSUPPORTED, std::string(c.prefix) + name + ": the scene has no Dirichlet mesh, so there are no colours to differentiate by");
    WOST_TRY(hipSetDevice(c.device));
    const size_t n_colors = (size_t)K * c.n_verts * 6;
    Batch b{stream};
    const float *d_in = in;
    float *d_out = dcolors;
    int rc = WOST_OK;
    if (on_host) {
        float *staged = nullptr;
        if ((rc = exits_stage(b, &staged, n_in, in_name)) != WOST_OK || (rc = exits_stage(b, &d_out, n_colors, "dcolors")) != WOST_OK) return rc;
        WOST_TRY(hipMemcpyAsync(staged, in, n_in * sizeof(float), hipMemcpyHostToDevice, stream));
        d_in = staged;
    }
    if ((rc = launch(b, d_in, d_out)) != WOST_OK) {
        (void)hipStreamSynchronize(stream);      // (the scratch arrays are freed on return)
        return rc;
    }
    if (on_host) WOST_TRY(b.fetch(dcolors, d_out, n_colors));
    return b.finish();
}

// the scattering adjoints in that frame: the zeroed fp64 sums, `scatter` (the atomic adds into acc), the rounding kernel
static int exits_adjoint_run(const ExitCall &c, const char *name, const float *in, size_t n_in, const char *in_name, int32_t K, float *dcolors, bool on_host,
                             hipStream_t stream, const std::function<void(const float *d_in, double *acc)> &scatter)
{
    const size_t n_colors = (size_t)K * std::max(c.n_verts, 0) * 6;
    return exits_adjoint_frame(c, name, in, n_in, in_name, K, dcolors, on_host, stream, [&](Batch &b, const float *d_in, float *d_out) {
        void *acc = nullptr;
        const int rc = exits_alloc(&acc, n_colors * sizeof(double), "the fp64 sums of the adjoint");
        if (rc != WOST_OK) return rc;
        b.scratch.ptrs.push_back(acc);
        WOST_TRY(hipMemsetAsync(acc, 0, n_colors * sizeof(double), stream));
        scatter(d_in, static_cast<double *>(acc));
        if (hipGetLastError() != hipSuccess) return set_error(WOST_ERR_DEVICE, "the adjoint kernel could not be launched");
        hipLaunchKernelGGL(exits_round_kernel, dim3((unsigned)((n_colors + 255) / 256)), dim3(256), 0, stream, static_cast<const double *>(acc), d_out, n_colors);
        if (hipGetLastError() != hipSuccess) return set_error(WOST_ERR_DEVICE, "the rounding kernel of the adjoint could not be launched");
        return (int)WOST_OK;
    });
}

// the gathering adjoints in that frame: one kernel, one wave per (bin, set), straight into dcolors
static int exits_ordered_run(const ExitCall &c, const char *name, const float *in, size_t n_in, const char *in_name, int32_t K, float *dcolors, bool on_host,
                             hipStream_t stream, bool gradient)
{
    const ExitList &l = *c.list;
    return exits_adjoint_frame(c, name, in, n_in, in_name, K, dcolors, on_host, stream, [&](Batch &, const float *d_in, float *d_out) {
        const ExitOrderedParams P{l.rec, c.verts, d_in, l.radius, l.dirs, l.index.nbar, l.index.bin_begin, l.index.inc, l.n, l.S, K, c.n_verts,
                                  c.dirichlet_intensity, c.eps, d_out};
        const size_t waves = 2 * (size_t)c.n_verts * (size_t)K;
        if ((waves + 3) / 4 > 0x7fffffffu) return set_error(WOST_ERR_INVALID, std::string(c.prefix) + name + ": K * n_verts is too large for one launch");
        const dim3 grid((unsigned)((waves + 3) / 4));
        if (gradient) {
            if (c.dim == 2) hipLaunchKernelGGL(exits_adjoint_gradient_ordered_kernel<2>, grid, dim3(256), 0, stream, P);
            else hipLaunchKernelGGL(exits_adjoint_gradient_ordered_kernel<3>, grid, dim3(256), 0, stream, P);
        } else {
            if (c.dim == 2) hipLaunchKernelGGL(exits_adjoint_ordered_kernel<2>, grid, dim3(256), 0, stream, P);
            else hipLaunchKernelGGL(exits_adjoint_ordered_kernel<3>, grid, dim3(256), 0, stream, P);
        }
        if (hipGetLastError() != hipSuccess) return set_error(WOST_ERR_DEVICE, "the ordered adjoint kernel could not be launched");
        return (int)WOST_OK;
    });
}

int exits_adjoint_ordered(const ExitCall &c, const float *dfield, int32_t K, float *dcolors, bool on_host, hipStream_t stream)
{
    return exits_ordered_run(c, "exits_adjoint_ordered", dfield, (size_t)K * c.list->n * 3, "dfield", K, dcolors, on_host, stream, false);
}

int exits_adjoint_gradient_ordered(const ExitCall &c, const float *dgrad, int32_t K, float *dcolors, bool on_host, hipStream_t stream)
{
    return exits_ordered_run(c, "exits_adjoint_gradient_ordered", dgrad, (size_t)K * c.list->n * 3 * (size_t)c.dim, "dgrad", K, dcolors, on_host, stream, true);
}

int exits_adjoint_gradient(const ExitCall &c, const float *dgrad, int32_t K, float *dcolors, bool on_host, hipStream_t stream)
{
    const ExitList &l = *c.list;
    return exits_adjoint_run(c, "exits_adjoint_gradient", dgrad, (size_t)K * l.n * 3 * (size_t)c.dim, "dgrad", K, dcolors, on_host, stream,
                             [&](const float *d_dgrad, double *acc) {
                                 const ExitAdjointGradParams P{l.rec, c.verts, d_dgrad, l.radius, l.dirs, l.n, l.S, K, c.n_verts, c.dirichlet_intensity, c.eps, acc};
                                 const dim3 grid((unsigned)((l.n + 3) / 4));
                                 if (c.dim == 2) hipLaunchKernelGGL(exits_adjoint_gradient_kernel<2>, grid, dim3(256), 0, stream, P);
                                 else hipLaunchKernelGGL(exits_adjoint_gradient_kernel<3>, grid, dim3(256), 0, stream, P);
                             });
}

int exits_records(const ExitCall &c, const wost_exit_records &out)
{
    WOST_TRY(hipSetDevice(c.device));
    const ExitList &l = *c.list;
    const size_t N = (size_t)l.n * l.S, uvs = (size_t)l.dim - 1;
    // uv and base are interleaved per walk for the caller: fetched array by array and woven on the host
    std::vector<float> uv(out.uv ? N * uvs : 0), base(out.base_rgb ? N * 3 : 0);
    if (out.prim) WOST_TRY(hipMemcpyAsync(out.prim, l.rec.prim(), N * 4, hipMemcpyDeviceToHost, c.stream));
    if (out.side) WOST_TRY(hipMemcpyAsync(out.side, l.rec.side(), N * 4, hipMemcpyDeviceToHost, c.stream));
    if (out.thp) WOST_TRY(hipMemcpyAsync(out.thp, l.rec.thp(), N * 4, hipMemcpyDeviceToHost, c.stream));
    if (out.uv) WOST_TRY(hipMemcpyAsync(uv.data(), l.rec.uv(0), N * uvs * 4, hipMemcpyDeviceToHost, c.stream));
    if (out.base_rgb) WOST_TRY(hipMemcpyAsync(base.data(), l.rec.base(l.dim, 0), N * 3 * 4, hipMemcpyDeviceToHost, c.stream));
    WOST_TRY(hipStreamSynchronize(c.stream));
    if (out.uv)
        for (size_t w = 0; w < N; ++w)
            for (size_t k = 0; k < uvs; ++k) out.uv[w * uvs + k] = uv[k * N + w];
    if (out.base_rgb)
        for (size_t w = 0; w < N; ++w)
            for (size_t k = 0; k < 3; ++k) out.base_rgb[w * 3 + k] = base[k * N + w];
    return WOST_OK;
}

static int exits_apply_dev(const ExitCall &c, const float *colors, int32_t K, float *field, float *se, hipStream_t stream)
{
    const ExitList &l = *c.list;
    const ExitApplyParams P{l.rec, c.verts, colors, l.n, l.S, K, c.n_verts, c.dirichlet_intensity, field, se};
    const dim3 grid((unsigned)((l.n + 3) / 4));
    if (c.dim == 2) hipLaunchKernelGGL(exits_apply_kernel<2>, grid, dim3(256), 0, stream, P);
    else hipLaunchKernelGGL(exits_apply_kernel<3>, grid, dim3(256), 0, stream, P);
    WOST_TRY(hipGetLastError());
    return WOST_OK;
}

int exits_apply(const ExitCall &c, const float *colors, int32_t K, float *field, float *stderr_rgb, bool on_host, hipStream_t stream)
{
    WOST_TRY(hipSetDevice(c.device));
    const size_t n_colors = (size_t)K * c.n_verts * 6, n_field = (size_t)K * c.list->n * 3;
    if (!on_host) {
        const int rc = exits_apply_dev(c, colors, K, field, stderr_rgb, stream);
        if (rc != WOST_OK) return rc;
        WOST_TRY(hipStreamSynchronize(stream));
        return WOST_OK;
    }
    Batch b{stream};
    float *d_colors = nullptr, *d_field = nullptr, *d_se = nullptr;
    int rc = exits_stage(b, &d_colors, n_colors, "the colours");
    if (rc == WOST_OK) rc = exits_stage(b, &d_field, n_field, "the field");
    if (rc == WOST_OK && stderr_rgb) rc = exits_stage(b, &d_se, n_field, "the standard errors");
    if (rc != WOST_OK) return rc;
    WOST_TRY(hipMemcpyAsync(d_colors, colors, n_colors * sizeof(float), hipMemcpyHostToDevice, stream));
    rc = exits_apply_dev(c, d_colors, K, d_field, d_se, stream);
    if (rc != WOST_OK) {
        (void)hipStreamSynchronize(stream);      // (the scratch arrays are freed on return)
        return rc;
    }
    WOST_TRY(b.fetch(field, d_field, n_field));
    WOST_TRY(b.fetch(stderr_rgb, d_se, n_field));
    return b.finish();
}

int exits_adjoint(const ExitCall &c, const float *dfield, int32_t K, float *dcolors, bool on_host, hipStream_t stream)
{
    const ExitList &l = *c.list;
    return exits_adjoint_run(c, "exits_adjoint", dfield, (size_t)K * l.n * 3, "dfield", K, dcolors, on_host, stream, [&](const float *d_dfield, double *acc) {
        const ExitAdjointParams P{l.rec, c.verts, d_dfield, l.n, l.S, K, c.n_verts, c.dirichlet_intensity, acc};
        const dim3 grid((unsigned)(((size_t)l.n * l.S + 255) / 256));
        if (c.dim == 2) hipLaunchKernelGGL(exits_adjoint_kernel<2>, grid, dim3(256), 0, stream, P);
        else hipLaunchKernelGGL(exits_adjoint_kernel<3>, grid, dim3(256), 0, stream, P);
    });
}

}  // namespace wost
