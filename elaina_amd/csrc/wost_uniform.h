// wost_uniform.h -- what the 2-D and the 3-D uniform handle share on the host (not part of the C-ABI): the members both contexts
// have (HandleBase) with the shared part of their creation and destruction, the bodies of the frame and point solves
// (UniformCalls, in the manner of CarryCalls, wost_carry.h) and the bodies of the five batch queries (query_*).  A dimension
// supplies its context, the functions that call its solve driver and the launches of its query kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <new>

#include "../../include/wost.h"
#include "wost_internal.h"
#include "wost_carry.h"
#include "wost_grad.h"
#include "wost_exits.h"

namespace wost {

// ---- the handle ----
// The members of wost_context and wost3_context that the shared bodies read (CarryCalls, PointListCtx, GradCall, UniformCalls,
// the queries); the meshes, the probe and the source term have a type per dimension and stay with the contexts.
struct HandleBase {
    int device = 0;
    wost_settings settings{};
    DevSettings dst{};
    uint8_t *mask = nullptr;        // device, width * height bytes, or nullptr
    size_t n_pixels = 0;
    float *field = nullptr;         // n_pixels * 3 (the host calls solve into it)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    CarryState carry;               // the carried frame solve (wost_solve_more & co., wost_carry.h)
    PointList list;                 // ... and, beside it, the carried point list (wost_points_carry & co.)
    GradScratch grad;               // the scratch of the gradient calls (wost_solve_gradient_points & co., wost_grad.h)
    GradList glist;                 // ... and the carried gradient list (wost_gradient_points_carry & co.), which shares it
    bool grad_source = false;       // the option "grad_source": the gradient calls take a scene with a source term (GradCall)
    bool exits_grad_source = false; // the option "exits_grad_source": a walk of the gradient's exit list takes such a scene (ExitCall)
    ExitList exits;                 // the exit list (wost_exits_walk & co., wost_exits.h), beside the three carried states
    int32_t dirichlet_verts = 0;    // ... and the vertices of the Dirichlet mesh, which size a set of its colours (0: no such mesh)
};

// (hidden: the dynamic symbol table of the library stays the C-ABI and what it held before; nothing here joins it)
#pragma GCC visibility push(hidden)

// the shared end of a handle: a dimension sets the device, frees its own members, calls this and deletes the context
inline void destroy_base(HandleBase *c)
{
    if (c->mask) (void)hipFree(c->mask);
    if (c->field) (void)hipFree(c->field);
    carry_free(c->carry);
    points_free(c->list);
    grad_free(c->grad);
    gradlist_free(c->glist);
    exits_free(c->exits);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
}

// the mask of the frame on the device (nullptr: none) ...
inline int upload_mask(HandleBase *c, const uint8_t *mask)
{
    if (!mask) return WOST_OK;
    WOST_TRY(hipMalloc((void **)&c->mask, c->n_pixels));
    WOST_TRY(hipMemcpy(c->mask, mask, c->n_pixels, hipMemcpyHostToDevice));
    return WOST_OK;
}
// ... and the field, the stream and the events of the host calls
inline int create_frame(HandleBase *c)
{
    WOST_TRY(hipMalloc((void **)&c->field, c->n_pixels * 3 * sizeof(float)));
    WOST_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    WOST_TRY(hipEventCreate(&c->ev0));
    WOST_TRY(hipEventCreate(&c->ev1));
    return WOST_OK;
}

// wost_create / wost3_create.  The shared part: the argument rules in the order of include/wost.h, the device and the context
// with its settings.  A dimension adds `fill` -- its probe, meshes, source term and buffers, with upload_mask and create_frame
// at the place they have among its own allocations: device memory and streams are made in the order they always were, which
// the addresses of the buffers and the hardware queues of the streams follow -- and `destroy`, which releases the context on
// every failure path.  packed_walker: 2-D keeps a walker's sample and depth in 20 and
// 10 bits of one word (META_PACK) and refuses what does not fit; a 3-D lane counts in registers and has no such limit.
template <class Ctx, class Scene>
int create_handle(const Scene *scene, const wost_settings *settings, int device, Ctx **out, bool packed_walker, void (*destroy)(Ctx *),
                  int (*fill)(Ctx *, const Scene &))
{
    if (!scene || !settings || !out) return set_error(WOST_ERR_INVALID, "null argument");
    *out = nullptr;
    if (settings->width <= 0 || settings->height <= 0 || settings->spp < 0 || settings->max_depth <= 0)
        return set_error(WOST_ERR_INVALID, "bad settings");
    if (packed_walker && (settings->spp >= (1 << 20) || settings->max_depth >= (1 << 10)))
        return set_error(WOST_ERR_UNSUPPORTED, "spp must be < 2^20 and max_depth < 2^10");
    if ((int64_t)settings->width * settings->height > (1 << 28)) return set_error(WOST_ERR_UNSUPPORTED, "frame too large");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return set_error(WOST_ERR_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= n_dev) return set_error(WOST_ERR_INVALID, "device index out of range");
    WOST_TRY(hipSetDevice(device));
    std::unique_ptr<Ctx, void (*)(Ctx *)> c(new (std::nothrow) Ctx(), destroy);
    if (!c) return set_error(WOST_ERR_NOMEM, "out of host memory");
    c->device = device;
    c->settings = *settings;
    c->dst = DevSettings{settings->width, settings->height, settings->spp, settings->max_depth, settings->eps_shell,
                         scene->dirichlet_intensity, scene->neumann_intensity};
    c->n_pixels = (size_t)settings->width * settings->height;
    const int rc = fill(c.get(), *scene);
    if (rc != WOST_OK) return rc;
    *out = c.release();
    return WOST_OK;
}

// the mesh a query names, or nullptr for an unknown selector
template <class Ctx>
auto *pick_mesh(Ctx *h, int which)
{
    return which == WOST_MESH_DIRICHLET ? &h->dm : which == WOST_MESH_NEUMANN ? &h->nm : nullptr;
}

// ---- the frame and point solves, written once for the 2-D and the 3-D context ----
// Ctx has device, n_pixels, field and stream.  What a dimension adds: the coordinates of a point and two functions that call its
// solve driver -- a frame step on a pixel range and a shard, and a point step on a device list (2-D cuts it into chunks).
template <class Ctx>
struct UniformCalls {
    int dim;
    int (*frame)(Ctx *c, int32_t pixel_begin, int32_t pixel_end, int32_t shard_index, int32_t shard_count, float *field_dev, int32_t field_base,
                 hipStream_t stream, wost_stats *stats);
    int (*points)(Ctx *c, const float *pts_dev, int32_t n, int32_t seed_base, int32_t seed_width, float *field_dev, hipStream_t stream,
                  wost_stats *stats);

    int solve(Ctx *h, int32_t pixel_begin, int32_t pixel_end, float *field_rgb, wost_stats *stats) const
    {
        if (!h || !field_rgb) return set_error(WOST_ERR_INVALID, "null argument");
        if (pixel_begin < 0 || pixel_end > (int64_t)h->n_pixels || pixel_begin > pixel_end)
            return set_error(WOST_ERR_INVALID, "pixel range outside the frame");
        const auto t0 = HostClock::now();
        const size_t n = (size_t)(pixel_end - pixel_begin);
        if (n == 0) {
            if (stats) std::memset(stats, 0, sizeof(*stats));
            return WOST_OK;
        }
        WOST_TRY(hipSetDevice(h->device));
        WOST_TRY(hipMemsetAsync(h->field, 0, n * 3 * sizeof(float), h->stream));
        const int rc = frame(h, pixel_begin, pixel_end, 0, 1, h->field, pixel_begin, h->stream, stats);
        if (rc != WOST_OK) return rc;
        WOST_TRY(hipMemcpyAsync(field_rgb, h->field, n * 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        WOST_TRY(hipStreamSynchronize(h->stream));
        stamp_solve_ms(stats, t0);
        return WOST_OK;
    }
    // (a null stream is the legacy default stream, which is also torch's default stream)
    int solve_sharded(Ctx *h, int32_t shard_index, int32_t shard_count, float *field_rgb_dev, void *stream, wost_stats *stats) const
    {
        if (!h || !field_rgb_dev) return set_error(WOST_ERR_INVALID, "null argument");
        if (shard_count <= 0 || shard_index < 0 || shard_index >= shard_count) return set_error(WOST_ERR_INVALID, "bad shard");
        return frame(h, 0, (int32_t)h->n_pixels, shard_index, shard_count, field_rgb_dev, 0, reinterpret_cast<hipStream_t>(stream), stats);
    }
    int solve_points_dev(Ctx *h, const float *pts_dev, int32_t n, int32_t seed_base, int32_t seed_width, float *field_rgb_dev, void *stream,
                         wost_stats *stats) const
    {
        const int rc = check_point_solve(h, pts_dev, field_rgb_dev, n, seed_base, seed_width);
        if (rc != WOST_OK) return rc;
        if (stats) std::memset(stats, 0, sizeof(*stats));
        if (n == 0) return WOST_OK;
        return points(h, pts_dev, n, seed_base, seed_width, field_rgb_dev, reinterpret_cast<hipStream_t>(stream), stats);
    }
    int solve_points(Ctx *h, const float *pts, int32_t n, int32_t seed_base, int32_t seed_width, float *field_rgb, wost_stats *stats) const
    {
        int rc = check_point_solve(h, pts, field_rgb, n, seed_base, seed_width);
        if (rc == WOST_OK) rc = check_points_finite(pts, n, dim);
        if (rc != WOST_OK) return rc;
        if (stats) std::memset(stats, 0, sizeof(*stats));
        if (n == 0) return WOST_OK;
        const auto t0 = HostClock::now();
        WOST_TRY(hipSetDevice(h->device));
        Batch b{h->stream};
        float *d_pts, *d_field;
        WOST_TRY(b.in(pts, (size_t)n * dim, &d_pts));
        WOST_TRY(b.out(&d_field, (size_t)n * 3));
        WOST_TRY(hipMemsetAsync(d_field, 0, (size_t)n * 3 * sizeof(float), h->stream));
        rc = points(h, d_pts, n, seed_base, seed_width, d_field, h->stream, stats);
        if (rc != WOST_OK) {
            (void)hipStreamSynchronize(h->stream);      // (the scratch arrays are freed on return)
            return rc;
        }
        WOST_TRY(b.fetch(field_rgb, d_field, (size_t)n * 3));
        if ((rc = b.finish()) == WOST_OK) stamp_solve_ms(stats, t0);
        return rc;
    }
};

// ---- the batch queries, written once for the 2-D and the 3-D context ----
// Q is what a dimension adds: dim, the coordinates of a point; uv, the floats of a closest point's parameter; count(view), the
// primitives of a mesh; and the launches of its five kernels on the handle's stream, each given the LDS of its stack columns.
// Q::sdf_out names the device array render_sdf fills: 2-D reuses the handle's field, 3-D takes scratch.

// the stack columns (stack_lds, wost_host.h) of a mesh that may be empty
template <class Q, class View>
size_t stack_lds_of(const View &v) { return stack_lds(Q::count(v) > 0 ? v.levels : 1); }

template <class Q, class Ctx>
int query_closest_point(Ctx *h, int which_mesh, const float *pts, int32_t n, int32_t *out_idx, float *out_dist, float *out_uv, int32_t *out_side)
{
    if (!h || !pts || n < 0) return set_error(WOST_ERR_INVALID, "null argument");
    auto *m = pick_mesh(h, which_mesh);
    if (!m || Q::count(m->view) == 0) return set_error(WOST_ERR_INVALID, "mesh is empty or unknown");
    if (n == 0) return WOST_OK;
    WOST_TRY(hipSetDevice(h->device));
    Batch b{h->stream};
    float *d_pts, *d_dist, *d_uv;
    int32_t *d_idx, *d_side;
    const size_t n_uv = (size_t)n * Q::uv;
    WOST_TRY(b.in(pts, (size_t)n * Q::dim, &d_pts)); WOST_TRY(b.out(&d_dist, n)); WOST_TRY(b.out(&d_uv, n_uv));
    WOST_TRY(b.out(&d_idx, n)); WOST_TRY(b.out(&d_side, n));
    Q::closest_point(h, m->view, stack_lds(m->view.levels), d_pts, n, d_idx, d_dist, d_uv, d_side);
    WOST_TRY(hipGetLastError());
    WOST_TRY(b.fetch(out_idx, d_idx, n));
    WOST_TRY(b.fetch(out_dist, d_dist, n));
    WOST_TRY(b.fetch(out_uv, d_uv, n_uv));
    WOST_TRY(b.fetch(out_side, d_side, n));
    return b.finish();
}

template <class Q, class Ctx>
int query_closest_silhouette(Ctx *h, int which_mesh, const float *pts, const float *rmax, int32_t n, float *out_dist)
{
    if (!h || !pts || !out_dist || n < 0) return set_error(WOST_ERR_INVALID, "null argument");
    auto *m = pick_mesh(h, which_mesh);
    if (!m) return set_error(WOST_ERR_INVALID, "unknown mesh selector");
    if (n == 0) return WOST_OK;
    WOST_TRY(hipSetDevice(h->device));
    Batch b{h->stream};
    float *d_pts, *d_rmax = nullptr, *d_out;
    WOST_TRY(b.in(pts, (size_t)n * Q::dim, &d_pts)); WOST_TRY(b.out(&d_out, n));
    if (rmax) WOST_TRY(b.in(rmax, n, &d_rmax));
    Q::silhouette(h, m->view, stack_lds_of<Q>(m->view), d_pts, d_rmax, n, d_out);
    WOST_TRY(hipGetLastError());
    WOST_TRY(b.fetch(out_dist, d_out, n));
    return b.finish();
}

template <class Q, class Ctx>
int query_ray_intersect(Ctx *h, int which_mesh, const float *origins, const float *dirs, const float *tmax, int32_t n, int32_t *out_hit,
                        float *out_t, int32_t *out_idx)
{
    if (!h || !origins || !dirs || !tmax || !out_hit || !out_t || !out_idx || n < 0) return set_error(WOST_ERR_INVALID, "null argument");
    auto *m = pick_mesh(h, which_mesh);
    if (!m) return set_error(WOST_ERR_INVALID, "unknown mesh selector");
    if (n == 0) return WOST_OK;
    WOST_TRY(hipSetDevice(h->device));
    Batch b{h->stream};
    float *d_o, *d_d, *d_tm, *d_t;
    int32_t *d_hit, *d_idx;
    WOST_TRY(b.in(origins, (size_t)n * Q::dim, &d_o)); WOST_TRY(b.in(dirs, (size_t)n * Q::dim, &d_d)); WOST_TRY(b.in(tmax, n, &d_tm));
    WOST_TRY(b.out(&d_t, n)); WOST_TRY(b.out(&d_hit, n)); WOST_TRY(b.out(&d_idx, n));
    Q::ray(h, m->view, stack_lds_of<Q>(m->view), d_o, d_d, d_tm, n, d_hit, d_t, d_idx);
    WOST_TRY(hipGetLastError());
    WOST_TRY(b.fetch(out_hit, d_hit, n));
    WOST_TRY(b.fetch(out_t, d_t, n));
    WOST_TRY(b.fetch(out_idx, d_idx, n));
    return b.finish();
}

template <class Q, class Ctx>
int query_render_sdf(Ctx *h, int which_mesh, float *out_dist)
{
    if (!h || !out_dist) return set_error(WOST_ERR_INVALID, "null argument");
    auto *m = pick_mesh(h, which_mesh);
    if (!m) return set_error(WOST_ERR_INVALID, "unknown mesh selector");
    WOST_TRY(hipSetDevice(h->device));
    const int n = (int)h->n_pixels;
    Batch b{h->stream};
    float *d_out;
    WOST_TRY(Q::sdf_out(h, b, n, &d_out));
    Q::sdf(h, m->view, which_mesh, stack_lds_of<Q>(m->view), n, d_out);
    WOST_TRY(hipGetLastError());
    WOST_TRY(b.fetch(out_dist, d_out, (size_t)n));
    return b.finish();
}

template <class Q, class Ctx>
int query_render_source(Ctx *h, float *out_rgb)
{
    if (!h || !out_rgb) return set_error(WOST_ERR_INVALID, "null argument");
    WOST_TRY(hipSetDevice(h->device));
    const int n = (int)h->n_pixels;
    Batch b{h->stream};
    float *d_out;
    WOST_TRY(b.out(&d_out, (size_t)n * 3));
    Q::source(h, n, d_out);
    WOST_TRY(hipGetLastError());
    WOST_TRY(b.fetch(out_rgb, d_out, (size_t)n * 3));
    return b.finish();
}

#pragma GCC visibility pop

}  // namespace wost
