// wost_carry.h -- the carried frame solve behind wost_solve_more & co., shared by the 2-D and the 3-D
// context: the per-pixel state, the kernel that closes a continued call (wost_carry.hip) and the drivers of the calls that
// continue a selection of pixels or stop by a per-pixel error estimate; and the carried point list behind wost_points_carry & co.
// (DESIGN 4.3e), which is the same state and the same drivers on a caller's points.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>

#include "../../include/wost.h"
#include "wost_internal.h"

namespace wost {

// What a handle carries.  Per pixel 52 bytes, allocated on the first continued call, zeroed then and after a restart:
//   rng      the PCG32 state after the pixel's samples so far            sum[3]   the raw fp32 sums of those samples
//   n        the samples done in this pixel                              batches  K, the continued calls that walked it
//   prev[3]  the sums as they stood after the previous batch             q[3]     sum over the batches of b_k^2 / m_k
// and, allocated when a call first needs them, the work buffers of a selection: the map the next call walks (sel), a caller's
// map on its way to the device (want), the selected pixel ids (ids, what the 3-D lanes read), standard errors (se), a count.
struct CarryState {
    void *mem = nullptr, *work = nullptr;
    uint64_t *rng = nullptr;
    float *sum = nullptr, *prev = nullptr, *q = nullptr;
    uint32_t *n = nullptr, *batches = nullptr;
    uint8_t *sel = nullptr, *want = nullptr;
    int32_t *ids = nullptr;
    float *se = nullptr;
    uint32_t *count = nullptr;
    bool stale = false;        // restarted or dropped: the 52 bytes are zeroed before their next use
    // the sum of more_spp over the calls since the restart (wost_solve_progress) and the shard they belong to (count 0: none yet)
    int32_t done = 0, shard_index = 0, shard_count = 0;
    uint32_t walks = 0;        // walks the running call has made so far (a driver's second walk appends to the launch list)
};

// the frame of the handle: what the kernel needs to know a pixel's owner and whether it is masked
struct CarryFrame {
    int device;
    int32_t width, height;
    const uint8_t *mask;       // device, width * height bytes, or nullptr
    bool nan_masked = false;   // a masked entry's field is NaN, not 0: the frame of a point list, masked where a point is not finite
};

// One walk of a driver: more_spp samples on the pixels of the device map sel (nullptr: every pixel of the shard) -- n_sel of
// them, their ids in `ids` -- into field_dev; WOST_OK or the error of the solve, recorded.
using CarryWalk = std::function<int(int32_t more_spp, const uint8_t *sel, const int32_t *ids, uint32_t n_sel, float *field_dev,
                                    hipStream_t stream, wost_stats *stats)>;

void carry_free(CarryState &s);
void carry_restart(CarryState &s);

// the argument rules that need no look at the handle (include/wost.h), in the order and words of wost_solve_more
int carry_check_more(const void *h, const void *field, int32_t more_spp);
int carry_check_shard(int32_t shard_index, int32_t shard_count);
int carry_check_adaptive(const void *h, const wost_adaptive *a, const void *field);

// wost_solve_more_where(_sharded): select (select_on_host: width * height host bytes, else device bytes; nullptr: every pixel)
int carry_more_where(CarryState &s, const CarryFrame &f, int32_t shard_index, int32_t shard_count, int32_t more_spp, const uint8_t *select,
                     bool select_on_host, float *field_dev, hipStream_t stream, wost_stats *stats, const CarryWalk &walk, const char *prefix);
// wost_solve_adaptive(_sharded): select, walk batch_spp samples on the selection, close and select again, until nothing is selected
int carry_adaptive(CarryState &s, const CarryFrame &f, int32_t shard_index, int32_t shard_count, const wost_adaptive &a, float *field_dev,
                   hipStream_t stream, wost_stats *stats, const CarryWalk &walk, const char *prefix);
// wost_solve_carried: host arrays, any of them nullptr
int carry_read(CarryState &s, const CarryFrame &f, int32_t *spp, int32_t *batches, float *sum_rgb, float *stderr_rgb, hipStream_t stream);

// (a context whose masked entries answer NaN has an overload of its own: PointListCtx below)
inline bool carry_nan_masked(const void *) { return false; }

// ---- the carried point list behind wost_points_carry & co.: the library's copy of the caller's points, the map
// of the finite ones (built once at bind time; it takes the place of the frame's mask), the list's own field and its own carried
// state.  dim is 2 or 3.  Beside the carried frame solve of the handle, never mixed with it.
struct PointList {
    float *pts = nullptr;        // device, n * dim floats
    uint8_t *finite = nullptr;   // device, n bytes: 0 where a coordinate is not finite
    float *field = nullptr;      // device, n * 3 floats
    int32_t n = 0, seed_base = 0, seed_width = 1;
    CarryState carry;
};
void points_free(PointList &l);
// the argument rules of a bind that need no look at the handle, in the order of include/wost.h
int points_check_bind(const void *h, const float *pts, int32_t n, int32_t seed_base, int32_t seed_width);
// wost_points_carry(_dev): the new list replaces the old one when every allocation and copy has succeeded; n == 0 releases
int points_bind(PointList &l, int device, int dim, const float *pts, bool pts_on_host, int32_t n, int32_t seed_base, int32_t seed_width,
                hipStream_t stream);

// What CarryCalls reads of a context, for the list of handle H: a frame n wide and 1 high in one shard -- carry_kernel's tile
// formula then owns every point -- masked by the map of the finite points.
template <class H>
struct PointListCtx {
    H *h;
    int device;
    struct { int32_t width, height; } settings;
    const uint8_t *mask;
    size_t n_pixels;
    float *field;
    hipStream_t stream;
    CarryState &carry;
    explicit PointListCtx(H *handle)
        : h(handle), device(handle->device), settings{handle->list.n, 1}, mask(handle->list.finite), n_pixels((size_t)handle->list.n),
          field(handle->list.field), stream(handle->stream), carry(handle->list.carry) {}
};
template <class H>
inline bool carry_nan_masked(const PointListCtx<H> *) { return true; }

// ---- the entry points of the continued solve, written once for the 2-D and the 3-D context ----
// Ctx has device, settings, mask, n_pixels, field, stream and carry.  What a dimension adds: the prefix of its entry points in
// messages, the walk of a shard (it calls the dimension's solve driver) and, optionally, what a call that made no walk has
// to tidy up (2-D: the launch list, which would still be that of the solve before it).
template <class Ctx>
struct CarryCalls {
    const char *prefix;
    CarryWalk (*walk)(Ctx *c, int32_t shard_index, int32_t shard_count);
    void (*no_walk)(Ctx *c);

    static CarryFrame frame(const Ctx *c) { return CarryFrame{c->device, c->settings.width, c->settings.height, c->mask, carry_nan_masked(c)}; }
    int driven(Ctx *h, int rc) const
    {
        if (rc == WOST_OK && no_walk && h->carry.walks == 0) no_walk(h);
        return rc;
    }
    // the field of a host call: the handle's device field, zero-filled; after the call it travels to the caller
    static int host_field_begin(Ctx *c)
    {
        WOST_TRY(hipSetDevice(c->device));
        WOST_TRY(hipMemsetAsync(c->field, 0, c->n_pixels * 3 * sizeof(float), c->stream));
        return WOST_OK;
    }
    static int host_field_end(Ctx *c, float *field_rgb, wost_stats *stats, HostClock::time_point t0)
    {
        WOST_TRY(hipMemcpyAsync(field_rgb, c->field, c->n_pixels * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        WOST_TRY(hipStreamSynchronize(c->stream));
        stamp_solve_ms(stats, t0);
        return WOST_OK;
    }

    int more_where(Ctx *h, int32_t more_spp, const uint8_t *select, float *field_rgb, wost_stats *stats) const
    {
        int rc = carry_check_more(h, field_rgb, more_spp);
        if (rc != WOST_OK) return rc;
        const auto t0 = HostClock::now();
        if ((rc = host_field_begin(h)) != WOST_OK) return rc;
        rc = driven(h, carry_more_where(h->carry, frame(h), 0, 1, more_spp, select, true, h->field, h->stream, stats, walk(h, 0, 1), prefix));
        return rc != WOST_OK ? rc : host_field_end(h, field_rgb, stats, t0);
    }
    int more_where_sharded(Ctx *h, int32_t shard_index, int32_t shard_count, int32_t more_spp, const uint8_t *select_dev, float *field_rgb_dev,
                           void *stream, wost_stats *stats) const
    {
        int rc = carry_check_more(h, field_rgb_dev, more_spp);
        if (rc == WOST_OK) rc = carry_check_shard(shard_index, shard_count);
        if (rc != WOST_OK) return rc;
        return driven(h, carry_more_where(h->carry, frame(h), shard_index, shard_count, more_spp, select_dev, false, field_rgb_dev,
                                          reinterpret_cast<hipStream_t>(stream), stats, walk(h, shard_index, shard_count), prefix));
    }
    int adaptive_sharded(Ctx *h, int32_t shard_index, int32_t shard_count, const wost_adaptive *a, float *field_rgb_dev, void *stream,
                         wost_stats *stats) const
    {
        int rc = carry_check_adaptive(h, a, field_rgb_dev);
        if (rc == WOST_OK) rc = carry_check_shard(shard_index, shard_count);
        if (rc != WOST_OK) return rc;
        return driven(h, carry_adaptive(h->carry, frame(h), shard_index, shard_count, *a, field_rgb_dev, reinterpret_cast<hipStream_t>(stream), stats,
                                        walk(h, shard_index, shard_count), prefix));
    }
    int adaptive(Ctx *h, const wost_adaptive *a, float *field_rgb, float *stderr_rgb, int32_t *spp_map, wost_stats *stats) const
    {
        int rc = carry_check_adaptive(h, a, field_rgb);
        if (rc != WOST_OK) return rc;
        const auto t0 = HostClock::now();
        if ((rc = host_field_begin(h)) != WOST_OK) return rc;
        rc = driven(h, carry_adaptive(h->carry, frame(h), 0, 1, *a, h->field, h->stream, stats, walk(h, 0, 1), prefix));
        if (rc != WOST_OK) return rc;
        if ((stderr_rgb || spp_map) && (rc = carry_read(h->carry, frame(h), spp_map, nullptr, nullptr, stderr_rgb, h->stream)) != WOST_OK) return rc;
        return host_field_end(h, field_rgb, stats, t0);
    }
    int carried(Ctx *h, int32_t *spp, int32_t *batches, float *sum_rgb, float *stderr_rgb) const
    {
        if (!h) return set_error(WOST_ERR_INVALID, "null argument");
        return carry_read(h->carry, frame(h), spp, batches, sum_rgb, stderr_rgb, h->stream);
    }
    int restart(Ctx *h) const
    {
        if (!h) return set_error(WOST_ERR_INVALID, "null argument");
        carry_restart(h->carry);
        return WOST_OK;
    }
    int progress(Ctx *h, int32_t *spp_done) const
    {
        if (!h || !spp_done) return set_error(WOST_ERR_INVALID, "null argument");
        *spp_done = h->carry.done;
        return WOST_OK;
    }
};

// ---- the entry points of the carried point list, written once for the 2-D and the 3-D handle ----
// H has device, stream and list.  What a dimension adds: its prefix, the columns of a point and the walk of the list.
template <class H>
struct PointCalls {
    CarryCalls<PointListCtx<H>> calls;
    int dim;

    // a call that needs a bound list (after the argument rules that need no look at the handle)
    static int bound(const H *h)
    {
        if (h->list.n <= 0) return set_error(WOST_ERR_INVALID, "no point list is bound to the handle (points_carry binds one)");
        return WOST_OK;
    }
    // host points travel on the handle's stream, device points on the caller's
    int bind(H *h, const float *pts, bool pts_on_host, int32_t n, int32_t seed_base, int32_t seed_width, void *stream) const
    {
        int rc = points_check_bind(h, pts, n, seed_base, seed_width);
        if (rc == WOST_OK && pts_on_host) rc = check_points_finite(pts, n, dim);
        if (rc != WOST_OK) return rc;
        return points_bind(h->list, h->device, dim, pts, pts_on_host, n, seed_base, seed_width,
                           pts_on_host ? h->stream : reinterpret_cast<hipStream_t>(stream));
    }
    int more(H *h, int32_t more_spp, const uint8_t *select, float *field_rgb, wost_stats *stats) const
    {
        int rc = carry_check_more(h, field_rgb, more_spp);
        if (rc == WOST_OK) rc = bound(h);
        if (rc != WOST_OK) return rc;
        PointListCtx<H> x(h);
        return calls.more_where(&x, more_spp, select, field_rgb, stats);
    }
    int more_dev(H *h, int32_t more_spp, const uint8_t *select_dev, float *field_rgb_dev, void *stream, wost_stats *stats) const
    {
        int rc = carry_check_more(h, field_rgb_dev, more_spp);
        if (rc == WOST_OK) rc = bound(h);
        if (rc != WOST_OK) return rc;
        PointListCtx<H> x(h);
        return calls.more_where_sharded(&x, 0, 1, more_spp, select_dev, field_rgb_dev, stream, stats);
    }
    int adaptive(H *h, const wost_adaptive *a, float *field_rgb, float *stderr_rgb, int32_t *spp_map, wost_stats *stats) const
    {
        int rc = carry_check_adaptive(h, a, field_rgb);
        if (rc == WOST_OK) rc = bound(h);
        if (rc != WOST_OK) return rc;
        PointListCtx<H> x(h);
        return calls.adaptive(&x, a, field_rgb, stderr_rgb, spp_map, stats);
    }
    int adaptive_dev(H *h, const wost_adaptive *a, float *field_rgb_dev, void *stream, wost_stats *stats) const
    {
        int rc = carry_check_adaptive(h, a, field_rgb_dev);
        if (rc == WOST_OK) rc = bound(h);
        if (rc != WOST_OK) return rc;
        PointListCtx<H> x(h);
        return calls.adaptive_sharded(&x, 0, 1, a, field_rgb_dev, stream, stats);
    }
    int carried(H *h, int32_t *spp, int32_t *batches, float *sum_rgb, float *stderr_rgb) const
    {
        if (!h) return set_error(WOST_ERR_INVALID, "null argument");
        const int rc = bound(h);
        if (rc != WOST_OK) return rc;
        PointListCtx<H> x(h);
        return calls.carried(&x, spp, batches, sum_rgb, stderr_rgb);
    }
    int restart(H *h) const
    {
        if (!h) return set_error(WOST_ERR_INVALID, "null argument");
        carry_restart(h->list.carry);
        return WOST_OK;
    }
    int progress(H *h, int32_t *n_points, int32_t *spp_done) const
    {
        if (!h || !n_points || !spp_done) return set_error(WOST_ERR_INVALID, "null argument");
        *n_points = h->list.n;
        *spp_done = h->list.carry.done;
        return WOST_OK;
    }
};

}  // namespace wost
