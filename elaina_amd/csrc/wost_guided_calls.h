// wost_guided_calls.h -- the front of the guided solve that callers touch, once for wost_guided_* (wost_guided.hip) and
// wost3_guided_* (wost_guided3.hip): the bodies of the entry points, the counters of a solve, the end of a solve, the phase of a
// sample and the choice of a walk kernel by the scene's flags.  Host code only; the training itself is wost_train.h's.  Not part of
// the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/wost.h"
#include "wost_train.h"

namespace wost {

// Counters of a solve.  Atomics on ONE cache line are served one after the other by its L2 channel
// (measured: about 120 M/s, 270 us for the 16 384 waves of one launch), so the counters exist in
// kGuidedStatCopies copies 256 bytes apart, a wave adds to the copy of its block, and the host sums them.
constexpr int kGuidedStatCopies = 64;
struct alignas(256) GuidedStatsDev {
    unsigned long long steps, started, absorbed, truncated, nhits, guided, net_points;
};

// the guiding state of sample `sample` of a solve whose first train_spp_count samples train (a point solve may override the settings')
template <class Settings>
GuidePhase phase_of(Settings s, int train_spp_count, int sample)
{
    s.train_spp_count = train_spp_count;
    return phase_at(s, sample);
}

// The scene's flags as the template arguments E(missive), T(ree), S(ource) of the walk kernels: f.of<E, T, S>()
template <class F>
auto by_scene_flags(bool e, bool t, bool s, const F &f) -> decltype(f.template of<false, false, false>())
{
    if (e && t) return s ? f.template of<true, true, true>() : f.template of<true, true, false>();
    if (e) return s ? f.template of<true, false, true>() : f.template of<true, false, false>();
    if (t) return s ? f.template of<false, true, true>() : f.template of<false, true, false>();
    return s ? f.template of<false, false, true>() : f.template of<false, false, false>();
}

// what the steps of a solve count and hand to each other, as far as both dimensions have it
struct GuidedRunBase {
    std::chrono::high_resolution_clock::time_point t_start;
    uint64_t net_launches_before; int opt_before;      // the network's counters when the solve began
    uint32_t launches = 0;                  // of the dimension's file; the network counts its own
    double train_ms = 0.0;
    uint64_t train_samples = 0;
};

// The end of a solve: resolve (not counted), the copies of the field, the counters folded and the stats.  H has s, n_pixels, net,
// sol, field and stats.  train_offset: the solve's trainPixelOffset, reported in `reserved`; net_infer_ms: the device time of the
// network-evaluating launches where the dimension measures it, read once the stream has drained.
template <class H>
int finish_guided_solve(H *g, const GuidedRunBase &run, int dim, const PointJob &job, uint32_t train_offset, hipStream_t stream, float *field_host,
                        float *field_dev, wost_guided_stats *stats, double (*net_infer_ms)(H *) = nullptr)
{
    const int N = job.pts ? job.n : (int)g->n_pixels;
    if (job.pts) launch_resolve_points(g->sol, job.pts, dim, N, (float)g->s.spp, g->field, stream);
    else launch_resolve(g->sol, N, (float)g->s.spp, g->field, stream);
    WOST_TRY(hipGetLastError());
    if (field_host) WOST_TRY(hipMemcpyAsync(field_host, g->field, (size_t)N * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (field_dev) WOST_TRY(hipMemcpyAsync(field_dev, g->field, (size_t)N * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
    std::vector<GuidedStatsDev> copies(kGuidedStatCopies);
    WOST_TRY(hipMemcpyAsync(copies.data(), g->stats, kGuidedStatCopies * sizeof(GuidedStatsDev), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipStreamSynchronize(stream));
    wost_guided_stats out{};
    for (const GuidedStatsDev &c : copies) {
        out.walk_steps += c.steps; out.walks_started += c.started; out.walks_absorbed += c.absorbed; out.walks_truncated += c.truncated;
        out.neumann_hits += c.nhits; out.guided_steps += c.guided; out.net_points += c.net_points;
    }
    out.train_samples = run.train_samples; out.train_ms = run.train_ms;
    if (net_infer_ms) out.net_infer_ms = net_infer_ms(g);
    out.optimizer_steps = (uint64_t)(net_optimizer_steps(g->net) - run.opt_before); out.reserved = train_offset;
    out.kernel_launches = run.launches + (uint32_t)(net_launch_count(g->net) - run.net_launches_before);
    out.solve_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - run.t_start).count();
    if (stats) *stats = out;
    return WOST_OK;
}

// centre and extent of the box that normalises the network's input (the scene's box inflated by 0.5 % of its diagonal)
struct GuidedBox { float c[3], e[3]; };

// ---- the entry points of the guided solve, written once for the 2-D and the 3-D handle ----
// H has device, n_pixels (the frame's: the capacity of a point solve), stream, scene, net, allocs, pts_buf, pts_cap, ts and
// last_train_n.  What a dimension adds: its solve driver, the columns of a point and its box.
template <class H>
struct GuidedCalls {
    // field_host (n * 3 floats for the n walkers of the solve, may be null) and / or field_dev (device); job: the caller's points instead of the frame
    int (*run)(H *g, int shard_index, int shard_count, float *field_host, float *field_dev, wost_guided_stats *stats, const PointJob &job);
    int dim;
    GuidedBox (*box)(const H *g);

    int network(H *h, wost_net_handle *net) const
    {
        if (!h || !net) return set_error(WOST_ERR_INVALID, "null argument");
        *net = h->net;
        return WOST_OK;
    }
    template <class Scene>
    int scene(H *h, Scene *scene) const
    {
        if (!h || !scene) return set_error(WOST_ERR_INVALID, "null argument");
        *scene = h->scene;
        return WOST_OK;
    }
    int solve(H *h, float *field_rgb, wost_guided_stats *stats) const
    {
        if (!h || !field_rgb) return set_error(WOST_ERR_INVALID, "null argument");
        return run(h, 0, 1, field_rgb, nullptr, stats, PointJob{});
    }
    int solve_sharded(H *h, int32_t shard_index, int32_t shard_count, float *field_rgb_dev, wost_guided_stats *stats) const
    {
        if (!h || !field_rgb_dev) return set_error(WOST_ERR_INVALID, "null argument");
        if (shard_count < 1 || shard_index < 0 || shard_index >= shard_count) return set_error(WOST_ERR_INVALID, "bad shard");
        return run(h, shard_index, shard_count, nullptr, field_rgb_dev, stats, PointJob{});
    }

    // The point solves: host points travel to a buffer of the handle, grown on demand, on the handle's stream; device points are
    // read where they lie.  The argument rules that need no look at the handle come first, then the empty list, then the check that
    // needs the handle: the per-pixel state, the record sets and the queues are sized by the frame.
    int solve_points(H *h, const float *pts, bool pts_on_host, int32_t n, int32_t seed_base, int32_t seed_width, int32_t train_spp_count,
                     float *field_rgb, wost_guided_stats *stats) const
    {
        int rc = check_guided_point_solve(h, pts, field_rgb, n, seed_base, seed_width, train_spp_count);
        if (rc == WOST_OK && pts_on_host) rc = check_points_finite(pts, n, dim);
        if (rc != WOST_OK) return rc;
        if (n == 0) {
            if (stats) *stats = wost_guided_stats{};
            return WOST_OK;
        }
        if ((size_t)n > h->n_pixels)
            return set_error(WOST_ERR_INVALID, "a guided point solve takes at most width * height = " + std::to_string(h->n_pixels) + " points per call (the handle's capacity); got " + std::to_string(n));
        if (!pts_on_host) return run(h, 0, 1, nullptr, field_rgb, stats, PointJob{pts, n, seed_base, seed_width, train_spp_count});
        WOST_TRY(hipSetDevice(h->device));
        if (h->pts_cap < (size_t)n) {
            // (nothing on the device reads the list between two solves)
            device_release(h->allocs, h->pts_buf);
            h->pts_buf = nullptr; h->pts_cap = 0;
            WOST_TRY(device_alloc(h->allocs, &h->pts_buf, (size_t)n * dim));
            h->pts_cap = (size_t)n;
        }
        WOST_TRY(hipMemcpyAsync(h->pts_buf, pts, (size_t)n * dim * sizeof(float), hipMemcpyHostToDevice, h->stream));
        return run(h, 0, 1, field_rgb, nullptr, stats, PointJob{h->pts_buf, n, seed_base, seed_width, train_spp_count});
    }

    // queryNetwork (reference exec.cu:175-186, guided/integrator.cu:566-615): the raw mixture parameters of the inference weights
    // at world positions
    int query_network(H *h, const float *pts, int32_t n, float *raw) const
    {
        if (!h || !pts || !raw || n < 0) return set_error(WOST_ERR_INVALID, "bad argument");
        const GuidedBox b = box(h);
        std::vector<float> in((size_t)n * dim);
        for (int i = 0; i < n; ++i)
            for (int a = 0; a < dim; ++a) in[(size_t)dim * i + a] = 0.5f + (pts[(size_t)dim * i + a] - b.c[a]) / b.e[a];
        return wost_net_inference(h->net, in.data(), n, raw, 1);
    }
    // the training set of the most recent training pass, (pixel, record) order; arrays may be null; *n = its size
    int train_set(H *h, int32_t capacity, int32_t *n, float *x, float *dir, float *solution, float *dir_pdf, float *normal, uint8_t *on_neumann) const
    {
        if (!h || !n || capacity < 0) return set_error(WOST_ERR_INVALID, "bad argument");
        WOST_TRY(hipSetDevice(h->device));
        *n = (int32_t)h->last_train_n;
        return copy_train_set(h->ts, dim, std::min<size_t>(h->last_train_n, (size_t)capacity), x, dir, solution, dir_pdf, normal, on_neumann);
    }
};

}  // namespace wost
