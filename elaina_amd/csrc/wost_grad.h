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

// the first ball stays clear of the Neumann boundary: R = min(dD, kGradNeumannShrink * dN).  Exact in binary; a design constant
constexpr float kGradNeumannShrink = 0.875f;

// The scratch of a handle's gradient calls, sized by the handle (n_pixels walks, what one point step takes), allocated on the
// first call and freed with the handle: per walk its first point and direction (dim floats each) and its result (RGB), per
// point of a block its radius; two pairs of events around the two kernels of a block.
struct GradScratch {
    void *mem = nullptr;
    float *first = nullptr, *dirs = nullptr, *w = nullptr, *radius = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};
void grad_free(GradScratch &s);

// The kernel in front of the walks, for `count` points of the caller's list from point `first` on, `spp` walks each: point j of
// the block draws its directions from the stream of pixel seed_base + first + j of a frame seed_width wide.  All pointers on
// the device; radius, dirs and first_pts are the block's (indexed from 0).
struct GradPrep {
    const float *pts;
    int32_t first, count, spp, seed_base, seed_width;
    float eps;
    float *radius, *dirs, *first_pts;
};
int grad_prep2(const DevMesh &dm, const DevMesh &nm, const GradPrep &p, hipStream_t stream);
int grad_prep3(const DevMesh3 &dm, const DevMesh3 &nm, const GradPrep &p, hipStream_t stream);

// What the driver reads of a context, and what a dimension adds: its kernel in front (grad_prep2 / grad_prep3 on its meshes) and
// its point step -- one sample at each of the n_walks device points, walk w on the stream of pixel seed_base + w, into w_rgb.
struct GradCall {
    const char *prefix;
    int dim, device;
    int32_t spp;
    size_t n_pixels;
    float eps;
    bool has_source;
    hipStream_t stream;      // the handle's own: where a host call runs
    GradScratch *scratch;
    std::function<int(const GradPrep &, hipStream_t)> prep;
    std::function<int(const float *first_pts, int32_t n_walks, int32_t seed_base, int32_t seed_width, float *w_rgb, hipStream_t stream,
                      wost_stats *stats)>
        walk;
};

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

}  // namespace wost
