// wost_exits.h -- the exit list of a handle (wost_exits_walk & co., include/wost.h "Exit lists"), shared by the 2-D
// and the 3-D context: per walk the record of where it left the domain -- the absorbing primitive, its projection ratio and
// side, the throughput and what the source and Neumann samples had added -- so that the solution for any Dirichlet data is one
// multiply-add per walk (apply) and its derivative with respect to that data a scatter over the same records (adjoint).  A
// dimension adds the kernel that walks (appended to wost_hip.hip / wost_hip3d.hip, on their unchanged step functions); the
// list, the two kernels behind it and the bodies of the entry points are here and in wost_exits.hip.  The list of the gradient
// (wost_exits_walk_gradient & co., "Exit lists of the gradient") is the same list walked from the first points of
// the gradient's estimator (wost_grad.h) and kept with their directions and radii: grad u for any Dirichlet data and the
// transpose of that map are two more kernels over the same records.  The index of a list by vertex (wost_exits_index & co., "Exit
// lists: the index and the ordered adjoint"; built in wost_exits_index.hip) turns both transposes into gathers
// with a fixed summation order.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <functional>

#include "../../include/wost.h"
#include "wost_grad.h"
#include "wost_internal.h"

namespace wost {

// The records on the device, one array per field (a wave's lanes write neighbouring walks: coalesced), walk (i, s) at i * S + s:
// 6 + DIM arrays of `stride` four-byte entries in one allocation -- prim, slot, side, thp, DIM - 1 of uv, three of base.  slot is
// the primitive's place in the tree's leaf order, where the mesh tables list its vertices; prim its index in the caller's array.
// (One pointer and the stride, not an address per array: the walk kernels hold what they are given in scalar registers to
// their end, and they are short of those.)
struct ExitRecords {
    int32_t *mem = nullptr;
    size_t stride = 0;
    __host__ __device__ int32_t *prim() const { return mem; }
    __host__ __device__ int32_t *slot() const { return mem + stride; }
    __host__ __device__ int32_t *side() const { return mem + 2 * stride; }
    __host__ __device__ float *thp() const { return reinterpret_cast<float *>(mem + 3 * stride); }
    __host__ __device__ float *uv(int k) const { return reinterpret_cast<float *>(mem + (4 + (size_t)k) * stride); }
    __host__ __device__ float *base(int dim, int c) const { return reinterpret_cast<float *>(mem + (3 + (size_t)dim + (size_t)c) * stride); }
};

// What a handle carries beside the carried frame solve, the carried point list and the gradient list: one allocation.  A list
// of the gradient (wost_exits_walk_gradient) has three more arrays in it, behind the records: per point the radius
// of its first ball, per walk its direction and its first point, dim floats each, interleaved per walk as GradPrep writes them
// -- 4 * (6 + 3 dim) bytes per walk and 4 per point in all.  A plain list has none of them (dirs == nullptr).
// A list of the gradient walked on a scene with a source term (the option "exits_grad_source"; DESIGN 4.3i "The in-ball term")
// has one more array behind those, 8-byte aligned: per point the in-ball term of the gradient's estimator, which does not depend
// on the Dirichlet data -- 6 dim + 3 doubles, T (dim * 3), seT (dim * 3) and U (3), 8 * (6 dim + 3) bytes per point.  Every
// other list has none (terms == nullptr): the mode is the list's, fixed at the walk.
// The index of a list by vertex (wost_exits_index), one allocation of its own: incidence w * DIM + j is corner j of
// the primitive of absorbed walk w, its bin 2 v + (side < 0) with v the corner's vertex in the caller's numbering; a bin holds
// its incidences ascending.  nbar (a list of the gradient only): per point and axis the mean direction as
// exits_adjoint_gradient_kernel forms it.  mem == nullptr: no index stands.
struct ExitIndex {
    void *mem = nullptr;
    int64_t *bin_begin = nullptr;      // 2 n_verts + 1
    double *nbar = nullptr;            // n * DIM, or nullptr
    int32_t *inc = nullptr;            // n_inc
    int64_t n_inc = 0, longest_bin = 0;
};
struct ExitList {
    void *mem = nullptr;
    ExitRecords rec;
    int dim = 0;
    int32_t n = 0, S = 0;
    float *radius = nullptr, *dirs = nullptr, *first = nullptr;
    double *terms = nullptr;
    ExitIndex index;                   // lives and dies with the list: whatever replaces or releases the list drops it
};
void exits_free(ExitList &l);
void exits_index_free(ExitIndex &x);

// One launch of a dimension's walk kernel: the `count` walks from walk `first_walk` of the list on, one lane each.  Walk w
// belongs to point w / S of pts and runs on the stream of pixel walk_seed_base + w of a frame seed_width wide.  counters: five
// 64-bit sums on the device (steps, started, absorbed, truncated, Neumann hits), added to.
struct ExitWalk {
    const float *pts;
    int32_t first_walk, count, S, walk_seed_base, seed_width;
    ExitRecords rec;
    unsigned long long *counters;
};
// the close of a walk kernel (all lanes of the wave call): the lanes' five counts summed over the wave, one add per non-zero sum
__device__ __forceinline__ void wave_add_counters(unsigned long long *counters, uint32_t steps, uint32_t started, uint32_t absorbed, uint32_t truncated,
                                                  uint32_t nhits)
{
    const uint32_t v[5] = {steps, started, absorbed, truncated, nhits};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        uint32_t x = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
        if ((threadIdx.x & 63) == 0 && x) atomicAdd(counters + k, (unsigned long long)x);
    }
}

// What the driver reads of a context, and what a dimension adds: its walk kernel with the template flags of its point solve.
// verts: the mesh table of the vertex ids of the primitive in a slot (DIM per slot), n_verts the Dirichlet mesh's vertices
// (0: the scene has no Dirichlet mesh).
struct ExitCall {
    const char *prefix;
    int dim, device;
    size_t n_pixels;
    hipStream_t stream;      // the handle's own: where a host call runs
    ExitList *list;
    const int32_t *verts;
    int32_t n_verts;
    float dirichlet_intensity;
    std::function<int(const ExitWalk &, hipStream_t)> walk;
    // ... and for a list of the gradient: the kernel in front (grad_prep2 / grad_prep3 on the context's meshes), the shell,
    // whether the scene has a source term, the handle's option "exits_grad_source" (without it such a scene is refused, with it
    // the list carries the in-ball term) and the in-ball kernel on the context's source grid (grad_ball2 / grad_ball3)
    std::function<int(const GradPrep &, hipStream_t)> prep;
    float eps = 0.0f;
    bool has_source = false, source_term = false;
    std::function<int(const GradBall &, hipStream_t)> ball;
    bool in_ball() const { return has_source && source_term; }
};

// the argument rules that need no look at the handle (include/wost.h), in the order of the header
int exits_check_walk(const void *h, const float *pts, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width);
int exits_check_apply(const void *h, const void *in, int32_t K, const void *out, const char *in_name, const char *out_name);
// the walk after them (n > 0): the new list, which replaces the old one when it stands whole
int exits_walk(const ExitCall &c, const float *pts, bool pts_on_host, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width,
               hipStream_t stream, wost_stats *stats);
int exits_records(const ExitCall &c, const wost_exit_records &out);
int exits_apply(const ExitCall &c, const float *colors, int32_t K, float *field, float *stderr_rgb, bool on_host, hipStream_t stream);
int exits_adjoint(const ExitCall &c, const float *dfield, int32_t K, float *dcolors, bool on_host, hipStream_t stream);

// ---- the list of the gradient (include/wost.h "Exit lists of the gradient") ----
// the seeds of a walk of the gradient: where the directions are drawn, where the walks run
struct ExitSeeds {
    int32_t seed_base, walk_seed_base, seed_width;
};
// the argument rules that need no look at the handle, in the order of the header
int exits_check_walk_gradient(const void *h, const float *pts, int32_t n, int32_t walks, const ExitSeeds &seeds);
// the walk after them (n > 0): the rule that needs the handle, then the kernel in front straight into the new list and the walks
// from its first points, one each
int exits_walk_gradient(const ExitCall &c, const float *pts, bool pts_on_host, int32_t n, int32_t walks, const ExitSeeds &seeds, hipStream_t stream,
                        wost_stats *stats);
int exits_gradient_records(const ExitCall &c, const wost_exit_gradient_records &out);
// grad is required, se and field may be nullptr
int exits_apply_gradient(const ExitCall &c, const float *colors, int32_t K, float *grad, float *se, float *field, bool on_host, hipStream_t stream);
int exits_adjoint_gradient(const ExitCall &c, const float *dgrad, int32_t K, float *dcolors, bool on_host, hipStream_t stream);
// the option "exits_grad_source" of a handle (wost_set_option, wost3_set_option): exactly 0 or 1
int exits_grad_source_option(double value, bool *option);
// the in-ball term the bound list carries into host arrays of n * dim * 3, n * dim * 3 and n * 3 doubles; any may be nullptr
int exits_gradient_terms(const ExitCall &c, double *T, double *seT, double *U);

// ---- the index and the ordered adjoints (include/wost.h "Exit lists: the index and the ordered adjoint") ----
// a device allocation that may fail for want of memory: WOST_ERR_NOMEM then, WOST_ERR_DEVICE for anything else
int exits_alloc(void **p, size_t bytes, const char *what);
// the index of the bound list, built on the default stream (wost_exits_index.hip); the list's old index, if any, stays on failure
int exits_index_build(const ExitCall &c);
int exits_index_records(const ExitCall &c, int64_t *bin_begin, int32_t *inc);
// the gathers over the index: the arguments and layouts of exits_adjoint and exits_adjoint_gradient
int exits_adjoint_ordered(const ExitCall &c, const float *dfield, int32_t K, float *dcolors, bool on_host, hipStream_t stream);
int exits_adjoint_gradient_ordered(const ExitCall &c, const float *dgrad, int32_t K, float *dcolors, bool on_host, hipStream_t stream);

// the bodies of the entry points, written once: H is the context (device, stream, exits), `call` what a dimension adds
template <class H>
struct ExitCalls {
    ExitCall (*call)(H *);
    int dim;

    static int bound(const H *h)
    {
        if (h->exits.n <= 0) return set_error(WOST_ERR_INVALID, "no exit list is bound to the handle (exits_walk binds one)");
        return WOST_OK;
    }
    // host points travel on the handle's stream, device points on the caller's
    int walk(H *h, const float *pts, bool pts_on_host, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width, void *stream,
             wost_stats *stats) const
    {
        int rc = exits_check_walk(h, pts, n, walks, walk_seed_base, seed_width);
        if (rc == WOST_OK && pts_on_host) rc = check_points_finite(pts, n, dim);
        if (rc != WOST_OK) return rc;
        if (stats) std::memset(stats, 0, sizeof(*stats));
        if (n == 0) {
            if (h->exits.mem) {
                WOST_TRY(hipSetDevice(h->device));
                exits_free(h->exits);
            }
            return WOST_OK;
        }
        return exits_walk(call(h), pts, pts_on_host, n, walks, walk_seed_base, seed_width,
                          pts_on_host ? h->stream : reinterpret_cast<hipStream_t>(stream), stats);
    }
    int records(H *h, const wost_exit_records *out) const
    {
        if (!h || !out) return set_error(WOST_ERR_INVALID, "null argument");
        const int rc = bound(h);
        if (rc != WOST_OK) return rc;
        return exits_records(call(h), *out);
    }
    int apply(H *h, const float *colors, int32_t K, float *field, float *stderr_rgb, bool on_host, void *stream) const
    {
        int rc = exits_check_apply(h, colors, K, field, "colors", "field_rgb");
        if (rc == WOST_OK) rc = bound(h);
        if (rc != WOST_OK) return rc;
        return exits_apply(call(h), colors, K, field, stderr_rgb, on_host, on_host ? h->stream : reinterpret_cast<hipStream_t>(stream));
    }
    int adjoint(H *h, const float *dfield, int32_t K, float *dcolors, bool on_host, void *stream) const
    {
        int rc = exits_check_apply(h, dfield, K, dcolors, "dfield", "dcolors");
        if (rc == WOST_OK) rc = bound(h);
        if (rc != WOST_OK) return rc;
        return exits_adjoint(call(h), dfield, K, dcolors, on_host, on_host ? h->stream : reinterpret_cast<hipStream_t>(stream));
    }
    // ---- the list of the gradient ----
    static int bound_gradient(const H *h)
    {
        const int rc = bound(h);
        if (rc != WOST_OK) return rc;
        if (!h->exits.dirs)
            return set_error(WOST_ERR_INVALID, "the exit list bound to the handle has no directions (wost_exits_walk_gradient binds one that has)");
        return WOST_OK;
    }
    int walk_gradient(H *h, const float *pts, bool pts_on_host, int32_t n, int32_t walks, const ExitSeeds &seeds, void *stream, wost_stats *stats) const
    {
        int rc = exits_check_walk_gradient(h, pts, n, walks, seeds);
        if (rc == WOST_OK && pts_on_host) rc = check_points_finite(pts, n, dim);
        if (rc != WOST_OK) return rc;
        if (stats) std::memset(stats, 0, sizeof(*stats));
        if (n == 0) {
            if (h->exits.mem) {
                WOST_TRY(hipSetDevice(h->device));
                exits_free(h->exits);
            }
            return WOST_OK;
        }
        return exits_walk_gradient(call(h), pts, pts_on_host, n, walks, seeds, pts_on_host ? h->stream : reinterpret_cast<hipStream_t>(stream), stats);
    }
    int gradient_records(H *h, const wost_exit_gradient_records *out) const
    {
        if (!h || !out) return set_error(WOST_ERR_INVALID, "null argument");
        const int rc = bound_gradient(h);
        if (rc != WOST_OK) return rc;
        return exits_gradient_records(call(h), *out);
    }
    int apply_gradient(H *h, const float *colors, int32_t K, float *grad, float *se, float *field, bool on_host, void *stream) const
    {
        int rc = exits_check_apply(h, colors, K, grad, "colors", "grad");
        if (rc == WOST_OK) rc = bound_gradient(h);
        if (rc != WOST_OK) return rc;
        return exits_apply_gradient(call(h), colors, K, grad, se, field, on_host, on_host ? h->stream : reinterpret_cast<hipStream_t>(stream));
    }
    int gradient_terms(H *h, double *T, double *seT, double *U) const
    {
        if (!h) return set_error(WOST_ERR_INVALID, "null argument");
        const int rc = bound_gradient(h);
        if (rc != WOST_OK) return rc;
        if (!h->exits.terms)
            return set_error(WOST_ERR_INVALID, "the exit list bound to the handle carries no in-ball term (a walk of the gradient on a scene with a source "
                                               "term under the option exits_grad_source binds one that does)");
        if (!T && !seT && !U) return WOST_OK;
        return exits_gradient_terms(call(h), T, seT, U);
    }
    int adjoint_gradient(H *h, const float *dgrad, int32_t K, float *dcolors, bool on_host, void *stream) const
    {
        int rc = exits_check_apply(h, dgrad, K, dcolors, "dgrad", "dcolors");
        if (rc == WOST_OK) rc = bound_gradient(h);
        if (rc != WOST_OK) return rc;
        return exits_adjoint_gradient(call(h), dgrad, K, dcolors, on_host, on_host ? h->stream : reinterpret_cast<hipStream_t>(stream));
    }
    // ---- the index and the ordered adjoints ----
    static int indexed(const H *h)
    {
        if (!h->exits.index.mem)
            return set_error(WOST_ERR_INVALID, "the exit list bound to the handle has no index (wost_exits_index builds one)");
        return WOST_OK;
    }
    int index(H *h) const
    {
        if (!h) return set_error(WOST_ERR_INVALID, "null argument");
        const int rc = bound(h);
        if (rc != WOST_OK) return rc;
        const ExitCall c = call(h);
        if (c.n_verts <= 0)
            return set_error(WOST_ERR_UNSUPPORTED, std::string(c.prefix) + "exits_index: the scene has no Dirichlet mesh, so no walk exits at a vertex");
        if (h->exits.index.mem) return WOST_OK;
        return exits_index_build(c);
    }
    int index_info(H *h, int64_t *n_incidences, int64_t *longest_bin) const
    {
        if (!h || !n_incidences || !longest_bin) return set_error(WOST_ERR_INVALID, "null argument");
        *n_incidences = h->exits.index.mem ? h->exits.index.n_inc : 0;
        *longest_bin = h->exits.index.mem ? h->exits.index.longest_bin : 0;
        return WOST_OK;
    }
    int index_records(H *h, int64_t *bin_begin, int32_t *inc) const
    {
        if (!h) return set_error(WOST_ERR_INVALID, "null argument");
        int rc = bound(h);
        if (rc == WOST_OK) rc = indexed(h);
        if (rc != WOST_OK) return rc;
        return exits_index_records(call(h), bin_begin, inc);
    }
    int adjoint_ordered(H *h, const float *dfield, int32_t K, float *dcolors, bool on_host, void *stream) const
    {
        int rc = exits_check_apply(h, dfield, K, dcolors, "dfield", "dcolors");
        if (rc == WOST_OK) rc = bound(h);
        if (rc == WOST_OK) rc = indexed(h);
        if (rc != WOST_OK) return rc;
        return exits_adjoint_ordered(call(h), dfield, K, dcolors, on_host, on_host ? h->stream : reinterpret_cast<hipStream_t>(stream));
    }
    int adjoint_gradient_ordered(H *h, const float *dgrad, int32_t K, float *dcolors, bool on_host, void *stream) const
    {
        int rc = exits_check_apply(h, dgrad, K, dcolors, "dgrad", "dcolors");
        if (rc == WOST_OK) rc = bound(h);
        if (rc == WOST_OK) rc = indexed(h);
        if (rc == WOST_OK) rc = bound_gradient(h);
        if (rc != WOST_OK) return rc;
        return exits_adjoint_gradient_ordered(call(h), dgrad, K, dcolors, on_host, on_host ? h->stream : reinterpret_cast<hipStream_t>(stream));
    }
    int progress(H *h, int32_t *n_points, int32_t *walks) const
    {
        if (!h || !n_points || !walks) return set_error(WOST_ERR_INVALID, "null argument");
        *n_points = h->exits.n;
        *walks = h->exits.S;
        return WOST_OK;
    }
};

}  // namespace wost
