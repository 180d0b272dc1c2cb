// wost_train.h -- from a guided solve's training records to its Adam steps, once for GuidedIntegrator<2> (wost_guided.hip) and
// GuidedIntegrator<3> (wost_guided3.hip): the record layout, the ordered training set (count, scan, scatter: wost_train.hip),
// the batch rule and the training passes.  Not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/wost.h"
#include "wost_internal.h"

namespace wost {

constexpr int kMaxTrainDepth = 4;     // reference parameters.h:7 (record slots per pixel)

// A training record of a D-dimensional walk: the first field of each member, kFields floats in all.  The walk kernels write
// records as rec[(slot * kFields + field) * rec_ld + column].
template <int D>
struct Rec {
    static constexpr int kSol = 0;               // solution rgb
    static constexpr int kPos = 3;               // position (D)
    static constexpr int kDir = 3 + D;           // direction (D)
    static constexpr int kPdf = 3 + 2 * D;
    static constexpr int kThp = 4 + 2 * D;       // throughput
    static constexpr int kNrm = 5 + 2 * D;       // Neumann normal (D)
    static constexpr int kOnN = 5 + 3 * D;       // on a Neumann boundary (0 / 1)
    static constexpr int kFields = 6 + 3 * D;
};

// generate_training_data (reference train.h:423-471): the valid records in (pixel, record) order
struct TrainSet {
    float *x, *dir, *sol, *li, *pdf, *nrm;      // normalised input (D), direction (D), |solution / thp| (3), its mean, pdf, normal (D)
    uint8_t *onn;
};

template <int D>
struct TrainSetParams {
    float min[D], max[D];     // scene.aabb: contains() with closed bounds (Eigen AlignedBox semantics)
    float c[D], e[D];         // centre and extent of the box inflated by 0.5 % of its diagonal (normalizeSpatialCoord, train.h:149-155)
    const float *rec;         // column 0 of the record set to gather
    size_t rec_ld;
    const uint32_t *cur_depth;
    uint32_t train_offset, train_stride;
    int32_t n_train_pixels;
    uint32_t *block_sums;     // [n_blocks + 1]: records per block of 256 training pixels; after the scan the block's first output index, then the total
    TrainSet ts;
};

struct TrainSchedule {
    int32_t batch_size, min_batch_size, batches_per_spp;
    float loss_scale;
};
template <class Settings>
TrainSchedule train_schedule(const Settings &s)
{
    return {s.batch_size, s.min_batch_size, s.batches_per_spp, s.loss_scale};
}

// shared-network mode: the collective hooks of the caller; fn == nullptr: the network is private
struct TrainSync {
    wost_sync_fn fn;
    void *user;
};

// The three launches that build the training set of T (blocks of 256 training pixels) on `st`, and the asynchronous copy of its
// size to the pinned word `host_total`.
template <int D>
int enqueue_train_set(const TrainSetParams<D> &T, int n_blocks, hipStream_t st, uint32_t *host_total);

// entries of batch `it` of a training set of n: what is left of the set, rounded down to 128; 0 = no further batch
size_t batch_len(size_t n, size_t it, const TrainSchedule &s);

// trainStep (reference integrator.cu:618-668): up to batches_per_spp Adam steps on the n entries of `ts`; adds the loss-gradient
// launches made to `launches` (the network counts its own)
template <int D>
int train_passes(wost_net_handle net, const TrainSet &ts, size_t n, const TrainSchedule &s, const TrainSync &sync, hipStream_t st,
                 uint32_t &launches);

// field = sol / spp for n pixels (rgb)
void launch_resolve(const float *sol, int n, float spp, float *field, hipStream_t st);
// ... for the n points of a point solve (`dim` coordinates each): a point with a non-finite coordinate was never walked, its entry is NaN
void launch_resolve_points(const float *sol, const float *points, int dim, int n, float spp, float *field, hipStream_t st);

// A guided solve at the caller's points instead of the frame's pixels (wost_guided_solve_points & co., include/wost.h): walker i
// is point i of `pts` (device, dim floats each) on the random stream of pixel seed_base + i of a frame seed_width wide.
// pts == nullptr: the frame solve.
struct PointJob {
    const float *pts;
    int32_t n, seed_base, seed_width;
    int32_t train_spp_count;      // -1: the handle's setting; >= 0: the first min(spp, train_spp_count) samples train
};
// the argument rules of the guided point solves: those of check_point_solve, then the training override
inline int check_guided_point_solve(const void *h, const void *pts, const void *field, int32_t n, int32_t seed_base, int32_t seed_width,
                                    int32_t train_spp_count)
{
    const int rc = check_point_solve(h, pts, field, n, seed_base, seed_width);
    if (rc != WOST_OK) return rc;
    if (train_spp_count < -1) return set_error(WOST_ERR_INVALID, "train_spp_count must be -1 (the handle's setting) or >= 0");
    return WOST_OK;
}

// `count` elements on the current device, owned by the allocation list of a handle
template <class T>
hipError_t device_alloc(std::vector<void *> &allocs, T **p, size_t count)
{
    void *v = nullptr;
    hipError_t e = hipMalloc(&v, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) {
        allocs.push_back(v);
        *p = reinterpret_cast<T *>(v);
    }
    return e;
}
// ... and one of them released before the handle goes (a buffer that is replaced by a larger one); p may be null
inline void device_release(std::vector<void *> &allocs, void *p)
{
    const auto it = std::find(allocs.begin(), allocs.end(), p);
    if (!p || it == allocs.end()) return;
    allocs.erase(it);
    (void)hipFree(p);
}

// the seven arrays of a training set of up to `capacity` entries in `dim` dimensions
hipError_t alloc_train_set(std::vector<void *> &allocs, TrainSet &ts, int dim, size_t capacity);

// the first m entries to the host (behind the *_guided_train_set entry points; arrays may be null)
int copy_train_set(const TrainSet &ts, int dim, size_t m, float *x, float *dir, float *solution, float *dir_pdf, float *normal,
                   uint8_t *on_neumann);

// the guiding state of a sample (ctor state integrator.cu:1158-1160, prepareSolve :125-126, the switch :991-996)
struct GuidePhase { bool training; float uniform_fraction; int max_guided_depth; };
template <class Settings>
GuidePhase phase_at(const Settings &s, int sample)
{
    if (sample < s.train_spp_count) return {true, s.uniform_fraction_training, s.max_guided_depth_training};
    return {false, s.uniform_fraction_guiding, s.max_guided_depth_guiding};
}

// one step of an integrator's host sampler (pcg32)
inline uint32_t host_pcg_next(uint64_t &state, uint64_t inc)
{
    const uint64_t old = state;
    state = old * WOST_PCG32_MULT + inc;
    const uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u), rot = (uint32_t)(old >> 59u);
    return (xorshifted >> rot) | (xorshifted << ((~rot + 1u) & 31));
}

}  // namespace wost
