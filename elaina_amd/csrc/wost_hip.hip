// wost_hip.hip -- walk kernels and the C-ABI of libwost_hip.so (gfx950 / MI355X only).
//
// Holds: the 2-D walk, init and query kernels; the solve driver (run_solve) with its launch steps; what the 2-D context adds to
// the shared bodies of the entry points (wost_uniform.h, wost_carry.h, wost_grad.h) and the entry points themselves, which
// forward to those bodies; wost_set_option.  The context is in wost_internal2.h, the mesh upload in wost_build2.hip.
//
// Design (DESIGN.md has the long form):
//   * one SoA walk-state queue; a queue slot is one PIXEL's walker, which carries its
//     PCG32 state, position, partial solution and the temporal hint of the last closest
//     segment.  A pixel's samples are strictly sequential in the reference (one RNG stream
//     per pixel, integrator/uniform/integrator.cu:71-77, one walk in flight per pixel), so a
//     slot restarts its next sample the moment the previous walk ends instead of idling
//     until every other walk of that sample is done -- same per-pixel arithmetic, no
//     starved late-depth launches.
//   * a launch ("round") advances every slot by up to `steps_per_round` walk steps held in
//     registers, then compacts the still-unfinished slots into the other queue with
//     ballot/popcount + one atomic per wave, and resolves finished pixels into the field.
//   * the per-lane LBVH traversal stack lives in LDS (one column per lane, bank = lane).
//   * with few samples per pixel the REFILL instantiation drains the queue in ONE launch; with many, and more walkers
//     than resident lanes, the first launch is PERSISTENT: lanes take whole pixels, longest expected chain first
//     (wost_order.h), until none is unread, and hand what they hold to a few rounds -- the remainders expected to be
//     long run to their end beside those rounds, four lanes to a walker (run_solve);
//     problems with a source term use the SOURCE instantiations (wost_walk.h).
//   * no managed memory, no CPU fallback.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/wost.h"
#include "lbvh.h"
#include "wost_build2.h"
#include "wost_order.h"
#include "wost_device.h"
#include "wost_internal.h"
#include "wost_internal2.h"
#include "wost_walk.h"
#include "wost_quad.h"
#include "wost_coop.h"

namespace wost {

// Atomics on one cache line are served one by one by its L2 channel (about 10 ns each: the eight
// counters of the 16 384 waves of a round cost over a millisecond), so the counters exist in
// kStatCopies copies 256 bytes apart, a block adds to the copy blockIdx % kStatCopies and the host
// sums the copies.
constexpr int kStatCopies = 64;
struct alignas(256) StatsDev {
    unsigned long long steps, started, absorbed, truncated, nhits, inner_visits, leaf_visits, trav_trips, step_trips, max_stack;
    unsigned long long sp_ge6, sp_ge10, sp_ge14;     // WOST_TRACK developer builds: visits that left at least that many stack entries
    // WOST_DRAIN developer builds, the persistent launch: wall_clock64() at the moment a wave stops on the dry queue (earliest,
    // latest, sum and number of waves; the earliest as the maximum of the complement: the counters start at zero) and the latest
    // moment a wave reached the end of the kernel
    unsigned long long stop_min, stop_max, stop_sum, stop_waves, end_max;
};
__device__ __forceinline__ StatsDev *my_stats(StatsDev *s) { return s + (blockIdx.x & (kStatCopies - 1)); }

struct RoundParams {
    DevMesh dm, nm;
    DevSettings st;
    DevProbe probe;
    DevSource src;
    WalkQueue in, out;
    const uint32_t *count_in;
    uint32_t *count_out;
    float *field;        // solution/spp written at field[(pix - field_base) * 3]
    int32_t field_base;
    StatsDev *stats;
    int32_t steps_per_round;
    int32_t stack_stride;  // = blockDim.x
    int32_t wait_weight;   // step phase runs when n_wait * wait_weight >= 8 * n_trav
    int32_t trav_burst;    // node visits per scheduling decision in the traversal phase
    int32_t lane_shift;    // one walker per 2^lane_shift lanes (0 = every lane)
    uint32_t *cursor;      // REFILL launches: next unread slot of the input queue
    const uint32_t *order; // the k-th walker of the launch is input slot order[k] (wost_order.h); nullptr = slot k
    int32_t reserve;       // REFILL launches: input slots a wave reserves per atomic on the cursor; 0 = exactly those it needs
    int32_t leave_dry;     // REFILL launches: 1 = a wave that finds the input queue dry finishes the steps in flight and hands its
                           //   walkers to the output queue (the host repacks them: rounds); 0 = it stays until its last pixel is done;
                           //   2 (PERSIST) = as 1, and a wave also looks at the cursor every few step trips: once the queue is dry
                           //   every wave stops at its next look, not only one that needs a refill
    int32_t dry_cadence;   //   ... walk steps of a wave's busiest lane between two looks once the queue is nearly dry (a power of
    int32_t dry_shift;     //   two), and while R slots are unread: max(dry_cadence, R >> dry_shift) steps (launch_ordinary)
    uint32_t *count_long;  // ... and counts the pixels it hands over that are expected to need long_steps walk steps or more
    float long_steps;
    // walk_quad_kernel, the launch of the long remainders: the first thin_count walkers sit four to a wave (sixteen to a workgroup)
    // in the first thin_blocks workgroups, the others sixteen to a wave behind them; thin_blocks == 0: lane_shift for all
    uint32_t thin_blocks, thin_count;
    // walkers that the plain kernel cannot serve exactly (a closest-point query that starts beyond dm.far2) leave the launch
    // at that point and are queued from the TOP of the output queue downwards: slot out_capacity - 1 - k, k from *count_far
    uint32_t *count_far;
    uint32_t out_capacity;
    // NEUMANN_TREE launches of walk_round_kernel: the Neumann-side tree queries of a step by the wave as a whole (wost_coop.h):
    // pool_cap tasks per pool and wave, pool_offset words into the block's LDS (behind the stack columns); 0 = per lane
    int32_t coop, pool_cap, pool_offset, ray_slot_trigger;
    // the carried launches (walk_round_carry_kernel, walk_quad_carry_kernel) of a continued solve (wost_solve_more): a pixel that is
    // resolved leaves its generator state and its three raw sums under its pixel id, and its field entry is sum / carry_total --
    // the samples of the earlier calls and of this one; st.spp is this call's count.  (At the end: no other entry reads them.)
    uint64_t *carry_rng;
    float *carry_sum;
    int32_t carry_total;
    // the chained start (wost_set_option "chain_start"): a lane whose walk is absorbed takes the depth-0 step of its pixel's
    // next sample in the same step trip (step_finish); 0 = that step waits for the wave's next step trip
    int32_t chain;
    // the root visit at query start (wost_set_option "root_visit"): a lane that begins a closest-point query visits the tree's
    // root in the same step trip, its rows fetched on the scalar path (trav_visit_root); 0 = in its first traversal burst
    int32_t root_visit;
};

struct InitParams {
    DevMesh dm;
    DevSettings st;
    DevProbe probe;
    WalkQueue out;
    uint32_t *count_out;
    const uint8_t *mask;
    float *field;
    int32_t field_base;
    int32_t pixel_begin, pixel_end;
    int32_t shard_index, shard_count;
    int32_t tiles_x, tiles_y;
    int32_t stack_stride;
    // a call of a continued solve (wost_solve_more & co., carry_n != nullptr): a walker of a pixel with carry_n[pid] > 0 samples
    // behind it starts from the pixel's carried generator state and raw sums instead of the seed and zero; st.spp is this call's
    // count and the walker counts its samples from 0.  select (nullptr: every pixel): a pixel whose byte is 0 is not queued.
    const uint64_t *carry_rng;
    const float *carry_sum;
    const uint32_t *carry_n;
    const uint8_t *select;
};

#define META_SAMPLE(m) ((m) & 0xfffffu)
#define META_DEPTH(m) (((m) >> 20) & 0x3ffu)
#define META_ONN(m) (((m) >> 30) & 1u)
#define META_PACK(s, d, n) ((uint32_t)(s) | ((uint32_t)(d) << 20) | ((uint32_t)(n) << 30))

// ------------------------------------------------------------------------------------------
// init: seed every owned pixel, cache its depth-0 closest point, compact into the queue
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void init_kernel(InitParams P)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t *stack = lds_stack + threadIdx.x;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int tile = t >> 6, i = t & 63;
    const int tx = tile % P.tiles_x, ty = tile / P.tiles_x;
    const int x = tx * 8 + (i & 7), y = ty * 8 + (i >> 3);
    bool owned = (ty < P.tiles_y) && (x < P.st.width) && (y < P.st.height);
    int pid = y * P.st.width + x;
    owned = owned && pid >= P.pixel_begin && pid < P.pixel_end && (tile % P.shard_count) == P.shard_index;
    bool active = owned && (P.mask == nullptr || P.mask[pid] != 0) && P.st.spp > 0;
    active = active && (P.select == nullptr || P.select[pid] != 0);
    if (owned && !active) {
        // masked pixel: solution stays 0 (reference integrator.cu:92-95, :616-620); a pixel that a continued call leaves out
        // gets its entry from the kernel that closes the call (wost_carry.hip)
        float *f = P.field + 3 * (size_t)(pid - P.field_base);
        float z = 0.0f / (float)P.st.spp;
        f[0] = z; f[1] = z; f[2] = z;
    }
    float x0 = 0, y0 = 0;
    Pcg rng{0, 1};
    Closest c0{WOST_INF, -1};
    if (active) {
        eval_point(P.probe, x, y, P.st.width, P.st.height, x0, y0);
        pcg_seed_pixel(rng, pid, P.st.width);
        if (P.dm.n_segs > 0) c0 = closest_point(P.dm, x0, y0, slot_candidate(P.dm, 0, x0, y0), stack, P.stack_stride);
    }
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    if (active && P.carry_n != nullptr && P.carry_n[pid] > 0u) {
        rng.state = P.carry_rng[pid];
        const float *cs = P.carry_sum + 3 * (size_t)pid;
        sr = cs[0]; sg = cs[1]; sb = cs[2];
    }
    const uint32_t s = block_push(active, P.count_out);
    if (active) {
        WalkQueue &q = P.out;
        q.pix[s] = pid;
        q.x0[s] = x0; q.y0[s] = y0;
        q.px[s] = x0; q.py[s] = y0;
        q.rng[s] = rng.state;
        q.meta[s] = META_PACK(0, 0, 0);
        q.nx[s] = 0.0f; q.ny[s] = 0.0f;
        q.hint[s] = c0.slot;
        q.thp[s] = 1.0f;
        q.sr[s] = sr; q.sg[s] = sg; q.sb[s] = sb;
        q.d0_d2[s] = c0.d2;
        q.d0_slot[s] = c0.slot;
    }
}

// ------------------------------------------------------------------------------------------
// init of a point solve (wost_solve_points): the caller's points instead of the frame's
// ------------------------------------------------------------------------------------------
struct InitPointsParams {
    DevMesh dm;
    DevSettings st;
    WalkQueue out;
    uint32_t *count_out;
    const float *points;     // the call's points (x, y); this launch takes points [first, first + n)
    float *field;            // the call's field: a walker's pix is its point's index in the call
    int32_t first, n;
    int32_t seed_base, seed_width;
    int32_t stack_stride;
    // a call on a carried point list (wost_points_more & co., carry_n != nullptr), as in InitParams: a point with carry_n[i] > 0
    // samples behind it starts from its carried generator state and raw sums (its depth-0 closest point is queried again); a
    // point whose byte in select (nullptr: every point) is 0 is not queued.  The kernel that closes the call writes the field.
    const uint64_t *carry_rng;
    const float *carry_sum;
    const uint32_t *carry_n;
    const uint8_t *select;
};

// Thread t takes point i = first + t of the call: the stream of pixel seed_base + i in a
// frame seed_width wide, pix = i, the rest as init_kernel writes it (the record is written out in both: a shared function
// changes init_kernel's code, EXPERIMENTS 51).  A point with a non-finite coordinate is never queued -- no walker may carry a
// NaN into a persistent launch -- and its field entry is NaN.  A caller's point can lie thousands of extents from the mesh,
// where the descent opens every box: the depth-0 query is closest_point_lockstep, which scans by the wave beyond dm.huge2.
__global__ __launch_bounds__(256) void init_points_kernel(InitPointsParams P)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t *stack = lds_stack + threadIdx.x;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool owned = t < P.n;
    const int pid = P.first + (owned ? t : 0);
    float x0 = 0, y0 = 0;
    if (owned) {
        x0 = P.points[2 * (size_t)pid];
        y0 = P.points[2 * (size_t)pid + 1];
    }
    const bool finite = isfinite(x0) && isfinite(y0);
    const bool active = owned && finite && P.st.spp > 0 && (P.select == nullptr || P.select[pid] != 0);
    if (owned && !active) {
        float *f = P.field + 3 * (size_t)pid;
        const float z = finite ? 0.0f / (float)P.st.spp : __int_as_float(0x7fc00000);
        f[0] = z; f[1] = z; f[2] = z;
    }
    Pcg rng{0, 1};
    if (active) pcg_seed_pixel(rng, P.seed_base + pid, P.seed_width);
    const Closest c0 = closest_point_lockstep(P.dm, x0, y0, active, stack, P.stack_stride);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    if (active && P.carry_n != nullptr && P.carry_n[pid] > 0u) {
        rng.state = P.carry_rng[pid];
        const float *cs = P.carry_sum + 3 * (size_t)pid;
        sr = cs[0]; sg = cs[1]; sb = cs[2];
    }
    const uint32_t s = block_push(active, P.count_out);
    if (active) {
        WalkQueue &q = P.out;
        q.pix[s] = pid;
        q.x0[s] = x0; q.y0[s] = y0;
        q.px[s] = x0; q.py[s] = y0;
        q.rng[s] = rng.state;
        q.meta[s] = META_PACK(0, 0, 0);
        q.nx[s] = 0.0f; q.ny[s] = 0.0f;
        q.hint[s] = c0.slot;
        q.thp[s] = 1.0f;
        q.sr[s] = sr; q.sg[s] = sg; q.sb[s] = sb;
        q.d0_d2[s] = c0.d2;
        q.d0_slot[s] = c0.slot;
    }
}

// ------------------------------------------------------------------------------------------
// the walk round
// ------------------------------------------------------------------------------------------
struct Lane {
    float x0, y0, px, py;
    Pcg rng;
    uint32_t sample, depth;
    bool on_n;
    float nx, ny;
    int32_t hint;
    float thp;
    float sr, sg, sb;
    float d0_d2;
    int32_t d0_slot;
};

// Per-lane event counters of one launch, packed two 16-bit fields per register (the kernels
// are register-bound; a lane makes at most steps_per_round <= 32767 steps per launch):
// a = steps | started << 16, b = absorbed | truncated << 16, c = Neumann hits, visits = LBVH
// nodes visited (32 bits).
struct LaneStats {
    uint32_t a, b, c, visits;
};

// The part of one walk step that follows the closest-point query.  One walk step = one item
// consumed from the reference's evaluation-point queue at one depth: separate ->
// handleBoundary -> sampleNeumann -> oneStepWalk (reference
// integrator/uniform/integrator.cu:128-211, 224-231, 336-444, 465-525).  `cp` is the result
// of lbvh nearest() for L.px,L.py (ignored when there is no Dirichlet boundary).
// Returns STEP_* status bits (STEP_ENDED when the walk ended in this step); the caller keeps
// the statistics, so no counter is ever touched inside a divergent branch.
// `chain` (the chained start): a walk that is absorbed here does not leave the function.  The next sample of the pixel starts
// at the evaluation point, whose closest point is cached (d0_d2, d0_slot), so its depth-0 step needs no query: the lane takes
// that sample's state and falls through the rest of the function as its depth-0 step, beside the lanes of the wave that are
// in the middle of a walk -- instead of waiting, masked off, for the wave's next step trip to do the same arithmetic there
// (STEP_ABSORBED | STEP_CHAINED, and STEP_ENDED only if the chained step itself ends its walk).  Not for the pixel's last
// sample, and not where the evaluation point lies inside the shell (or its distance is a NaN): that depth-0 step absorbs
// again and stays on the old path; with r0 >= eps the in-shell test that the chained step skips is false whatever uv is.
// status bits returned by step_finish
enum : uint32_t { STEP_ENDED = 1u, STEP_ABSORBED = 2u, STEP_TRUNCATED = 4u, STEP_NEUMANN_HIT = 8u, STEP_CHAINED = 16u };

// UNI: the tables of a flat Neumann mesh through the scalar path (wost_device.h: table_load) -- for the kernels that store to
// global memory inside their scheduler loop, where the compiler reads them per lane otherwise.
template <bool NEUMANN_EMISSIVE, bool NEUMANN_TREE, bool SOURCE = false, bool UNI = false, class STK = LdsColumn>
__device__ __forceinline__ uint32_t step_finish(const DevMesh &dm, const DevMesh &nm, const DevSettings &st, Lane &L,
                                                const Closest cp, const STK &stk, const DevSource &src = DevSource{},
                                                const bool chain = false)
{
    const bool has_d = dm.n_segs > 0, has_n = nm.n_segs > 0;
    const float eps = st.eps;
    float px = L.px, py = L.py;
    uint32_t chained = 0u;

    // ---- separateEvaluationPoint -------------------------------------------------------
    float R_D = WOST_INF;
    if (has_d) {
        L.hint = cp.slot;
        const float4 a = dm.segA[cp.slot];
        const float inv = dm.segInv[cp.slot];
        const float wx = px - a.x, wy = py - a.y;
        const float uv = dot2(wx, wy, a.z, a.w) * inv;       // computeProjectionRatio
        const float cr = cross2(a.z, a.w, wx, wy);           // checkPointSide
        const int side = (0.0f < cr) - (cr < 0.0f);
        R_D = sqrtf(cp.d2);
        const bool in_shell = (R_D < eps) && (uv > 0.0f && uv < 1.0f);
        if (in_shell) {
            // ---- handleBoundary ----
            float r, g, b;
            surface_color(dm.segCol + 12 * (size_t)cp.slot, side, uv, r, g, b);
            r *= st.dirichlet_intensity; g *= st.dirichlet_intensity; b *= st.dirichlet_intensity;
            r *= L.thp; g *= L.thp; b *= L.thp;
            L.sr = r + L.sr; L.sg = g + L.sg; L.sb = b + L.sb;
            const float r0 = sqrtf(L.d0_d2);
            if (!(chain && L.sample + 1u < (uint32_t)st.spp && r0 >= eps)) return STEP_ENDED | STEP_ABSORBED;
            // ---- the chained start: generateEvaluationPoints for the next sample, and its depth-0 step from here ----
            L.sample++;
            px = L.x0; py = L.y0;
            L.depth = 0; L.on_n = false; L.nx = 0.0f; L.ny = 0.0f;
            L.thp = 1.0f;
            L.hint = L.d0_slot;
            R_D = r0;
            chained = STEP_ABSORBED | STEP_CHAINED;
        }
    }
    float R_N = WOST_INF;
    if (has_n) R_N = closest_silhouette<NEUMANN_TREE, UNI>(nm, px, py, R_D, stk);
    float R_B = fmaxf(WOST_R_B_FLOOR, fminf(R_D, R_N));
    R_B *= WOST_R_B_SHRINK;
    if (isinf(R_B)) return STEP_ENDED | chained;

    // ---- sampleSource (problems with a source term only) ------------------------------------
    if (SOURCE) {
        float cr_, cg_, cb_;
        if (source_sample<NEUMANN_TREE, UNI>(src, nm, eps, px, py, R_B, L.on_n, L.nx, L.ny, L.thp, L.rng, stk, cr_, cg_, cb_)) {
            L.sr = cr_ + L.sr; L.sg = cg_ + L.sg; L.sb = cb_ + L.sb;
        }
    }

    // ---- sampleNeumann -------------------------------------------------------------------
    if (has_n) {
        float cr_, cg_, cb_;
        if (neumann_sample<NEUMANN_EMISSIVE, NEUMANN_TREE, UNI>(nm, st.neumann_intensity, eps, px, py, R_B, L.on_n, L.nx, L.ny,
                                                                L.thp, L.rng, stk, cr_, cg_, cb_)) {
            L.sr = cr_ + L.sr; L.sg = cg_ + L.sg; L.sb = cb_ + L.sb;
        }
    }

    // ---- oneStepWalk ---------------------------------------------------------------------
    float dirx, diry, pdf, alpha;
    uniform_direction(L.on_n, L.nx, L.ny, L.rng, dirx, diry, pdf, alpha);
    float nxt_x, nxt_y, hnx, hny;
    const bool hit = walk_advance<NEUMANN_TREE, UNI>(nm, eps, px, py, R_B, L.on_n, L.nx, L.ny, dirx, diry, stk, nxt_x, nxt_y,
                                                     hnx, hny);
    const uint32_t hit_count = hit ? 1u : 0u;
    // 1/pdf/alpha/2pi is exactly 1.0f in fp32 for both branches (tests/test_oracle_units.py),
    // so a unit throughput stays a unit throughput without three IEEE divisions
    if (L.thp != 1.0f) L.thp = L.thp / pdf / alpha / WOST_2PI;
    L.px = nxt_x; L.py = nxt_y;
    L.on_n = hit; L.nx = hnx; L.ny = hny;
    L.depth++;
    const bool truncated = L.depth == (uint32_t)st.max_depth;
    return (truncated ? (STEP_ENDED | STEP_TRUNCATED) : 0u) | (hit_count ? STEP_NEUMANN_HIT : 0u) | chained;
}

// step_finish for ALL lanes of a wave at once, `stepping` marking those that take the step: the same statements in the same
// order per walker, but the two tree queries on the Neumann side -- the closest silhouette vertex after the Dirichlet part, the
// walker's ray at the end -- are answered by the wave as a whole between the parts (wost_coop.h).  Neumann meshes on the tree only.
template <bool NEUMANN_EMISSIVE, bool SOURCE, class STK>
__device__ __forceinline__ uint32_t step_finish_wave(const DevMesh &dm, const DevMesh &nm, const DevSettings &st, Lane &L, const Closest cp,
                                                     bool stepping, const WavePool &W, const STK &stk, int ray_slot_trigger, const DevSource &src)
{
    const bool has_d = dm.n_segs > 0;
    const float eps = st.eps;
    const float px = L.px, py = L.py;
    uint32_t status = 0u;
    bool mid = stepping;
    // ---- separateEvaluationPoint / handleBoundary ----
    float R_D = WOST_INF;
    if (stepping && has_d) {
        L.hint = cp.slot;
        const float4 a = dm.segA[cp.slot];
        const float inv = dm.segInv[cp.slot];
        const float wx = px - a.x, wy = py - a.y;
        const float uv = dot2(wx, wy, a.z, a.w) * inv;
        const float cr = cross2(a.z, a.w, wx, wy);
        const int side = (0.0f < cr) - (cr < 0.0f);
        R_D = sqrtf(cp.d2);
        if ((R_D < eps) && (uv > 0.0f && uv < 1.0f)) {
            float r, g, b;
            surface_color(dm.segCol + 12 * (size_t)cp.slot, side, uv, r, g, b);
            r *= st.dirichlet_intensity; g *= st.dirichlet_intensity; b *= st.dirichlet_intensity;
            r *= L.thp; g *= L.thp; b *= L.thp;
            L.sr = r + L.sr; L.sg = g + L.sg; L.sb = b + L.sb;
            status = STEP_ENDED | STEP_ABSORBED;
            mid = false;
        }
    }
    const float R_N = closest_silhouette_wave(nm, px, py, R_D, mid, W, stk);
    float R_B = 0.0f, dirx = 0.0f, diry = 0.0f, pdf = 1.0f, alpha = 1.0f;
    bool go = false;
    if (mid) {
        R_B = fmaxf(WOST_R_B_FLOOR, fminf(R_D, R_N));
        R_B *= WOST_R_B_SHRINK;
        if (isinf(R_B)) {
            status = STEP_ENDED;
        } else {
            if (SOURCE) {
                float cr_, cg_, cb_;
                if (source_sample<true>(src, nm, eps, px, py, R_B, L.on_n, L.nx, L.ny, L.thp, L.rng, stk, cr_, cg_, cb_)) {
                    L.sr = cr_ + L.sr; L.sg = cg_ + L.sg; L.sb = cb_ + L.sb;
                }
            }
            {
                float cr_, cg_, cb_;
                if (neumann_sample<NEUMANN_EMISSIVE, true>(nm, st.neumann_intensity, eps, px, py, R_B, L.on_n, L.nx, L.ny, L.thp, L.rng, stk, cr_, cg_, cb_)) {
                    L.sr = cr_ + L.sr; L.sg = cg_ + L.sg; L.sb = cb_ + L.sb;
                }
            }
            uniform_direction(L.on_n, L.nx, L.ny, L.rng, dirx, diry, pdf, alpha);
            go = true;
        }
    }
    // ---- oneStepWalk: walk_advance with the ray answered by the wave ----
    float cxp = px, cyp = py;
    if (go && L.on_n) {
        cxp += eps * L.nx;
        cyp += eps * L.ny;
    }
    float t = 0.0f;
    int hi = -1;
    const bool hit = ray_closest_wave(nm, cxp, cyp, dirx, diry, R_B, go, t, hi, W, stk, ray_slot_trigger);
    if (go) {
        float nxt_x = px + R_B * dirx, nxt_y = py + R_B * diry, hnx = 0.0f, hny = 0.0f;
        if (hit) {
            hnx = nm.flat[hi].nx;
            hny = nm.flat[hi].ny;
            if (dot2(hnx, hny, dirx, diry) > 0) { hnx = -hnx; hny = -hny; }
            nxt_x = cxp + t * dirx;
            nxt_y = cyp + t * diry;
        }
        if (L.thp != 1.0f) L.thp = L.thp / pdf / alpha / WOST_2PI;
        L.px = nxt_x; L.py = nxt_y;
        L.on_n = hit; L.nx = hnx; L.ny = hny;
        L.depth++;
        const bool truncated = L.depth == (uint32_t)st.max_depth;
        status = (truncated ? (STEP_ENDED | STEP_TRUNCATED) : 0u) | (hit ? STEP_NEUMANN_HIT : 0u);
    }
    return status;
}

__device__ __forceinline__ void load_lane(const WalkQueue &q, uint32_t slot, Lane &L, uint32_t &pix)
{
    pix = q.pix[slot];
    L.x0 = q.x0[slot]; L.y0 = q.y0[slot];
    L.px = q.px[slot]; L.py = q.py[slot];
    L.rng.state = q.rng[slot]; L.rng.inc = 1;
    const uint32_t m = q.meta[slot];
    L.sample = META_SAMPLE(m); L.depth = META_DEPTH(m); L.on_n = META_ONN(m) != 0;
    L.nx = q.nx[slot]; L.ny = q.ny[slot];
    L.hint = q.hint[slot];
    L.thp = q.thp[slot];
    L.sr = q.sr[slot]; L.sg = q.sg[slot]; L.sb = q.sb[slot];
    L.d0_d2 = q.d0_d2[slot]; L.d0_slot = q.d0_slot[slot];
}

__device__ __forceinline__ void store_lane(const WalkQueue &q, uint32_t s, const Lane &L, uint32_t pix)
{
    q.pix[s] = pix;
    q.x0[s] = L.x0; q.y0[s] = L.y0;
    q.px[s] = L.px; q.py[s] = L.py;
    q.rng[s] = L.rng.state;
    q.meta[s] = META_PACK(L.sample, L.depth, L.on_n ? 1 : 0);
    q.nx[s] = L.nx; q.ny[s] = L.ny;
    q.hint[s] = L.hint;
    q.thp[s] = L.thp;
    q.sr[s] = L.sr; q.sg[s] = L.sg; q.sb[s] = L.sb;
    q.d0_d2[s] = L.d0_d2; q.d0_slot[s] = L.d0_slot;
}

// A pixel is resolved (reference integrator.cu:616-620): its sums divided by its samples.  CARRY (a continued solve): the
// generator state and the raw sums stay behind under the pixel id for the next call, and the samples are those of all calls.
template <bool CARRY>
__device__ __forceinline__ void resolve_pixel(const RoundParams &P, uint32_t pix, const Lane &L)
{
    float *f = P.field + 3 * (size_t)((int32_t)pix - P.field_base);
    if (CARRY) {
        P.carry_rng[pix] = L.rng.state;
        float *cs = P.carry_sum + 3 * (size_t)pix;
        cs[0] = L.sr; cs[1] = L.sg; cs[2] = L.sb;
    }
    const float spp = (float)(CARRY ? P.carry_total : P.st.spp);
    f[0] = L.sr / spp; f[1] = L.sg / spp; f[2] = L.sb / spp;
}

// walkers order[0 .. n) of `in` (0 .. n without an order) copied to slots 0 .. n of `out`
__global__ __launch_bounds__(256) void gather_walkers_kernel(WalkQueue in, const uint32_t *order, uint32_t n, WalkQueue out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Lane L;
    uint32_t pix;
    load_lane(in, order ? order[i] : i, L, pix);
    store_lane(out, i, L, pix);
}

// REFILL = false: one thread per queue slot, the round ends after steps_per_round steps and the
// survivors are compacted (the throughput path: with many samples per pixel a slot keeps itself
// busy by regenerating).  REFILL = true: a fixed number of resident threads; a lane whose pixel
// is complete writes it out and takes the next unread slot of the input queue (one atomic per
// wave), so the whole solve is ONE launch and no lane idles while work is left -- the
// low-sample-count path (time-to-1spp), where regeneration cannot fill the lanes.
// SLACK = false, the kernel of every ordinary launch: node visits in the plain form, exact within dm.far2 of the Dirichlet mesh.
// A walker whose query starts beyond that (it leaked through a corner of the boundary or escaped through an open one, or the
// probe looks at the scene from afar) stops there, untouched, and goes to the far end of the output queue; the host runs those
// few walkers through the SLACK = true instantiation -- node visits exact at any distance (trav_visit<true>), which costs this
// kernel a quarter of its throughput: more visits and, above all, registers -- for the length of a walk and returns them.
// PERSIST (with REFILL): the persistent first launch of a many-sample solve.  The same code, minus the state that only the
// few-samples form needs: no wave-private reservation (a refill is rare: exactly the slots needed, one atomic per refill), no
// 32-bit totals of the lane counters (a lane adds its counters to the statistics when its pixel is complete: six atomics per
// pixel).  Eight registers fewer -- the instantiation wants 98 where six waves per SIMD allow 80, and what it spilled was not
// only cold: the PCG state went through scratch at every step (a build with 96 registers and five waves per SIMD was 7 % faster
// than the spilling one at the same five waves, profiles/r06_o_*).
// CARRY: the body of walk_round_carry_kernel, the entry of a continued solve (resolve_pixel).  A flag of the body and a second
// entry, not a seventh parameter of walk_round_kernel and not a test at run time: the frame kernels keep their names and their code.
template <bool NEUMANN_EMISSIVE, bool NEUMANN_TREE, bool REFILL, bool SOURCE, bool SLACK, bool PERSIST, bool CARRY>
__device__ __forceinline__ void walk_round_body(const RoundParams &P)
{
    extern __shared__ uint32_t lds_stack[];       // the traversal stack columns, one per lane
    uint32_t *stack = lds_stack + threadIdx.x;
    // thin waves (lane_shift > 0, the last launches of a solve): only every 2^shift-th lane holds a
    // walker, so a wave waits for the longest query of 64 >> shift walkers instead of 64
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t slot = tid >> P.lane_shift;
    const uint32_t n_in = *P.count_in;
    const bool valid = slot < n_in && (tid & ((1u << P.lane_shift) - 1u)) == 0u;
    Lane L;
    LaneStats S{0, 0, 0, 0};
    uint32_t pix = 0;
    bool alive = false;
    if (valid) {
        load_lane(P.in, P.order ? P.order[slot] : slot, L, pix);
        alive = L.sample < (uint32_t)P.st.spp;
    }
    bool open = valid;            // this lane holds a pixel whose result has not been written
    uint32_t wide[6] = {0, 0, 0, 0, 0, 0};   // REFILL: 32-bit totals of the packed 16-bit lane counters
    uint32_t pool_next = 0, pool_end = 0;    // REFILL: this wave's reserved input slots [next, end)
    // Per-lane state machine.  A lane either has an INNER node or a LEAF of the LBVH to visit
    // for its current walk position, WAITs with a finished query for the step logic, or is DONE
    // for this round.  Query lengths differ wildly between lanes, so instead of running every
    // lane's query to completion in lock step, each trip of the loop runs ONE of two bodies
    // -- "visit one node" or "finish a step and start the next query" -- whichever more lanes
    // of the wave are ready for (weighted), while the lanes of the other kind accumulate.
    enum { MODE_TRAV = 1, MODE_WAIT = 3, MODE_DONE = 4, MODE_REFILL = 5, MODE_FAR = 6, MODE_HUGE = 7 };
    const bool has_d = P.dm.n_segs > 0;
    int mode = alive ? MODE_WAIT : MODE_DONE;
    bool fresh = true;   // first trip: no finished step yet, only start the query
    // (PERSIST with leave_dry 2: no round ends such a launch, and the budget counts the steps to the wave's next look at the
    // cursor instead, above kLookBase -- see the end of the step phase; no register beside the 80 the instantiation lives on)
    constexpr int kLookBase = 1 << 30;
    int budget = (PERSIST && P.leave_dry == 2) ? kLookBase + P.dry_cadence : P.steps_per_round;
    Trav T = trav_begin(Closest{WOST_INF, -1});
    uint32_t trav_trips = 0, step_trips = 0;   // wave-uniform: scheduler diagnostics
#ifdef WOST_TRACK
    uint32_t trk_leaf = 0, trk_ge6 = 0, trk_ge10 = 0, trk_ge14 = 0;
    int trk_sp = 0;
#define WOST_TRACK_VISIT_PRE() do { trk_leaf += (T.level == P.dm.levels) ? 1u : 0u; } while (0)
#define WOST_TRACK_VISIT_POST() do { trk_sp = max(trk_sp, T.sp); trk_ge6 += T.sp >= 6; trk_ge10 += T.sp >= 10; trk_ge14 += T.sp >= 14; } while (0)
#else
#define WOST_TRACK_VISIT_PRE() do {} while (0)
#define WOST_TRACK_VISIT_POST() do {} while (0)
#endif
#ifdef WOST_DRAIN
    // (no lane has left the loop's wave-uniform control flow at either place: the first active lane speaks for the wave; a
    // wave's budgets are all positive until it stops and none is afterwards)
#define WOST_DRAIN_STOP() do { if (PERSIST && budget > 0 && (threadIdx.x & 63) == 0) { \
        const unsigned long long t_ = wall_clock64(); StatsDev *sd_ = my_stats(P.stats); \
        atomicMax(&sd_->stop_min, ~t_); atomicMax(&sd_->stop_max, t_); atomicAdd(&sd_->stop_sum, t_); atomicAdd(&sd_->stop_waves, 1ull); } } while (0)
#else
#define WOST_DRAIN_STOP() do {} while (0)
#endif
    const LdsColumn stk{stack, (uint32_t)P.stack_stride};
    for (;;) {
        if (REFILL) {
            // lanes whose pixel is complete: write it, then take the next unread input slot
            const unsigned long long need = __ballot(mode == MODE_REFILL);
            if (need) {
                // slots come from a wave-private reservation of 64 (one atomic on the shared cursor
                // per 64 pixels, not per refill: same-address atomics serialise in L2)
                // (many samples per pixel: a refill is rare -- config 2: one per wave and 30 walk steps -- and unread slots
                // parked in 6 000 private reservations would be a fifth of the frame when the cursor runs dry: reserve = 0 takes
                // exactly the slots needed)
                const int lane_ = threadIdx.x & 63;
                const uint32_t needed = (uint32_t)__popcll(need);
                const uint32_t rank = (uint32_t)__popcll(need & ((1ull << lane_) - 1ull));
                uint32_t s2;
                if (PERSIST) {
                    uint32_t fresh_base = 0;
                    if (lane_ == 0) fresh_base = atomicAdd(P.cursor, needed);
                    s2 = __shfl(fresh_base, 0) + rank;
                } else {
                    const uint32_t avail = pool_end - pool_next;
                    uint32_t fresh_base = 0;
                    const uint32_t want = P.reserve > 0 ? (uint32_t)P.reserve : needed - min(needed, avail);
                    if (needed > avail) {
                        if (lane_ == 0) fresh_base = atomicAdd(P.cursor, want);
                        fresh_base = __shfl(fresh_base, 0);
                    }
                    s2 = rank < avail ? pool_next + rank : fresh_base + (rank - avail);
                    if (needed > avail) {
                        pool_next = fresh_base + (needed - avail);
                        pool_end = fresh_base + want;
                    } else {
                        pool_next += needed;
                    }
                }
                // the queue is dry: with leave_dry the wave stops here -- no new step starts (budget 0), queries in flight finish
                // their step, pixels still open go to the output queue at the end of the kernel like the survivors of a round
                if (P.leave_dry && __ballot(mode == MODE_REFILL && s2 >= n_in)) {
                    WOST_DRAIN_STOP();
                    budget = 0;
                }
                if (mode == MODE_REFILL) {
                    if (open) {       // (a walker that left for the slack launch is not resolved here: `open` is false)
                        resolve_pixel<CARRY>(P, pix, L);
                    }
                    open = false;
                    if (PERSIST) {
                        StatsDev *sd = my_stats(P.stats);
                        if (S.a & 0xffffu) atomicAdd(&sd->steps, (unsigned long long)(S.a & 0xffffu));
                        if (S.a >> 16) atomicAdd(&sd->started, (unsigned long long)(S.a >> 16));
                        if (S.b & 0xffffu) atomicAdd(&sd->absorbed, (unsigned long long)(S.b & 0xffffu));
                        if (S.b >> 16) atomicAdd(&sd->truncated, (unsigned long long)(S.b >> 16));
                        if (S.c) atomicAdd(&sd->nhits, (unsigned long long)S.c);
                        if (S.visits) atomicAdd(&sd->inner_visits, (unsigned long long)S.visits);
                    } else {
                        wide[0] += S.a & 0xffffu; wide[1] += S.a >> 16; wide[2] += S.b & 0xffffu; wide[3] += S.b >> 16;
                        wide[4] += S.c; wide[5] += S.visits;
                    }
                    S = LaneStats{0, 0, 0, 0};
                    if (s2 < n_in) {
                        load_lane(P.in, P.order ? P.order[s2] : s2, L, pix);
                        open = true;
                        alive = L.sample < (uint32_t)P.st.spp;
                        fresh = true;
                        mode = alive ? MODE_WAIT : MODE_REFILL;
                    } else {
                        mode = MODE_DONE;
                    }
                }
            }
        }
        int n_trav = __popcll(__ballot(mode == MODE_TRAV));
        int n_wait = __popcll(__ballot(mode == MODE_WAIT));
        if (n_trav + n_wait == 0) {
            if (REFILL && __ballot(mode == MODE_REFILL)) continue;
            break;
        }
        if (n_wait * P.wait_weight < n_trav * 8) {
            // ---- traversal phase: every traversing lane visits one node ----
            // The phase is a loop of its own: after a burst the scheduler's test is made right here, and while it still
            // prefers traversal the next burst follows without a trip through the outer loop.  The outer loop carries the
            // whole lane state (Lane, Trav, mode, counters) and the compiler gives that state one home in registers across
            // the back edge and another inside each body, with copies in and out; about two of three traversal trips follow
            // a traversal trip, and those now pay none of them (EXPERIMENTS "Register copies around the scheduler loop").
            // Same ballots, same test, same counters: the sequence of bodies a wave runs is what it was.  A lane that waits
            // for a refill (a REFILL launch took a pixel with no sample left) is served at the head of the outer loop, so
            // such a wave goes back there after every burst as before; no lane turns to MODE_REFILL inside this phase.
            const bool refill_waiting = REFILL && __ballot(mode == MODE_REFILL) != 0ull;
            for (;;) {
                ++trav_trips;
#ifndef WOST_TRAV_BURST
#define WOST_TRAV_BURST 3       // the burst the kernel is unrolled for: the automatic one of rounds with a Neumann mesh on the tree (set_schedule)
#endif
                if (!PERSIST && P.trav_burst == WOST_TRAV_BURST) {
                    // that burst, unrolled: no loop counter, and the compiler may start a visit's node load early
#pragma unroll
                    for (int b = 0; b < WOST_TRAV_BURST; ++b) {
                        if (mode == MODE_TRAV) {
                            S.visits++;
                            WOST_TRACK_VISIT_PRE();
                            if (!trav_visit<SLACK>(P.dm, L.px, L.py, T, stk)) mode = MODE_WAIT;
                            WOST_TRACK_VISIT_POST();
                        }
                    }
                } else {
                    for (int b = 0; b < P.trav_burst; ++b) {
                        if (mode == MODE_TRAV) {
                            S.visits++;
                            WOST_TRACK_VISIT_PRE();
                            if (!trav_visit<SLACK>(P.dm, L.px, L.py, T, stk)) mode = MODE_WAIT;
                            WOST_TRACK_VISIT_POST();
                        }
                    }
                }
                if (refill_waiting) break;
                n_trav = __popcll(__ballot(mode == MODE_TRAV));
                n_wait = __popcll(__ballot(mode == MODE_WAIT));
                if (n_wait * P.wait_weight >= n_trav * 8) break;      // (also when no lane is left in either mode)
            }
            // The test prefers the step phase now, and it is the test the next trip would make on the same modes: the step phase
            // follows at once, in this trip, with the state where the traversal left it -- not after a round through the back
            // edge, which moved every value to its register of the loop head and back.  Only a wave with nothing left to do, or
            // with a lane waiting for a refill, goes to the head.
            // (Not in the persistent launch, which lives on 80 registers: with both phases in one trip its scratch grew from
            // 44 to 104 bytes per lane, spill code inside the loop.  It goes to the head, which makes the same test again.)
            if (PERSIST || refill_waiting || n_trav + n_wait == 0) continue;
        }
        {
            // ---- step phase ----
            ++step_trips;
            uint32_t wave_status = 0u;
            if (NEUMANN_TREE && P.coop) {
                // (8-byte LDS atomics: the pools start at an 8-byte boundary whatever lies before the dynamic segment)
                uint32_t *pw = reinterpret_cast<uint32_t *>((reinterpret_cast<uintptr_t>(lds_stack + P.pool_offset) + 7u) & ~(uintptr_t)7u) +
                               (threadIdx.x >> 6) * (2 * P.pool_cap + kPoolOwnerWords);
                const WavePool W{pw + kPoolOwnerWords, pw + kPoolOwnerWords + P.pool_cap, pw, P.pool_cap};
                wave_status = step_finish_wave<NEUMANN_EMISSIVE, SOURCE>(P.dm, P.nm, P.st, L, T.best, mode == MODE_WAIT && !fresh, W, stk, P.ray_slot_trigger, P.src);
            }
            // (two branches side by side, not one inside the other: nested, every value that only the inner one changes was
            // copied to its register of the join twice, once in front of each)
            if (mode == MODE_WAIT && !fresh) {
                {
                    const uint32_t status = (NEUMANN_TREE && P.coop) ? wave_status
                                                                     : step_finish<NEUMANN_EMISSIVE, NEUMANN_TREE, SOURCE, REFILL>(P.dm, P.nm, P.st, L, T.best, stk, P.src, P.chain && budget > 1);
                    const bool ended = (status & STEP_ENDED) != 0u;
                    S.b += ((status >> 1) & 1u) | (((status >> 2) & 1u) << 16);
                    S.c += (status >> 3) & 1u;
                    // a chained start is two walk steps: the absorbed one, counted when its query began, and the next sample's
                    // depth-0 step -- one step and one walk started, and a unit of the budget of its own.  (budget > 1 above:
                    // the lane stays within steps_per_round and its 16-bit counters, a round of one step takes the old path, a
                    // wave that has stopped -- budget 0 -- starts nothing.)
                    if (status & STEP_CHAINED) {
                        S.a += 0x10001u;
                        --budget;
                    }
                    if (ended) {
                        // next sample of this pixel starts right away (generateEvaluationPoints,
                        // reference integrator.cu:90-99 + workqueue.h:99-110)
                        L.sample++;
                        L.px = L.x0; L.py = L.y0;
                        L.depth = 0; L.on_n = false; L.nx = 0.0f; L.ny = 0.0f;
                        L.thp = 1.0f;
                        L.hint = L.d0_slot;
                        alive = L.sample < (uint32_t)P.st.spp;
                    }
                    --budget;
                }
            }
            if (mode == MODE_WAIT) {
                fresh = false;
                if (alive && budget > 0) {
                    if (!has_d || L.depth == 0) {
                        // depth 0 starts at the same point for every sample of the pixel: cached
                        S.a += 1u + ((L.depth == 0) ? 0x10000u : 0u);
                        T.best = Closest{L.d0_d2, L.d0_slot};
                        mode = MODE_WAIT;
                    } else {
                        T = trav_begin(slot_candidate(P.dm, L.hint, L.px, L.py));
                        if (!SLACK && T.best.d2 > P.dm.far2) {
                            mode = MODE_FAR;      // not started, not counted: the SLACK launch takes the step from here
                            if (REFILL) {
                                // a resident lane must go on draining the input queue (parked, it would strand the unread slots
                                // of its wave's reservation, and a launch whose lanes all strayed would drop the rest of the
                                // frame): the walker goes to the far end of the output queue right away -- strayed walkers are
                                // few, so one atomic each -- and the lane takes the next pixel
                                const uint32_t k = atomicAdd(P.count_far, 1u);
                                store_lane(P.out, P.out_capacity - 1u - k, L, pix);
                                open = false;
                                mode = MODE_REFILL;
                            }
                        } else {
                            S.a += 1u;
                            // SLACK: a query from so far away that every segment of the mesh ties within rounding is answered
                            // by the whole wave at the end of this trip
                            mode = (SLACK && T.best.d2 > P.dm.huge2) ? MODE_HUGE : MODE_TRAV;
                            // every query starts at the root, one address for the whole chip: visited here, from the scalar
                            // cache, not as the first gather of the lane's first burst.  (UNI as for the flat tables: the refilling
                            // kernels store inside this loop, and with a Neumann mesh on the tree the compiler proves nothing
                            // either -- the plain read was six per-lane loads there; the others issue scalar loads by themselves.)
                            if (P.root_visit && mode == MODE_TRAV) {
                                S.visits++;
                                WOST_TRACK_VISIT_PRE();
                                if (!trav_visit_root<SLACK, REFILL || NEUMANN_TREE>(P.dm, L.px, L.py, T, stk)) mode = MODE_WAIT;
                                WOST_TRACK_VISIT_POST();
                            }
                        }
                    }
                } else {
                    mode = (REFILL && !alive) ? MODE_REFILL : MODE_DONE;
                }
            }
            if (SLACK) {
                unsigned long long hb = __ballot(mode == MODE_HUGE);
                while (hb) {
                    const int src = __builtin_ctzll(hb);
                    const Closest r = closest_point_wave(P.dm, __shfl(L.px, src), __shfl(L.py, src));
                    if ((int)(threadIdx.x & 63) == src) {
                        T.best = r;
                        mode = MODE_WAIT;
                    }
                    hb &= hb - 1;
                }
            }
            if (PERSIST && P.leave_dry == 2 && __ballot((uint32_t)(budget - 1) < (uint32_t)kLookBase)) {
                // the global look (leave_dry 2): a wave that needs no refill learns here that the queue is dry, and stops like one
                // that does -- without it a wave walks on until one of ITS lanes completes a pixel, half a millisecond on average,
                // and the launch lasts until the last of six thousand waves has (9 - 12 ms in config 2, EXPERIMENTS 32), while
                // what the others handed over waits behind it.  The cursor only grows and claims beyond n_in keep it there, so
                // cursor >= n_in is exactly "no unread slot"; an atomic load of agent scope sees the other waves' atomics (a plain
                // load may be served from a stale line).  Such a load is answered beyond the L2 of the wave's XCD and the wave waits
                // for it: a look on every fourth trip of the whole launch cost 13 % of it.  So the wave looks rarely while the
                // queue is far from dry -- R unread slots last at least R >> dry_shift steps -- and every dry_cadence steps at the
                // end.  The steps are counted where they are counted already: every lane gets the number of steps to the next look
                // as its budget above kLookBase, and the first lane to use them up (a budget in 1 .. kLookBase; a wave that has
                // stopped has none above 0) makes the wave look.  (A chained start takes two units in one trip: from kLookBase + 1
                // the budget lands on kLookBase - 1, still inside 1 .. kLookBase, so no look is skipped.)
                const uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(P.cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if (cur >= n_in) WOST_DRAIN_STOP();
                budget = cur >= n_in ? 0 : kLookBase + (int)max((uint32_t)P.dry_cadence, (n_in - cur) >> P.dry_shift);
            }
        }
    }
    // ---- resolve finished pixels (reference integrator.cu:616-620) -------------------------
    if (open && !alive) {
        resolve_pixel<CARRY>(P, pix, L);
    }
    // ---- stream compaction of the survivors: ballot + popcount, one atomic per block ------
    const int lane = threadIdx.x & 63;
    const bool far = !SLACK && mode == MODE_FAR;
    uint32_t s = block_push(alive && open && !far, P.count_out);
    if (!SLACK) {
        __syncthreads();      // block_push reuses its shared words
        const uint32_t k = block_push(alive && open && far, P.count_far);
        if (far) s = P.out_capacity - 1u - k;
    }
    if (alive && open) store_lane(P.out, s, L, pix);
    if (REFILL && P.leave_dry) {
        // a persistent launch hands its open pixels to the rounds: how many walk steps a pixel still needs is known well by now --
        // its samples so far took S.a steps (the lane's counters restart with every pixel it takes), the rest will take about as
        // many each.  The host starts the longest remainders at once, four lanes to a walker, beside the rounds of the others.
        const float done = (float)L.sample, left = (float)((uint32_t)P.st.spp - L.sample);
        const float est = left * ((float)max(S.a & 0xffffu, 4u) / fmaxf(done, 1.0f));
        const bool is_long = alive && open && !far && est >= P.long_steps;
        if (alive && open && !far) P.out.est[s] = est;
        const unsigned long long lb = __ballot(is_long);
        if (lane == 0 && lb) atomicAdd(P.count_long, (uint32_t)__popcll(lb));
    }
    // ---- statistics: wave reduction, one atomic per counter per wave -----------------------
    uint32_t v[7] = {(S.a & 0xffffu) + wide[0], (S.a >> 16) + wide[1], (S.b & 0xffffu) + wide[2], (S.b >> 16) + wide[3],
                     S.c + wide[4], S.visits + wide[5], 0u};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        uint32_t x = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
        v[k] = x;
    }
    if (lane == 0) {
        StatsDev *st = my_stats(P.stats);
        if (v[0]) atomicAdd(&st->steps, (unsigned long long)v[0]);
        if (v[1]) atomicAdd(&st->started, (unsigned long long)v[1]);
        if (v[2]) atomicAdd(&st->absorbed, (unsigned long long)v[2]);
        if (v[3]) atomicAdd(&st->truncated, (unsigned long long)v[3]);
        if (v[4]) atomicAdd(&st->nhits, (unsigned long long)v[4]);
        if (v[5]) atomicAdd(&st->inner_visits, (unsigned long long)v[5]);
        atomicAdd(&st->trav_trips, (unsigned long long)trav_trips);
        atomicAdd(&st->step_trips, (unsigned long long)step_trips);
    }
#ifdef WOST_DRAIN
    if (PERSIST && lane == 0) atomicMax(&my_stats(P.stats)->end_max, (unsigned long long)wall_clock64());
#endif
#ifdef WOST_TRACK
    {
        uint32_t w[4] = {trk_leaf, trk_ge6, trk_ge10, trk_ge14};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            for (int off = 32; off > 0; off >>= 1) w[k] += __shfl_down(w[k], off);
        for (int off = 32; off > 0; off >>= 1) trk_sp = max(trk_sp, __shfl_down(trk_sp, off));
        if (lane == 0) {
            StatsDev *st = my_stats(P.stats);
            atomicAdd(&st->leaf_visits, (unsigned long long)w[0]);
            atomicAdd(&st->sp_ge6, (unsigned long long)w[1]);
            atomicAdd(&st->sp_ge10, (unsigned long long)w[2]);
            atomicAdd(&st->sp_ge14, (unsigned long long)w[3]);
            atomicMax(&st->max_stack, (unsigned long long)trk_sp);
        }
    }
#endif
}

#ifndef WOST_ROUND_WAVES
#define WOST_ROUND_WAVES 6      // waves per SIMD the round kernel is compiled for (tuning builds override it)
#endif
template <bool NEUMANN_EMISSIVE, bool NEUMANN_TREE, bool REFILL = false, bool SOURCE = false, bool SLACK = false, bool PERSIST = false>
__global__ __launch_bounds__(256, NEUMANN_TREE ? 4 : WOST_ROUND_WAVES) void walk_round_kernel(RoundParams P)
{
    walk_round_body<NEUMANN_EMISSIVE, NEUMANN_TREE, REFILL, SOURCE, SLACK, PERSIST, false>(P);
}
template <bool NEUMANN_EMISSIVE, bool NEUMANN_TREE, bool REFILL = false, bool SOURCE = false, bool SLACK = false, bool PERSIST = false>
__global__ __launch_bounds__(256, NEUMANN_TREE ? 4 : WOST_ROUND_WAVES) void walk_round_carry_kernel(RoundParams P)
{
    walk_round_body<NEUMANN_EMISSIVE, NEUMANN_TREE, REFILL, SOURCE, SLACK, PERSIST, true>(P);
}


// ------------------------------------------------------------------------------------------
// the walk round of an under-filled launch: four lanes per walker (wost_quad.h)
// ------------------------------------------------------------------------------------------
// Same rounds, same queue records, same per-walker arithmetic as walk_round_kernel -- and so the same field, counters
// and visiting order -- but a quad of lanes holds ONE walker: the closest-point descent is shared between the four
// lanes (one child box each), everything else runs replicated.  The host launches it when the walkers left would fill
// less than a quarter of the resident lanes, where a launch lasts as long as its longest chain of dependent visits.
template <bool NEUMANN_EMISSIVE, bool NEUMANN_TREE, bool SOURCE, bool SLACK, bool CARRY>
__device__ __forceinline__ void walk_quad_body(const RoundParams &P)
{
    extern __shared__ uint32_t lds_stack[];
    const int j = threadIdx.x & 3;
    const QuadColumn stk{lds_stack + (threadIdx.x >> 2) * P.stack_stride};     // stack_stride = entries per column here
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    // lane_shift > 0 (the very last rounds): only every 2^shift-th quad holds a walker, down to one walker per wave -- such a
    // wave never waits for another walker's query
    const uint32_t quad_id = tid >> 2;
    const uint32_t n_in = *P.count_in;
    uint32_t slot = quad_id >> P.lane_shift;
    bool valid = slot < n_in && (quad_id & ((1u << P.lane_shift) - 1u)) == 0u;
    if (P.thin_blocks > 0u) {
        const uint32_t quads_per_block = blockDim.x >> 2;
        if (blockIdx.x < P.thin_blocks) {
            slot = quad_id >> 2;
            valid = slot < P.thin_count && (quad_id & 3u) == 0u;
        } else {
            slot = P.thin_count + (quad_id - P.thin_blocks * quads_per_block);
            valid = slot < n_in;
        }
    }
    Lane L;
    LaneStats S{0, 0, 0, 0};
    uint32_t pix = 0;
    bool alive = false;
    if (valid) {
        load_lane(P.in, P.order ? P.order[slot] : slot, L, pix);
        alive = L.sample < (uint32_t)P.st.spp;
    }
    const bool open = valid;
    enum { MODE_TRAV = 1, MODE_WAIT = 3, MODE_DONE = 4, MODE_FAR = 6, MODE_HUGE = 7 };
    const bool has_d = P.dm.n_segs > 0;
    int mode = alive ? MODE_WAIT : MODE_DONE;       // quad-uniform throughout
    bool fresh = true;
    int budget = P.steps_per_round;
    Trav T = trav_begin(Closest{WOST_INF, -1});
    uint32_t trav_trips = 0, step_trips = 0;
    for (;;) {
        int n_trav = __popcll(__ballot(mode == MODE_TRAV));
        int n_wait = __popcll(__ballot(mode == MODE_WAIT));
        if (n_trav + n_wait == 0) break;
        if (n_wait * P.wait_weight < n_trav * 8) {
            // the traversal phase lasts while the scheduler's test prefers it, and the step phase follows it in the same trip
            // (see walk_round_kernel)
            for (;;) {
                ++trav_trips;
                for (int b = 0; b < P.trav_burst; ++b) {
                    if (mode == MODE_TRAV) {
                        S.visits++;
                        if (!quad_visit<SLACK>(P.dm, L.px, L.py, T, stk, j)) mode = MODE_WAIT;
                    }
                }
                n_trav = __popcll(__ballot(mode == MODE_TRAV));
                n_wait = __popcll(__ballot(mode == MODE_WAIT));
                if (n_wait * P.wait_weight >= n_trav * 8) break;
            }
            if (n_trav + n_wait == 0) break;
        }
        {
            ++step_trips;
            if (mode == MODE_WAIT && !fresh) {       // (beside the next branch, not around it: see walk_round_kernel)
                {
                    const uint32_t status = step_finish<NEUMANN_EMISSIVE, NEUMANN_TREE, SOURCE>(P.dm, P.nm, P.st, L, T.best, stk, P.src, P.chain && budget > 1);
                    const bool ended = (status & STEP_ENDED) != 0u;
                    S.b += ((status >> 1) & 1u) | (((status >> 2) & 1u) << 16);
                    S.c += (status >> 3) & 1u;
                    if (status & STEP_CHAINED) {       // the next sample's depth-0 step as well (see walk_round_kernel)
                        S.a += 0x10001u;
                        --budget;
                    }
                    if (ended) {
                        L.sample++;
                        L.px = L.x0; L.py = L.y0;
                        L.depth = 0; L.on_n = false; L.nx = 0.0f; L.ny = 0.0f;
                        L.thp = 1.0f;
                        L.hint = L.d0_slot;
                        alive = L.sample < (uint32_t)P.st.spp;
                    }
                    --budget;
                }
            }
            if (mode == MODE_WAIT) {
                fresh = false;
                if (alive && budget > 0) {
                    if (!has_d || L.depth == 0) {
                        S.a += 1u + ((L.depth == 0) ? 0x10000u : 0u);
                        T.best = Closest{L.d0_d2, L.d0_slot};
                        mode = MODE_WAIT;
                    } else {
                        T = trav_begin(slot_candidate(P.dm, L.hint, L.px, L.py));
                        if (!SLACK && T.best.d2 > P.dm.far2) {
                            mode = MODE_FAR;
                        } else {
                            S.a += 1u;
                            mode = (SLACK && T.best.d2 > P.dm.huge2) ? MODE_HUGE : MODE_TRAV;
                        }
                    }
                } else {
                    mode = MODE_DONE;
                }
            }
            if (SLACK) {
                unsigned long long hb = __ballot(mode == MODE_HUGE);
                while (hb) {
                    const int src = __builtin_ctzll(hb);
                    const Closest r = closest_point_wave(P.dm, __shfl(L.px, src), __shfl(L.py, src));
                    if (((int)(threadIdx.x & 63) >> 2) == (src >> 2)) {
                        T.best = r;
                        mode = MODE_WAIT;
                    }
                    hb &= ~(0xfull << (src & ~3));
                }
            }
        }
    }
    const bool lead = j == 0;       // one lane of the quad speaks for the walker
    if (open && !alive && lead) {
        resolve_pixel<CARRY>(P, pix, L);
    }
    const int lane = threadIdx.x & 63;
    const bool far = !SLACK && mode == MODE_FAR;
    uint32_t s = block_push(alive && open && !far && lead, P.count_out);
    if (!SLACK) {
        __syncthreads();
        const uint32_t k = block_push(alive && open && far && lead, P.count_far);
        if (far) s = P.out_capacity - 1u - k;
    }
    if (alive && open && lead) store_lane(P.out, s, L, pix);
    uint32_t v[7] = {(S.a & 0xffffu), (S.a >> 16), (S.b & 0xffffu), (S.b >> 16), S.c, S.visits, 0u};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        uint32_t x = lead ? v[k] : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
        v[k] = x;
    }
    if (lane == 0) {
        StatsDev *st = my_stats(P.stats);
        if (v[0]) atomicAdd(&st->steps, (unsigned long long)v[0]);
        if (v[1]) atomicAdd(&st->started, (unsigned long long)v[1]);
        if (v[2]) atomicAdd(&st->absorbed, (unsigned long long)v[2]);
        if (v[3]) atomicAdd(&st->truncated, (unsigned long long)v[3]);
        if (v[4]) atomicAdd(&st->nhits, (unsigned long long)v[4]);
        if (v[5]) atomicAdd(&st->inner_visits, (unsigned long long)v[5]);
        atomicAdd(&st->trav_trips, (unsigned long long)trav_trips);
        atomicAdd(&st->step_trips, (unsigned long long)step_trips);
    }
}

template <bool NEUMANN_EMISSIVE, bool NEUMANN_TREE, bool SOURCE, bool SLACK>
__global__ __launch_bounds__(256, 4) void walk_quad_kernel(RoundParams P)
{
    walk_quad_body<NEUMANN_EMISSIVE, NEUMANN_TREE, SOURCE, SLACK, false>(P);
}
template <bool NEUMANN_EMISSIVE, bool NEUMANN_TREE, bool SOURCE, bool SLACK>
__global__ __launch_bounds__(256, 4) void walk_quad_carry_kernel(RoundParams P)
{
    walk_quad_body<NEUMANN_EMISSIVE, NEUMANN_TREE, SOURCE, SLACK, true>(P);
}

// ------------------------------------------------------------------------------------------
// batch query kernels (the lbvh::query_device call sites, exposed for tests and SDF renders)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void closest_point_kernel(DevMesh m, const float *pts, int n, int32_t *out_idx,
                                                            float *out_dist, float *out_uv, int32_t *out_side,
                                                            int stack_stride)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t *stack = lds_stack + threadIdx.x;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float qx = pts[2 * i], qy = pts[2 * i + 1];
    const Closest c = closest_point(m, qx, qy, slot_candidate(m, 0, qx, qy), stack, stack_stride);
    float uv;
    int32_t side;
    segment_uv_side(m, c.slot, qx, qy, uv, side);
    if (out_idx) out_idx[i] = m.segOrig[c.slot];
    if (out_dist) out_dist[i] = sqrtf(c.d2);
    if (out_uv) out_uv[i] = uv;
    if (out_side) out_side[i] = side;
}

__global__ __launch_bounds__(256) void sdf_kernel(DevMesh m, DevProbe probe, int width, int height, int which,
                                                  float *out, int stack_stride)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t *stack = lds_stack + threadIdx.x;
    const int pid = blockIdx.x * blockDim.x + threadIdx.x;
    if (pid >= width * height) return;
    float x, y;
    eval_point(probe, pid % width, pid / width, width, height, x, y);
    float d = WOST_INF;
    if (m.n_segs > 0) {
        if (which == WOST_MESH_DIRICHLET) {
            d = sqrtf(closest_point(m, x, y, slot_candidate(m, 0, x, y), stack, stack_stride).d2);
        } else {
            d = (m.n_segs <= WOST_FLAT_MAX) ? closest_silhouette_flat(m, x, y, WOST_INF)
                                             : closest_silhouette_tree(m, x, y, WOST_INF, LdsColumn{stack, (uint32_t)stack_stride});
        }
    }
    out[pid] = d;
}

__global__ __launch_bounds__(256) void source_kernel(DevSource src, DevProbe probe, int width, int height, float *out)
{
    const int pid = blockIdx.x * blockDim.x + threadIdx.x;
    if (pid >= width * height) return;
    float x, y, r = 0.0f, g = 0.0f, b = 0.0f;
    eval_point(probe, pid % width, pid / width, width, height, x, y);
    if (src.rgb) source_eval(src, x, y, r, g, b);
    out[3 * (size_t)pid] = r; out[3 * (size_t)pid + 1] = g; out[3 * (size_t)pid + 2] = b;
}

__global__ __launch_bounds__(256) void silhouette_kernel(DevMesh m, const float *pts, const float *rmax, int n,
                                                         float *out)
{
    extern __shared__ uint32_t lds_stack[];
    const LdsColumn stk{lds_stack + threadIdx.x, (uint32_t)blockDim.x};
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float r = rmax ? rmax[i] : WOST_INF;
    out[i] = (m.n_segs <= WOST_FLAT_MAX) ? closest_silhouette_flat(m, pts[2 * i], pts[2 * i + 1], r)
                                         : closest_silhouette_tree(m, pts[2 * i], pts[2 * i + 1], r, stk);
}

__global__ __launch_bounds__(256) void ray_kernel(DevMesh m, const float *o, const float *d, const float *tmax, int n,
                                                  int32_t *out_hit, float *out_t, int32_t *out_idx)
{
    extern __shared__ uint32_t lds_stack[];
    const LdsColumn stk{lds_stack + threadIdx.x, (uint32_t)blockDim.x};
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float t;
    int idx;
    const bool hit = (m.n_segs <= WOST_FLAT_MAX)
                         ? ray_closest_flat(m, o[2 * i], o[2 * i + 1], d[2 * i], d[2 * i + 1], tmax[i], t, idx)
                         : ray_tree<false>(m, o[2 * i], o[2 * i + 1], d[2 * i], d[2 * i + 1], tmax[i], t, idx, stk);
    out_hit[i] = hit ? 1 : 0;
    out_t[i] = t;
    out_idx[i] = idx;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

// (declared in wost_host.h: every translation unit of the library reports through it)
int set_error(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}

}  // namespace wost

using namespace wost;

namespace wost {
SceneView scene_view(wost_handle h)
{
    return SceneView{h->device, h->dm.view, h->nm.view, h->dst, h->probe, h->mask, h->stream, h->src};
}
}  // namespace wost

// The arrays of a queue, in the order they are carved from its one allocation: the 8-byte array first, then the 4-byte arrays.
// f gets a reference to each pointer (the element size is sizeof(*p)).
template <class F>
static void for_each_array(WalkQueue &q, F &&f)
{
    f(q.rng); f(q.pix); f(q.x0); f(q.y0); f(q.px); f(q.py); f(q.meta); f(q.nx); f(q.ny);
    f(q.hint); f(q.thp); f(q.sr); f(q.sg); f(q.sb); f(q.d0_d2); f(q.d0_slot); f(q.est);
}

// bytes of a queue of n slots
static size_t queue_bytes(size_t n)
{
    WalkQueue q{};
    size_t bytes = 0;
    for_each_array(q, [&](auto *&a) { bytes += n * sizeof(*a); });
    return bytes;
}

static void carve_queue(void *mem, size_t n, WalkQueue &q)
{
    char *p = static_cast<char *>(mem);
    for_each_array(q, [&](auto *&a) {
        a = reinterpret_cast<std::remove_reference_t<decltype(a)>>(p);
        p += n * sizeof(*a);
    });
}

// the queue that starts k slots into q
static WalkQueue queue_from(WalkQueue q, size_t k)
{
    for_each_array(q, [&](auto *&a) { a += k; });
    return q;
}

static void destroy_ctx(wost_context *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (void *p : c->dm.allocs) (void)hipFree(p);
    for (void *p : c->nm.allocs) (void)hipFree(p);
    if (c->src.rgb) (void)hipFree(const_cast<float *>(c->src.rgb));
    for (int i = 0; i < 2; ++i)
        if (c->queue_mem[i]) (void)hipFree(c->queue_mem[i]);
    if (c->counts) (void)hipFree(c->counts);
    if (c->stats) (void)hipFree(c->stats);
    if (c->cursor) (void)hipFree(c->cursor);
    order_free(c->order);
    if (c->long_mem) (void)hipFree(c->long_mem);
    if (c->long_stream) (void)hipStreamDestroy(c->long_stream);
    if (c->long_ev0) (void)hipEventDestroy(c->long_ev0);
    if (c->long_ev1) (void)hipEventDestroy(c->long_ev1);
    if (c->far_stream) (void)hipStreamDestroy(c->far_stream);
    if (c->far_ev0) (void)hipEventDestroy(c->far_ev0);
    if (c->far_ev1) (void)hipEventDestroy(c->far_ev1);
    if (c->host_count) (void)hipHostFree(c->host_count);
    if (c->host_stats) (void)hipHostFree(c->host_stats);
    destroy_base(c);
    delete c;
}

// What wost_create adds to the shared part (create_handle, wost_uniform.h): the probe, the meshes, the source grid, the queues
// and counters of the rounds, the side streams and the order buffers.
static int fill_ctx(wost_context *c, const wost_scene_desc &scene)
{
    c->probe = DevProbe{scene.probe_scale, scene.probe_pos[0], scene.probe_pos[1], scene.probe_up[0], scene.probe_up[1]};
    int rc = upload_mesh(scene.dirichlet, c->dm);
    if (rc == WOST_OK) rc = upload_mesh(scene.neumann, c->nm);
    if (rc == WOST_OK) rc = upload_mask(c, scene.mask);
    if (rc != WOST_OK) return rc;
    c->dirichlet_verts = scene.dirichlet.n_segs > 0 ? scene.dirichlet.n_verts : 0;
    if (scene.source.nx > 0 && scene.source.ny > 0) {
        const wost_source_desc &sd = scene.source;
        if (!sd.rgb) return set_error(WOST_ERR_INVALID, "source grid without data");
        const size_t bytes = (size_t)sd.nx * sd.ny * 3 * sizeof(float);
        float *dev = nullptr;
        WOST_TRY(hipMalloc((void **)&dev, bytes));
        c->src = DevSource{dev, sd.nx, sd.ny, sd.index_scale[0], sd.index_scale[1], sd.index_offset[0], sd.index_offset[1],
                           sd.intensity};
        WOST_TRY(hipMemcpy(dev, sd.rgb, bytes, hipMemcpyHostToDevice));
    }
    const size_t qbytes = queue_bytes(c->n_pixels);
    for (int i = 0; i < 2; ++i) {
        WOST_TRY(hipMalloc(&c->queue_mem[i], qbytes));
        carve_queue(c->queue_mem[i], c->n_pixels, c->queue[i]);
    }
    WOST_TRY(hipMalloc((void **)&c->counts, 12 * sizeof(uint32_t)));   // two queue counts, the far count and its input copy; [4..7]: the hand-over of a persistent launch
    WOST_TRY(hipMalloc((void **)&c->stats, kStatCopies * sizeof(StatsDev)));
    WOST_TRY(hipMalloc((void **)&c->cursor, sizeof(uint32_t)));
    WOST_TRY(hipDeviceGetAttribute(&c->n_cus, hipDeviceAttributeMultiprocessorCount, c->device));
    WOST_TRY(hipHostMalloc((void **)&c->host_count, 8 * sizeof(uint32_t)));
    WOST_TRY(hipHostMalloc((void **)&c->host_stats, kStatCopies * sizeof(StatsDev)));
    if ((rc = create_frame(c)) != WOST_OK) return rc;
    WOST_TRY(hipStreamCreateWithFlags(&c->far_stream, hipStreamNonBlocking));
    WOST_TRY(hipEventCreateWithFlags(&c->far_ev0, hipEventDisableTiming));
    WOST_TRY(hipEventCreateWithFlags(&c->far_ev1, hipEventDisableTiming));
    {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        WOST_TRY(hipStreamCreateWithPriority(&c->long_stream, hipStreamNonBlocking, greatest));
    }
    WOST_TRY(hipEventCreateWithFlags(&c->long_ev0, hipEventDisableTiming));
    WOST_TRY(hipEventCreateWithFlags(&c->long_ev1, hipEventDisableTiming));
    {
        // the order of a persistent / one-launch solve: its buffers and the first use of its sort kernels (their code objects load
        // then: 2.5 ms) belong here, beside the tree builds, not inside the first solve -- time-to-1spp of a fresh handle
        WOST_TRY((hipError_t)order_alloc(c->order, c->n_pixels));
        const uint32_t n_warm = (uint32_t)std::min<size_t>(c->n_pixels, 1024);
        const uint32_t *unused = nullptr;
        WOST_TRY(hipMemsetAsync(c->queue[0].d0_d2, 0, n_warm * sizeof(float), c->stream));
        WOST_TRY(hipMemsetAsync(c->queue[0].est, 0, n_warm * sizeof(float), c->stream));
        WOST_TRY((hipError_t)order_by_distance(c->order, c->queue[0].d0_d2, n_warm, c->stream, &unused));
        WOST_TRY((hipError_t)order_by_estimate(c->order, c->queue[0].est, n_warm, c->stream, &unused));
        WOST_TRY(hipStreamSynchronize(c->stream));
    }
    return WOST_OK;
}

extern "C" {

// 0.2: the sync callback of a shared guiding network is also asked for the number of ranks (WOST_SYNC_RANKS_I64_HOST)
// 0.3: the carried point list (wost_points_carry & co., wost3_points_carry & co.)
const char *wost_version(void) { return "wost-hip 0.3 (gfx950)"; }

const char *wost_last_error(void) { return g_last_error.c_str(); }

int wost_create(const wost_scene_desc *scene, const wost_settings *settings, int device, wost_handle *out)
{
    return create_handle(scene, settings, device, out, true, destroy_ctx, fill_ctx);
}

int wost_destroy(wost_handle h)
{
    destroy_ctx(h);
    return WOST_OK;
}

int wost_set_option(wost_handle h, const char *key, double value)
{
    if (!h || !key) return set_error(WOST_ERR_INVALID, "null argument");
    const std::string k(key);
    if (k == "steps_per_round") {
        if (value < 0 || value > 32767) return set_error(WOST_ERR_INVALID, "steps_per_round must be in 0..32767 (0 = automatic)");
        h->steps_per_round = (int)value;
    } else if (k == "block_size") {
        const int b = (int)value;
        if (b != 64 && b != 128 && b != 256) return set_error(WOST_ERR_INVALID, "block_size must be 64, 128 or 256");
        h->block_size = b;
    } else if (k == "wait_weight") {
        if (value < 1 || value > 512) return set_error(WOST_ERR_INVALID, "wait_weight must be in 1..512");
        h->wait_weight = (int)value;
    } else if (k == "trav_burst") {
        if (value < 1 || value > 16) return set_error(WOST_ERR_INVALID, "trav_burst must be in 1..16");
        h->trav_burst = (int)value;
    } else if (k == "spp") {
        if (value < 0 || value >= (1 << 20)) return set_error(WOST_ERR_INVALID, "spp must be in 0..2^20-1");
        h->settings.spp = (int32_t)value;
        h->dst.spp = (int32_t)value;
    } else if (k == "refill") {
        if (value != -1 && value != 0 && value != 1) return set_error(WOST_ERR_INVALID, "refill must be -1 (auto), 0 or 1");
        h->refill = (int)value;
    } else if (k == "persist") {
        if (value != -1 && value != 0 && value != 1) return set_error(WOST_ERR_INVALID, "persist must be -1 (auto), 0 or 1");
        h->persist = (int)value;
    } else if (k == "persist_order") {
        h->persist_order = value != 0;
    } else if (k == "few_order") {
        h->few_order = value != 0;
    } else if (k == "long_steps") {
        // (the bound: above it the order by estimate no longer puts the long remainders first, wost_order.h)
        static_assert(kOrderMaxThreshold == 32760, "the bound is part of the option's text");
        if (value < 0 || value > kOrderMaxThreshold || ((int)value & 7)) return set_error(WOST_ERR_INVALID, "long_steps must be a multiple of 8 in 0..32760 (0 = no pixel runs beside the rounds)");
        h->long_steps = (int)value;
    } else if (k == "long_cap") {
        if (value < 1 || value > (1 << 20)) return set_error(WOST_ERR_INVALID, "long_cap must be in 1..2^20");
        h->long_cap = (int)value;
        if (h->long_mem) (void)hipFree(h->long_mem);
        h->long_mem = nullptr;
    } else if (k == "long_thin") {
        if (value < 0 || value > (1 << 20)) return set_error(WOST_ERR_INVALID, "long_thin must be in 0..2^20");
        h->long_thin = (int)value;
    } else if (k == "tail_sort") {
        h->tail_sort = value != 0;
    } else if (k == "dry_stop") {
        if (value != 0 && value != 1) return set_error(WOST_ERR_INVALID, "dry_stop must be 0 or 1");
        h->dry_stop = (int)value;
    } else if (k == "dry_cadence") {
        const int v = (int)value;
        if (value != v || v < 1 || v > 1024 || (v & (v - 1))) return set_error(WOST_ERR_INVALID, "dry_cadence must be a power of two in 1..1024");
        h->dry_cadence = v;
    } else if (k == "chain_start") {
        if (value != 0 && value != 1) return set_error(WOST_ERR_INVALID, "chain_start must be 0 or 1");
        h->chain_start = (int)value;
    } else if (k == "root_visit") {
        if (value != 0 && value != 1) return set_error(WOST_ERR_INVALID, "root_visit must be 0 or 1");
        h->root_visit = (int)value;
    } else if (k == "resident_blocks") {
        if (value < 0 || value > 65535) return set_error(WOST_ERR_INVALID, "resident_blocks must be in 0..65535 (0 = what the chip holds)");
        h->resident_blocks = (int)value;
    } else if (k == "quad") {
        if (value != -1 && value != 0 && value != 1) return set_error(WOST_ERR_INVALID, "quad must be -1 (auto), 0 or 1");
        h->quad = (int)value;
    } else if (k == "quad_fill") {
        if (!(value > 0) || value > 64) return set_error(WOST_ERR_INVALID, "quad_fill must be in (0, 64]");
        h->quad_fill = value;
    } else if (k == "coop") {
        h->coop = value != 0;
    } else if (k == "pool_cap") {
        if (value != 0 && (value < 96 || value > 2048)) return set_error(WOST_ERR_INVALID, "pool_cap must be 0 (automatic) or in 96..2048");
        h->pool_cap = (int)value;
    } else if (k == "ray_slot_trigger") {
        if (value < 1 || value > 64) return set_error(WOST_ERR_INVALID, "ray_slot_trigger must be in 1..64");
        h->ray_slot_trigger = (int)value;
    } else if (k == "thin_waves") {
        h->thin_waves = value != 0;
    } else if (k == "time_kernels") {
        h->time_kernels = value != 0;
    } else if (k == "grad_source") {
        return grad_source_option(value, &h->grad_source);
    } else if (k == "exits_grad_source") {
        return exits_grad_source_option(value, &h->exits_grad_source);
    } else {
        return set_error(WOST_ERR_INVALID, "unknown option: " + k);
    }
    return WOST_OK;
}

}  // extern "C"

// What the launches of a 2-D solve share, fixed by the handle: the block shape, the LDS of a block and how many blocks the chip holds.
struct LaunchGeometry {
    int bs, stack_depth;      // threads per block, entries of a lane stack
    size_t lds, lds_quad;     // the stack columns of a block: one per lane, one per quad (walk_quad_kernel)
    bool emissive, ntree, has_src;
    int32_t coop, pool_cap;   // the wave task pools of a Neumann mesh on the tree (RoundParams) ...
    size_t lds_pools;         // ... and their LDS, behind the stack columns
    size_t lds_round;         // what a walk_round_kernel block asks for
    unsigned blocks_per_cu, resident_threads;
    unsigned resident;        // blocks of a one-launch / persistent launch
};

static LaunchGeometry launch_geometry(const wost_context *c)
{
    LaunchGeometry g{};
    g.bs = c->block_size;
    const int levels_any = std::max(c->dm.view.n_segs > 0 ? c->dm.view.levels : 1, c->nm.view.n_segs > 0 ? c->nm.view.levels : 1);
    // closest point: pushes happen on the inner levels 0..L-1, at most 3 per level, and the
    // branch-free pushes never write beyond entry 3L-1; the Neumann tree queries push up to 4
    // and pop 1 per inner level: 3L+1 entries
    g.stack_depth = 3 * levels_any + 1;
    g.lds = (size_t)g.stack_depth * g.bs * sizeof(uint32_t);
    g.lds_quad = (size_t)g.stack_depth * (g.bs / 4) * sizeof(uint32_t);
    g.emissive = c->nm.view.n_segs > 0 && c->nm.view.emissive;
    g.ntree = c->nm.view.n_segs > WOST_FLAT_MAX;
    g.has_src = c->src.rgb != nullptr;
    // a Neumann mesh on the tree: the task pools of every wave behind the stack columns (wost_coop.h)
    g.coop = (g.ntree && c->coop && c->nm.view.levels <= 11) ? 1 : 0;
    g.pool_cap = c->pool_cap > 0 ? c->pool_cap : std::min(1024, std::max(384, 128 * c->nm.view.levels));
    auto pools_bytes = [&](int cap) { return (size_t)(g.bs / 64) * (2 * (size_t)cap + kPoolOwnerWords) * sizeof(uint32_t) + 8; };
    // (the automatic size gives way to the stack columns of a deep Dirichlet tree; with no room at all: one descent per lane)
    while (c->pool_cap <= 0 && g.pool_cap > 256 && g.lds + pools_bytes(g.pool_cap) > 64 * 1024) g.pool_cap -= 64;
    g.lds_pools = g.coop ? pools_bytes(g.pool_cap) : 0;
    if (g.lds + g.lds_pools > 64 * 1024) { g.coop = 0; g.lds_pools = 0; }
    // developer experiment: extra LDS per block lowers the number of resident blocks (occupancy sensitivity)
    g.lds_round = g.lds + g.lds_pools + (getenv("WOST_EXP_LDS_PAD") ? (size_t)atoi(getenv("WOST_EXP_LDS_PAD")) : 0);
    // blocks a CU holds: the register bound of the instantiation (launch bounds: 6 waves per SIMD, 4 with the tree queries), and
    // no more than fit its 160 KB of LDS -- with the wave task pools a block asks for about 64 KB (two per CU, not four)
    const unsigned blocks_by_regs = (unsigned)((g.ntree ? 4 : 6) * 4 * 64 / g.bs);
    const unsigned blocks_by_lds = (unsigned)std::max<size_t>(1, (size_t)160 * 1024 / std::max<size_t>(g.lds_round, 1));
    g.blocks_per_cu = std::max(1u, std::min(blocks_by_regs, blocks_by_lds));
    g.resident_threads = (unsigned)c->n_cus * g.blocks_per_cu * (unsigned)g.bs;
    g.resident = (unsigned)c->n_cus * g.blocks_per_cu;
    if (c->resident_blocks > 0) g.resident = std::min((unsigned)c->resident_blocks, g.resident);
    return g;
}

// The step scheduling of a walk launch.  A trav_burst / wait_weight set with wost_set_option holds for every launch; the
// automatic ones (0) are
//   the persistent launch:  trav_burst 5,              wait_weight ntree ? 1 : 6
//   every other launch:     trav_burst ntree ? 3 : 5,  wait_weight ntree ? 1 : 8
// Bursts of five: round 6, + 1-2 % in rounds and shards as well as in the persistent launch (profiles/r06_v_*); there every lane
// holds a live walker throughout, and an earlier step trip pays too (config 2 222 -> 217 ms, config 3 327 -> 317,
// profiles/r06_i_burst_variants.txt).  A step that answers its Neumann queries on the tree is long and divergent: served when
// eight ninths of the busy lanes wait (tools/probes/bench2d_wiggly.py: 3.87 -> 4.40 x 10^8 walk-steps/s on 3000 segments), and
// its rounds keep the bursts of three that scheduling was tuned with.
static void set_schedule(const wost_context *c, bool ntree, bool persistent, RoundParams &rp)
{
    rp.trav_burst = c->trav_burst > 0 ? c->trav_burst : (ntree && !persistent ? 3 : 5);
    rp.wait_weight = c->wait_weight > 0 ? c->wait_weight : (ntree ? 1 : (persistent ? 6 : 8));
}

// The fields of RoundParams that every launch of a solve shares; a launch copies them and sets its queues, counters and lanes.
static RoundParams base_params(const wost_context *c, const LaunchGeometry &g, float *field_dev, int32_t field_base)
{
    RoundParams rp{};
    rp.dm = c->dm.view; rp.nm = c->nm.view; rp.st = c->dst; rp.probe = c->probe; rp.src = c->src;
    rp.field = field_dev; rp.field_base = field_base; rp.stats = c->stats;
    rp.count_far = c->counts + 2; rp.out_capacity = (uint32_t)c->n_pixels;
    rp.count_long = c->counts + 4; rp.long_steps = c->long_steps > 0 ? (float)c->long_steps : WOST_INF;
    // a slot regenerates its pixel's next sample inside a round, so rounds are long: 256 steps unless the caller chose
    // otherwise (shorter rounds only added launches: 128^2 at 1 spp 0.95 -> 1.39 ms with 8-step rounds)
    rp.steps_per_round = c->steps_per_round > 0 ? c->steps_per_round : 256;
    rp.stack_stride = g.bs;
    rp.chain = c->chain_start;
    rp.root_visit = c->root_visit;
    set_schedule(c, g.ntree, false, rp);
    rp.coop = g.coop; rp.pool_cap = g.pool_cap; rp.pool_offset = (int32_t)(g.lds / sizeof(uint32_t)); rp.ray_slot_trigger = c->ray_slot_trigger;
    return rp;
}

// The walk kernel of a launch (kind WOST_LAUNCH_ROUND / QUAD / ONE / PERSISTENT): the scene's flags become its template
// arguments E(missive), T(ree), S(ource).  These are all the instantiations there are:
//   ROUND  walk_round_kernel<E, T, 0, S, slack, 0>    ONE         walk_round_kernel<E, T, 1, 0, 0, 0>  (no source term: launch_ordinary)
//   QUAD   walk_quad_kernel<E, T, S, slack>           PERSISTENT  walk_round_kernel<E, T, 1, S, 0, 1>
// and beside each its carried entry (walk_round_carry_kernel, walk_quad_carry_kernel), which the launches of a continued solve
// take (rp.carry_rng != nullptr).
static void launch_walk(const LaunchGeometry &g, int kind, bool slack, unsigned grid, hipStream_t stream, const RoundParams &rp)
{
    auto launch = [&](auto E, auto T, auto S) {
        constexpr bool e = decltype(E)::value, t = decltype(T)::value, s = decltype(S)::value;
        if (rp.carry_rng) {
            if (kind == WOST_LAUNCH_QUAD && slack) hipLaunchKernelGGL((walk_quad_carry_kernel<e, t, s, true>), dim3(grid), dim3(g.bs), g.lds_quad, stream, rp);
            else if (kind == WOST_LAUNCH_QUAD) hipLaunchKernelGGL((walk_quad_carry_kernel<e, t, s, false>), dim3(grid), dim3(g.bs), g.lds_quad, stream, rp);
            else if (kind == WOST_LAUNCH_PERSISTENT) hipLaunchKernelGGL((walk_round_carry_kernel<e, t, true, s, false, true>), dim3(grid), dim3(g.bs), g.lds_round, stream, rp);
            else if (kind == WOST_LAUNCH_ONE) hipLaunchKernelGGL((walk_round_carry_kernel<e, t, true, false, false, false>), dim3(grid), dim3(g.bs), g.lds_round, stream, rp);
            else if (slack) hipLaunchKernelGGL((walk_round_carry_kernel<e, t, false, s, true, false>), dim3(grid), dim3(g.bs), g.lds_round, stream, rp);
            else hipLaunchKernelGGL((walk_round_carry_kernel<e, t, false, s, false, false>), dim3(grid), dim3(g.bs), g.lds_round, stream, rp);
        } else if (kind == WOST_LAUNCH_QUAD && slack) hipLaunchKernelGGL((walk_quad_kernel<e, t, s, true>), dim3(grid), dim3(g.bs), g.lds_quad, stream, rp);
        else if (kind == WOST_LAUNCH_QUAD) hipLaunchKernelGGL((walk_quad_kernel<e, t, s, false>), dim3(grid), dim3(g.bs), g.lds_quad, stream, rp);
        else if (kind == WOST_LAUNCH_PERSISTENT) hipLaunchKernelGGL((walk_round_kernel<e, t, true, s, false, true>), dim3(grid), dim3(g.bs), g.lds_round, stream, rp);
        else if (kind == WOST_LAUNCH_ONE) hipLaunchKernelGGL((walk_round_kernel<e, t, true, false, false, false>), dim3(grid), dim3(g.bs), g.lds_round, stream, rp);
        else if (slack) hipLaunchKernelGGL((walk_round_kernel<e, t, false, s, true, false>), dim3(grid), dim3(g.bs), g.lds_round, stream, rp);
        else hipLaunchKernelGGL((walk_round_kernel<e, t, false, s, false, false>), dim3(grid), dim3(g.bs), g.lds_round, stream, rp);
    };
    auto with_src = [&](auto E, auto T) { g.has_src ? launch(E, T, std::true_type{}) : launch(E, T, std::false_type{}); };
    auto with_tree = [&](auto E) { g.ntree ? with_src(E, std::true_type{}) : with_src(E, std::false_type{}); };
    g.emissive ? with_tree(std::true_type{}) : with_tree(std::false_type{});
}

// Synchronises a side stream when it goes out of scope, if armed: run_solve arms one once it has queued a launch there, so that
// no return -- an early one on an error included -- leaves that launch reading the queues and counters the next solve rewrites.
// (The success path orders those launches through far_ev1 / long_ev1 and disarms it.)
struct SideStreamGuard {
    hipStream_t stream = nullptr;
    ~SideStreamGuard() { if (stream) (void)hipStreamSynchronize(stream); }
};

// One pass of run_solve's loop: one ordinary launch on the solve's stream, and what starts beside it on the side streams.
struct Pass {
    int cur;                  // input queue: c->queue[cur]; output queue: c->queue[cur ^ 1]
    uint32_t n_active;        // walkers in the input queue
    uint32_t far;             // strayed walkers at its far end, for the launch on far_stream (0 once they joined the long remainders)
    uint32_t beside_far;      // strayed walkers that joined the long remainders
    uint32_t n_round;         // walkers of the ordinary launch
    int kind;                 // ... its WOST_LAUNCH_*, workgroups and parameters
    unsigned grid;
    RoundParams rp;
};
// walkers a pass started on the side streams (long remainders, strayed walkers), and whether it started anything at all: the
// passes wost_last_launches lists are the passes wost_stats.kernel_launches counts
static uint32_t pass_beside(const Pass &p) { return p.n_active - p.n_round + p.far + p.beside_far; }
static bool pass_launched(const Pass &p) { return p.n_round > 0 || pass_beside(p) > 0; }

// The hand-over after a persistent launch: it left one partly solved pixel per lane, each with an estimate of the walk steps it
// still needs (config 2: 387 000 pixels, 12 % of the solve's steps; half of them need 650 steps more, a few thousand over 1 500),
// and the walkers that strayed beyond the plain visits' range during that launch, parked since with most of their samples
// ahead of them.  In rounds the few long ones add launch after launch of a nearly empty chip (16 of the 52 ms that followed
// the persistent launch), so they start NOW and run to their end -- four lanes to a walker, exact at any distance (SLACK: no
// walker leaves such a launch), the longest a thousand or two four to a wave, the others sixteen -- on long_stream beside the
// rounds of the rest; and the first round takes the rest sorted by estimate: the walkers of a wave finish together and the
// wave leaves, instead of a third of the lanes of every wave idling behind finished pixels.
static int hand_over(wost_context *c, const LaunchGeometry &g, hipStream_t stream, Pass &p, SideStreamGuard &long_guard)
{
    const bool beside = c->long_steps > 0;
    const uint32_t n_far = (beside && p.far <= 1024u && p.far <= (uint32_t)c->long_cap) ? p.far : 0u;
    const uint32_t n_long = beside ? std::min<uint32_t>(std::min<uint32_t>(c->host_count[4], (uint32_t)c->long_cap - n_far), p.n_active) : 0u;
    const uint32_t *ord = nullptr;
    if (p.n_active > 0 && (n_long > 0 || c->tail_sort)) {
        if (c->order.cap < c->n_pixels) WOST_TRY((hipError_t)order_alloc(c->order, c->n_pixels));
        WOST_TRY((hipError_t)order_by_estimate(c->order, c->queue[p.cur].est, p.n_active, stream, &ord));
        p.rp.order = ord + n_long;
    }
    const uint32_t n_beside = n_far + n_long;
    if (n_beside == 0) return WOST_OK;
    if (!c->long_mem) {
        WOST_TRY(hipMalloc(&c->long_mem, queue_bytes((size_t)c->long_cap)));
        carve_queue(c->long_mem, (size_t)c->long_cap, c->long_queue);
    }
    // the strayed first (most of a pixel ahead of them as a rule), then the long remainders, longest first
    if (n_far > 0) {
        hipLaunchKernelGGL(gather_walkers_kernel, dim3((n_far + 255) / 256), dim3(256), 0, stream, queue_from(c->queue[p.cur], c->n_pixels - n_far),
                           (const uint32_t *)nullptr, n_far, c->long_queue);
        WOST_TRY(hipGetLastError());
        p.far = 0; p.beside_far = n_far;
    }
    if (n_long > 0) {
        hipLaunchKernelGGL(gather_walkers_kernel, dim3((n_long + 255) / 256), dim3(256), 0, stream, c->queue[p.cur], ord, n_long, queue_from(c->long_queue, n_far));
        WOST_TRY(hipGetLastError());
    }
    const uint32_t n_thin = std::min<uint32_t>(n_beside, (uint32_t)std::max(c->long_thin, 0));
    c->host_count[5] = n_beside;
    c->host_count[6] = p.n_active - n_long;
    WOST_TRY(hipMemcpyAsync(c->counts + 5, c->host_count + 5, 2 * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    WOST_TRY(hipEventRecord(c->long_ev0, stream));
    WOST_TRY(hipStreamWaitEvent(c->long_stream, c->long_ev0, 0));
    RoundParams lp = p.rp;
    lp.in = c->long_queue; lp.order = nullptr; lp.count_in = c->counts + 5;
    lp.count_out = lp.count_far = c->counts + 8;       // (nothing comes out: every walker runs to the end of its pixel)
    lp.steps_per_round = 0x7fffffff; lp.stack_stride = g.stack_depth; lp.lane_shift = 0;
    const uint32_t quads_per_block = (uint32_t)g.bs / 4u;
    lp.thin_count = n_thin;
    lp.thin_blocks = (n_thin * 4u + quads_per_block - 1u) / quads_per_block;
    const unsigned lgrid = lp.thin_blocks + (n_beside - n_thin + quads_per_block - 1u) / quads_per_block;
    long_guard.stream = c->long_stream;
    launch_walk(g, WOST_LAUNCH_QUAD, true, lgrid, c->long_stream, lp);
    WOST_TRY(hipGetLastError());
    WOST_TRY(hipEventRecord(c->long_ev1, c->long_stream));
    p.rp.count_in = c->counts + 6;
    p.n_round = p.n_active - n_long;
    return WOST_OK;
}

// Walkers that left the previous launch at a query beyond the plain kernel's range wait at the far end of its output queue,
// which is this launch's input queue.  The SLACK instantiation takes them through max_depth steps -- the walk that strayed
// ends within that many -- on far_stream, next to this launch, and appends them to the same output queue (both kernels only
// read the input queue and claim output slots from one counter).
static int launch_strayed(wost_context *c, const LaunchGeometry &g, hipStream_t stream, const Pass &p, SideStreamGuard &far_guard)
{
    c->host_count[3] = p.far;
    WOST_TRY(hipMemcpyAsync(c->counts + 3, c->host_count + 3, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    WOST_TRY(hipEventRecord(c->far_ev0, stream));                      // the counters are ready
    WOST_TRY(hipStreamWaitEvent(c->far_stream, c->far_ev0, 0));
    RoundParams fp = p.rp;
    fp.order = nullptr; fp.in = queue_from(c->queue[p.cur], c->n_pixels - p.far); fp.count_in = c->counts + 3;
    fp.steps_per_round = std::max(1, c->settings.max_depth);
    // a few strayed walkers (leaks of a closed scene): one per wave -- a query from very far away is a scan of the whole
    // mesh by the 64 lanes (closest_point_wave), and the launch lasts as long as its slowest wave; many (an open scene:
    // every walk that misses the boundary strays): every lane loaded
    fp.lane_shift = p.far <= 4096u ? 6 : 0;
    far_guard.stream = c->far_stream;
    launch_walk(g, WOST_LAUNCH_ROUND, true, (unsigned)((((uint64_t)p.far << fp.lane_shift) + g.bs - 1) / g.bs), c->far_stream, fp);
    WOST_TRY(hipGetLastError());
    WOST_TRY(hipEventRecord(c->far_ev1, c->far_stream));
    // (not a launch of its own in `launches`: kernel_launches counts passes, and a pass is counted once whatever it started)
    return WOST_OK;
}

// The ordinary launch of a pass, on the solve's stream: its kind, lanes and grid.  The first launch of a solve may drain the
// queue in ONE launch (few samples per pixel) or be PERSISTENT (many); the others are QUAD (under-filled) or ROUND.
static int launch_ordinary(wost_context *c, const LaunchGeometry &g, hipStream_t stream, bool first, Pass &p)
{
    RoundParams &rp = p.rp;
    const int bs = g.bs;
    // When the walkers left fill less than 1/16 of the resident threads, spread them out: the duration of such a launch is the
    // latency of its slowest wave, and a wave is as slow as the longest query among its walkers (config 2's last three
    // launches: 13.1 -> 8.9 ms; with 2 or 4 lanes per walker the extra waves cost more than they save: 9.2 -> 11.8 ms).
    rp.lane_shift = 0;
    if (c->thin_waves) {
        while (rp.lane_shift < 6 && ((uint64_t)p.n_round << (rp.lane_shift + 1)) <= g.resident_threads) ++rp.lane_shift;
        if (rp.lane_shift < 4) rp.lane_shift = 0;
    }
    p.grid = (unsigned)((((uint64_t)p.n_round << rp.lane_shift) + bs - 1) / bs);
    // REFILL launch: as many resident threads as the chip holds, each draining the input queue.  Worth it when regeneration
    // cannot keep the lanes busy (measured on config 2's frame: 1 spp 3.5 -> 3.0 ms, 4 spp 8.3 -> 7.9 ms, 8 spp 13.0 -> 13.5 ms)
    // and the queue is larger than one residency; the 16-bit lane counters bound spp * max_depth.
    // (the one-launch form of few samples has no instantiation with a source term; the persistent launch has)
    // (the samples of this solve: rp.st.spp -- the handle's setting, or the count of a continued call)
    const int32_t spp = rp.st.spp;
    const bool can_persist = (int64_t)spp * c->settings.max_depth < 65535 && first;
    const bool can_refill = can_persist && !g.has_src;
    // (the automatic choice of the one-launch form gives way to a persistent launch the caller asked for: persist 1)
    const bool few = can_refill && (c->refill == 1 || (c->refill == -1 && c->persist != 1 && spp <= 4 && p.grid > g.resident));
    // PERSISTENT first launch (many samples per pixel, more walkers than resident lanes): the same resident threads, but the
    // lanes take whole pixels -- all of a pixel's samples, the pixels in the order of wost_order.h, longest expected chain first
    // -- until the input queue is dry; then every wave hands what it holds to the output queue and the rest of the solve runs
    // in rounds.  No lane idles behind a finished pixel and no launch ends while pixels are unread (in rounds, config 2 spent
    // 108 of its 252 ms in launches where a third of the lanes had finished their pixel, EXPERIMENTS 25); what the rounds
    // get is the remainder of one pixel per lane.
    const bool persist = can_persist && !few && c->refill != 1 &&
                         (c->persist == 1 || (c->persist == -1 && spp > 4 && p.n_active > g.resident_threads));
    if (few || persist) {
        p.kind = persist ? WOST_LAUNCH_PERSISTENT : WOST_LAUNCH_ONE;
        rp.lane_shift = 0;
        p.grid = std::min((unsigned)((p.n_active + bs - 1) / bs), g.resident);
        c->host_count[1] = p.grid * (unsigned)bs;      // first unread slot (pinned staging word)
        WOST_TRY(hipMemcpyAsync(c->cursor, c->host_count + 1, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        rp.cursor = c->cursor;
        rp.steps_per_round = 0x7fffffff;
        rp.reserve = persist ? 0 : 64;
        rp.leave_dry = persist ? (c->dry_stop ? 2 : 1) : 0;
        rp.dry_cadence = c->dry_cadence;
        // How long R unread slots last at least: a pixel takes spp walk steps or more, so the resident lanes claim at most
        // lanes / spp slots per walk step of a lane.  R >> dry_shift steps with 2^dry_shift >= lanes / spp end before the queue is
        // dry, and the bound is pessimistic (config 2: 1 536 slots per trip possible, 220 taken).
        rp.dry_shift = 0;
        while (rp.dry_shift < 31 && ((uint64_t)std::max(spp, 1) << rp.dry_shift) < (uint64_t)p.grid * (unsigned)bs) ++rp.dry_shift;
        if (persist) set_schedule(c, g.ntree, true, rp);
        if (persist ? c->persist_order : c->few_order) {
            if (c->order.cap < c->n_pixels) WOST_TRY((hipError_t)order_alloc(c->order, c->n_pixels));
            WOST_TRY((hipError_t)order_by_distance(c->order, c->queue[p.cur].d0_d2, p.n_active, stream, &rp.order));
        }
    } else if (p.n_round > 0 &&
               (c->quad == 1 || (c->quad == -1 && 4.0 * (double)p.n_round <= c->quad_fill * (double)g.resident_threads))) {
        // Under-filled launch: four lanes per walker (walk_quad_kernel).  Such a launch lasts as long as its longest chain of
        // dependent node visits; sharing a descent between the lanes of a quad halves that chain.
        // Few walkers: fewer quads per wave (16 -> 4 -> 1), as long as the waves still fit the chip.
        p.kind = WOST_LAUNCH_QUAD;
        rp.lane_shift = 0;
        while (rp.lane_shift < 4 && ((uint64_t)p.n_round << (2 + rp.lane_shift + 2)) <= g.resident_threads) rp.lane_shift += 2;
        rp.stack_stride = g.stack_depth;      // entries per (contiguous) quad column
        p.grid = (unsigned)((((uint64_t)p.n_round << (2 + rp.lane_shift)) + bs - 1) / bs);
    } else {
        p.kind = WOST_LAUNCH_ROUND;
    }
    // (the last strayed walkers can outlive the ordinary queue: then only their launch runs)
    if (p.n_round > 0) {
        launch_walk(g, p.kind, false, p.grid, stream, rp);
        WOST_TRY(hipGetLastError());
    }
    return WOST_OK;
}

// The end of a pass: the solve's stream waits for the strayed walkers' launch, the counts (with time_kernels also the
// counters) come back, and the pass is recorded for wost_last_launches.
static int finish_pass(wost_context *c, hipStream_t stream, const Pass &p, uint32_t launches, double &kernel_ms)
{
    if (p.far > 0) WOST_TRY(hipStreamWaitEvent(stream, c->far_ev1, 0));
    if (c->time_kernels) WOST_TRY(hipEventRecord(c->ev1, stream));
    WOST_TRY(hipMemcpyAsync(c->host_count, c->counts + (p.cur ^ 1), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipMemcpyAsync(c->host_count + 2, c->counts + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    const bool persist = p.kind == WOST_LAUNCH_PERSISTENT;
    if (persist) WOST_TRY(hipMemcpyAsync(c->host_count + 4, c->counts + 4, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (c->time_kernels) WOST_TRY(hipMemcpyAsync(c->host_stats, c->stats, kStatCopies * sizeof(StatsDev), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipStreamSynchronize(stream));
    if (!c->time_kernels) return WOST_OK;
    float ms = 0.0f;
    WOST_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    kernel_ms += ms;
    if (!pass_launched(p)) return WOST_OK;
    // (a pass whose walkers all went to the side streams has no ordinary launch: WOST_LAUNCH_BESIDE)
    wost_launch_info li{p.n_round > 0 ? p.kind : (int)WOST_LAUNCH_BESIDE, p.n_round, pass_beside(p), p.n_round > 0 ? p.grid : 0u, ms, 0};
    li.walk_steps_done = c->steps_before;
    for (int k = 0; k < kStatCopies; ++k) li.walk_steps_done += c->host_stats[k].steps;
    c->last_launches.push_back(li);
    if (getenv("WOST_TRACE_LAUNCHES")) fprintf(stderr, "launch %d: walkers %u of %u (+ %u strayed) grid %u %.3f ms -> %u left, %u strayed%s\n", launches, p.n_round, p.n_active, p.far, p.grid, ms, c->host_count[0], c->host_count[2], persist ? " (persistent)" : "");
    return WOST_OK;
}

// The first step of a solve, the one that fills queue 0: the frame init on a pixel range and a shard, or (points != nullptr) the
// point init on points [first, first + n) of a call -- one chunk of a point solve, at most n_pixels points.
// A frame step with carry_more > 0 is a call of a continued solve (wost_solve_more & co.): carry_more samples on top of those in
// the handle's carried buffers -- the solve runs with spp = carry_more, whatever the handle's own setting -- on the pixels of the
// device map carry_select (nullptr: every pixel).  carry_append: not the first walk of its call, it appends to last_launches.
// A point step with carry_more > 0 is the same on a chunk of the handle's carried point list (wost_points_more & co.): the
// buffers are the list's, the map is indexed by the point's index in the list.
// spp > 0: the samples of a step that carries nothing, whatever the handle's setting (the walks of a gradient call: one each).
struct FirstStep {
    int32_t pixel_begin, pixel_end, shard_index, shard_count;
    const float *points;
    int32_t first, n, seed_base, seed_width;
    int32_t carry_done, carry_more;
    const uint8_t *carry_select;
    bool carry_append;
    int32_t spp = 0;
};
static FirstStep frame_step(int32_t pixel_begin, int32_t pixel_end, int32_t shard_index, int32_t shard_count, int32_t carry_done = 0,
                            int32_t carry_more = 0, const uint8_t *carry_select = nullptr, bool carry_append = false)
{
    return FirstStep{pixel_begin, pixel_end, shard_index, shard_count, nullptr, 0, 0, 0, 0, carry_done, carry_more, carry_select, carry_append};
}

// the shared solve driver: field_dev indexed by (pix - field_base)
// (a later chunk of a point solve, fs.first > 0, appends to last_launches, its walk_steps_done counted on from c->steps_before)
static int run_solve(wost_context *c, const FirstStep &fs, float *field_dev, int32_t field_base, hipStream_t stream, wost_stats *stats)
{
    const auto t_start = std::chrono::high_resolution_clock::now();
    WOST_TRY(hipSetDevice(c->device));
    const LaunchGeometry g = launch_geometry(c);
    WOST_TRY(hipMemsetAsync(c->counts, 0, 12 * sizeof(uint32_t), stream));
    WOST_TRY(hipMemsetAsync(c->stats, 0, kStatCopies * sizeof(StatsDev), stream));
    // the plan of the solve takes its sample count from here: the handle's setting, or the count of a continued call
    const bool carried = fs.carry_more > 0;
    const CarryState &cs = fs.points ? c->list.carry : c->carry;
    DevSettings st = c->dst;
    if (carried) st.spp = fs.carry_more;
    else if (fs.spp > 0) st.spp = fs.spp;

    if (fs.points) {
        const InitPointsParams ip{c->dm.view, st, c->queue[0], c->counts + 0, fs.points, field_dev, fs.first, fs.n, fs.seed_base, fs.seed_width, g.bs,
                                  cs.rng, cs.sum, carried ? cs.n : nullptr, carried ? fs.carry_select : nullptr};
        hipLaunchKernelGGL(init_points_kernel, dim3((unsigned)(((long long)fs.n + g.bs - 1) / g.bs)), dim3(g.bs), g.lds, stream, ip);
    } else {
        const int tiles_x = (c->settings.width + 7) / 8, tiles_y = (c->settings.height + 7) / 8;
        const InitParams ip{c->dm.view, st, c->probe, c->queue[0], c->counts + 0, c->mask, field_dev, field_base,
                            fs.pixel_begin, fs.pixel_end, fs.shard_index, fs.shard_count, tiles_x, tiles_y, g.bs,
                            c->carry.rng, c->carry.sum, carried ? c->carry.n : nullptr, carried ? fs.carry_select : nullptr};
        const long long n_threads = (long long)tiles_x * tiles_y * 64;
        const unsigned init_grid = (unsigned)((n_threads + g.bs - 1) / g.bs);
        hipLaunchKernelGGL(init_kernel, dim3(init_grid), dim3(g.bs), g.lds, stream, ip);
    }
    WOST_TRY(hipGetLastError());
    WOST_TRY(hipMemcpyAsync(c->host_count, c->counts, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipStreamSynchronize(stream));
    uint32_t n_active = c->host_count[0];

    double kernel_ms = 0.0;
    uint32_t launches = 0;
    int cur = 0;
    const bool later_chunk = (fs.points && fs.first > 0) || (carried && fs.carry_append);
    if (!later_chunk) {
        c->last_launches.clear();
        c->steps_before = 0;
    }
    RoundParams base = base_params(c, g, field_dev, field_base);
    base.st = st;
    if (carried) {
        base.carry_rng = cs.rng; base.carry_sum = cs.sum; base.carry_total = fs.carry_done + fs.carry_more;
    }
    SideStreamGuard long_guard, far_guard;   // armed: a launch of the long remainders / of strayed walkers was queued
    uint32_t pending_far = 0;     // walkers at the far end of queue[cur] that the previous launch could not serve (launch_strayed)
    bool handed_over = false;     // the previous launch was persistent: queue[cur] holds what it handed over, with estimates
    while (n_active > 0 || pending_far > 0) {
        const int nxt = cur ^ 1;
        WOST_TRY(hipMemsetAsync(c->counts + nxt, 0, sizeof(uint32_t), stream));
        WOST_TRY(hipMemsetAsync(c->counts + 2, 0, sizeof(uint32_t), stream));
        Pass p{};
        p.cur = cur; p.n_active = p.n_round = n_active; p.far = pending_far;
        p.rp = base;
        p.rp.in = c->queue[cur]; p.rp.out = c->queue[nxt]; p.rp.count_in = c->counts + cur; p.rp.count_out = c->counts + nxt;
        if (c->time_kernels) WOST_TRY(hipEventRecord(c->ev0, stream));
        int rc = handed_over ? hand_over(c, g, stream, p, long_guard) : WOST_OK;
        if (rc == WOST_OK && p.far > 0) rc = launch_strayed(c, g, stream, p, far_guard);
        if (rc == WOST_OK) rc = launch_ordinary(c, g, stream, launches == 0, p);
        if (rc == WOST_OK) rc = finish_pass(c, stream, p, launches, kernel_ms);
        if (rc != WOST_OK) return rc;
        handed_over = p.kind == WOST_LAUNCH_PERSISTENT;
        if (pass_launched(p)) ++launches;
        pending_far = c->host_count[2];
        n_active = c->host_count[0];
        cur = nxt;
    }
    if (long_guard.stream) {
        // the long remainders may outlast the rounds: what is left of their launch counts as kernel time of the solve
        if (c->time_kernels) WOST_TRY(hipEventRecord(c->ev0, stream));
        WOST_TRY(hipStreamWaitEvent(stream, c->long_ev1, 0));
        if (c->time_kernels) {
            WOST_TRY(hipEventRecord(c->ev1, stream));
            WOST_TRY(hipStreamSynchronize(stream));
            float ms = 0.0f;
            WOST_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
            kernel_ms += ms;
            c->last_launches.push_back(wost_launch_info{WOST_LAUNCH_WAIT, 0, 0, 0, ms, 0});
            if (getenv("WOST_TRACE_LAUNCHES")) fprintf(stderr, "waited %.3f ms for the launch of the long remainders\n", ms);
        }
    }
    std::vector<StatsDev> copies(kStatCopies);
    WOST_TRY(hipMemcpyAsync(copies.data(), c->stats, kStatCopies * sizeof(StatsDev), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipStreamSynchronize(stream));
    // the solve's stream has waited for every side launch (far_ev1, long_ev1): nothing is left running
    long_guard.stream = far_guard.stream = nullptr;
    StatsDev sd{};
    for (const StatsDev &k : copies) {
        sd.steps += k.steps; sd.started += k.started; sd.absorbed += k.absorbed; sd.truncated += k.truncated;
        sd.nhits += k.nhits; sd.inner_visits += k.inner_visits; sd.leaf_visits += k.leaf_visits;
        sd.trav_trips += k.trav_trips; sd.step_trips += k.step_trips;
        sd.max_stack = std::max(sd.max_stack, k.max_stack);
        sd.sp_ge6 += k.sp_ge6; sd.sp_ge10 += k.sp_ge10; sd.sp_ge14 += k.sp_ge14;
    }
#ifdef WOST_DRAIN
    {
        // the drain of the persistent launch, on the 100 MHz clock of wall_clock64(): when the waves stopped on the dry queue,
        // counted from the first that did, and when the last wave reached the end of the kernel
        unsigned long long t0 = ~0ull, t1 = 0, n = 0, t_end = 0;
        for (const StatsDev &k : copies) {
            if (k.stop_waves) t0 = std::min(t0, ~k.stop_min);
            t1 = std::max(t1, k.stop_max); n += k.stop_waves; t_end = std::max(t_end, k.end_max);
        }
        double sum = 0.0;
        for (const StatsDev &k : copies) sum += (double)(k.stop_sum - k.stop_waves * t0);
        if (n) fprintf(stderr, "WOST_DRAIN: %llu waves stopped on the dry queue; after the first: mean %.3f ms, last %.3f ms, end of the kernel %.3f ms\n", n,
                       sum / (double)n * 1e-5, (double)(t1 - t0) * 1e-5, (double)(t_end - t0) * 1e-5);
    }
#endif
#ifdef WOST_TRACK
    fprintf(stderr, "WOST_TRACK: visits %llu leaf %llu max_stack %llu visits leaving >=6 / >=10 / >=14 entries: %llu / %llu / %llu\n", sd.inner_visits,
            sd.leaf_visits, sd.max_stack, sd.sp_ge6, sd.sp_ge10, sd.sp_ge14);
#endif
    if (stats) {
        const auto t_end = std::chrono::high_resolution_clock::now();
        stats->walk_steps = sd.steps;
        stats->walks_started = sd.started;
        stats->walks_absorbed = sd.absorbed;
        stats->walks_truncated = sd.truncated;
        stats->neumann_hits = sd.nhits;
        stats->inner_visits = sd.inner_visits;
        stats->leaf_visits = sd.leaf_visits;
        stats->trav_trips = sd.trav_trips;
        stats->step_trips = sd.step_trips;
        stats->reserved = (uint32_t)sd.max_stack;
        stats->kernel_ms = kernel_ms;
        stats->kernel_launches = launches;
        stats->solve_ms = std::chrono::duration<double, std::milli>(t_end - t_start).count();
    }
    return WOST_OK;
}

// ---- the frame and point solves (the bodies of the entry points: UniformCalls, wost_uniform.h) ----
static int frame_solve(wost_context *c, int32_t pixel_begin, int32_t pixel_end, int32_t shard_index, int32_t shard_count, float *field_dev,
                       int32_t field_base, hipStream_t stream, wost_stats *stats)
{
    return run_solve(c, frame_step(pixel_begin, pixel_end, shard_index, shard_count), field_dev, field_base, stream, stats);
}

// A point list of n points in chunks of at most n_pixels points -- what the handle's queues, order buffers and out_capacity hold --
// each a pass of the driver on `fs` with its first and n set; a walker's pix is its point's index in the list, so every chunk
// writes the one field.  The stats are the sum of the chunks.  steps_before, the walk steps of the earlier chunks: a point solve
// sets it, a call on the carried list (fs.carry_more > 0), whose second walk counts on from its first, adds to it and appends
// to last_launches from its second chunk on.
static int solve_point_chunks(wost_context *c, FirstStep fs, int32_t n, float *field_dev, hipStream_t stream, wost_stats *stats)
{
    const auto t0 = HostClock::now();
    wost_stats total{};
    const int32_t cap = (int32_t)std::min<size_t>(c->n_pixels, (size_t)1 << 28);
    for (fs.first = 0; fs.first < n; fs.first += cap) {
        fs.n = std::min(cap, n - fs.first);
        wost_stats st{};
        const int rc = run_solve(c, fs, field_dev, 0, stream, &st);
        if (rc != WOST_OK) return rc;
        add_stats(total, st);
        if (fs.carry_more > 0) {
            c->steps_before += st.walk_steps;
            fs.carry_append = true;
        } else {
            c->steps_before = total.walk_steps;
        }
    }
    stamp_solve_ms(&total, t0);
    if (stats) *stats = total;
    return WOST_OK;
}

static int point_solve(wost_context *c, const float *pts_dev, int32_t n, int32_t seed_base, int32_t seed_width, float *field_dev, hipStream_t stream,
                       wost_stats *stats)
{
    return solve_point_chunks(c, FirstStep{0, 0, 0, 1, pts_dev, 0, 0, seed_base, seed_width, 0, 0, nullptr, false}, n, field_dev, stream, stats);
}

static const UniformCalls<wost_context> kUniform{2, frame_solve, point_solve};

// ---- the continued frame solve (the drivers: wost_carry.hip; the bodies of the entry points: CarryCalls, wost_carry.h) ----
// a walk of the carried solve: a pass of the solve driver on the selected pixels (the 2-D walkers are queued by init_kernel from
// the map; the id list is the 3-D lanes')
static CarryWalk carry_walk(wost_context *c, int32_t shard_index, int32_t shard_count)
{
    return [c, shard_index, shard_count](int32_t more_spp, const uint8_t *sel, const int32_t *, uint32_t, float *field_dev, hipStream_t stream,
                                         wost_stats *stats) {
        const bool append = c->carry.walks > 0;
        if (!append) c->steps_before = 0;
        const int rc = run_solve(c, frame_step(0, (int32_t)c->n_pixels, shard_index, shard_count, c->carry.done, more_spp, sel, append), field_dev, 0,
                                 stream, stats);
        if (rc == WOST_OK && stats) c->steps_before += stats->walk_steps;
        return rc;
    };
}

// (a call that made no walk launched nothing: wost_last_launches reports an empty list, not the solve before it)
static const CarryCalls<wost_context> kCarry{"wost_", carry_walk, [](wost_context *c) { c->last_launches.clear(); }};

// ---- the carried point list (wost_points_carry & co.; the bodies of the entry points: PointCalls, wost_carry.h) ----
// A walk of the list: chunks of at most n_pixels points by index range, as the point solve cuts them -- each a pass of the solve
// driver on the chunk's selected points.  A chunk in which nothing is selected queues no walker and launches no walk.
static CarryWalk points_walk(PointListCtx<wost_context> *x, int32_t, int32_t)
{
    wost_context *c = x->h;
    return [c](int32_t more_spp, const uint8_t *sel, const int32_t *, uint32_t, float *field_dev, hipStream_t stream, wost_stats *stats) {
        const PointList &l = c->list;
        const bool append = l.carry.walks > 0;
        if (!append) c->steps_before = 0;
        return solve_point_chunks(c, FirstStep{0, 0, 0, 1, l.pts, 0, 0, l.seed_base, l.seed_width, l.carry.done, more_spp, sel, append}, l.n, field_dev,
                                  stream, stats);
    };
}

static const PointCalls<wost_context> kPoints{{"wost_points_", points_walk, [](PointListCtx<wost_context> *x) { x->h->last_launches.clear(); }}, 2};

// ---- the gradient at the caller's points (the driver and its kernels: wost_grad.hip; the body of the entry points: grad_entry) ----
// what the 2-D context adds: the kernel in front on its meshes, a point step of one sample per walk on the handle's queues, and
// the in-ball kernel on its source grid
static GradCall grad_call(wost_context *c)
{
    GradCall g{"wost_", 2, c->device, c->dst.spp, c->n_pixels, c->dst.eps, c->src.rgb != nullptr, c->grad_source, c->stream, &c->grad, nullptr, nullptr,
               nullptr};
    g.prep = [c](const GradPrep &p, hipStream_t stream) { return grad_prep2(c->dm.view, c->nm.view, p, stream); };
    g.walk = [c](const float *first_pts, int32_t n_walks, int32_t seed_base, int32_t seed_width, float *w_rgb, hipStream_t stream, wost_stats *stats) {
        const FirstStep fs{0, 0, 0, 1, first_pts, 0, n_walks, seed_base, seed_width, 0, 0, nullptr, false, 1};
        return run_solve(c, fs, w_rgb, 0, stream, stats);
    };
    g.ball = [c](const GradBall &p, hipStream_t stream) { return grad_ball2(c->src, p, stream); };
    return g;
}

// ---- the carried gradient list (wost_gradient_points_carry & co.; the bodies of the entry points: GradListCalls, wost_grad.h) ----
static const GradListCalls<wost_context> kGradList{grad_call, 2};

// ---- the launches of the batch queries (their bodies: query_*, wost_uniform.h).  The closest-point and the distance kernel
// take the stride of the stack columns; render_sdf renders into the handle's field buffer (n_pixels floats fit) and tells its
// kernel which mesh it is ----
namespace {
struct Query2 {
    static constexpr int dim = 2, uv = 1, bs = 256;
    static int32_t count(const DevMesh &m) { return m.n_segs; }
    static dim3 grid(int n) { return dim3((n + bs - 1) / bs); }
    static void closest_point(wost_context *h, const DevMesh &m, size_t lds, const float *pts, int n, int32_t *idx, float *dist, float *uv, int32_t *side)
    {
        hipLaunchKernelGGL(closest_point_kernel, grid(n), dim3(bs), lds, h->stream, m, pts, n, idx, dist, uv, side, bs);
    }
    static void silhouette(wost_context *h, const DevMesh &m, size_t lds, const float *pts, const float *rmax, int n, float *out)
    {
        hipLaunchKernelGGL(silhouette_kernel, grid(n), dim3(bs), lds, h->stream, m, pts, rmax, n, out);
    }
    static void ray(wost_context *h, const DevMesh &m, size_t lds, const float *o, const float *d, const float *tmax, int n, int32_t *hit, float *t,
                    int32_t *idx)
    {
        hipLaunchKernelGGL(ray_kernel, grid(n), dim3(bs), lds, h->stream, m, o, d, tmax, n, hit, t, idx);
    }
    static hipError_t sdf_out(wost_context *h, Batch &, int, float **out)
    {
        *out = h->field;
        return hipSuccess;
    }
    static void sdf(wost_context *h, const DevMesh &m, int which_mesh, size_t lds, int n, float *out)
    {
        hipLaunchKernelGGL(sdf_kernel, grid(n), dim3(bs), lds, h->stream, m, h->probe, h->settings.width, h->settings.height, which_mesh, out, bs);
    }
    static void source(wost_context *h, int n, float *out)
    {
        hipLaunchKernelGGL(source_kernel, grid(n), dim3(bs), 0, h->stream, h->src, h->probe, h->settings.width, h->settings.height, out);
    }
};
}  // namespace

extern "C" {

int wost_points_carry(wost_handle h, const float *pts_xy, int32_t n, int32_t seed_base, int32_t seed_width)
{
    return kPoints.bind(h, pts_xy, true, n, seed_base, seed_width, nullptr);
}

int wost_points_carry_dev(wost_handle h, const float *pts_xy_dev, int32_t n, int32_t seed_base, int32_t seed_width, void *stream)
{
    return kPoints.bind(h, pts_xy_dev, false, n, seed_base, seed_width, stream);
}

int wost_points_more(wost_handle h, int32_t more_spp, const uint8_t *select, float *field_rgb, wost_stats *stats)
{
    return kPoints.more(h, more_spp, select, field_rgb, stats);
}

int wost_points_more_dev(wost_handle h, int32_t more_spp, const uint8_t *select_dev, float *field_rgb_dev, void *stream, wost_stats *stats)
{
    return kPoints.more_dev(h, more_spp, select_dev, field_rgb_dev, stream, stats);
}

int wost_points_carried(wost_handle h, int32_t *spp, int32_t *batches, float *sum_rgb, float *stderr_rgb)
{
    return kPoints.carried(h, spp, batches, sum_rgb, stderr_rgb);
}

int wost_points_adaptive(wost_handle h, const wost_adaptive *a, float *field_rgb, float *stderr_rgb, int32_t *spp_map, wost_stats *stats)
{
    return kPoints.adaptive(h, a, field_rgb, stderr_rgb, spp_map, stats);
}

int wost_points_adaptive_dev(wost_handle h, const wost_adaptive *a, float *field_rgb_dev, void *stream, wost_stats *stats)
{
    return kPoints.adaptive_dev(h, a, field_rgb_dev, stream, stats);
}

int wost_points_restart(wost_handle h) { return kPoints.restart(h); }

int wost_points_progress(wost_handle h, int32_t *n_points, int32_t *spp_done) { return kPoints.progress(h, n_points, spp_done); }

int wost_solve(wost_handle h, int32_t pixel_begin, int32_t pixel_end, float *field_rgb, wost_stats *stats)
{
    return kUniform.solve(h, pixel_begin, pixel_end, field_rgb, stats);
}

int wost_solve_sharded(wost_handle h, int32_t shard_index, int32_t shard_count, float *field_rgb_dev, void *stream, wost_stats *stats)
{
    return kUniform.solve_sharded(h, shard_index, shard_count, field_rgb_dev, stream, stats);
}

int wost_solve_more_where(wost_handle h, int32_t more_spp, const uint8_t *select, float *field_rgb, wost_stats *stats)
{
    return kCarry.more_where(h, more_spp, select, field_rgb, stats);
}

int wost_solve_more(wost_handle h, int32_t more_spp, float *field_rgb, wost_stats *stats)
{
    return kCarry.more_where(h, more_spp, nullptr, field_rgb, stats);
}

int wost_solve_more_where_sharded(wost_handle h, int32_t shard_index, int32_t shard_count, int32_t more_spp, const uint8_t *select_dev,
                                  float *field_rgb_dev, void *stream, wost_stats *stats)
{
    return kCarry.more_where_sharded(h, shard_index, shard_count, more_spp, select_dev, field_rgb_dev, stream, stats);
}

int wost_solve_more_sharded(wost_handle h, int32_t shard_index, int32_t shard_count, int32_t more_spp, float *field_rgb_dev, void *stream,
                            wost_stats *stats)
{
    return kCarry.more_where_sharded(h, shard_index, shard_count, more_spp, nullptr, field_rgb_dev, stream, stats);
}

int wost_solve_adaptive_sharded(wost_handle h, int32_t shard_index, int32_t shard_count, const wost_adaptive *a, float *field_rgb_dev, void *stream,
                                wost_stats *stats)
{
    return kCarry.adaptive_sharded(h, shard_index, shard_count, a, field_rgb_dev, stream, stats);
}

int wost_solve_adaptive(wost_handle h, const wost_adaptive *a, float *field_rgb, float *stderr_rgb, int32_t *spp_map, wost_stats *stats)
{
    return kCarry.adaptive(h, a, field_rgb, stderr_rgb, spp_map, stats);
}

int wost_solve_carried(wost_handle h, int32_t *spp, int32_t *batches, float *sum_rgb, float *stderr_rgb)
{
    return kCarry.carried(h, spp, batches, sum_rgb, stderr_rgb);
}

int wost_solve_restart(wost_handle h) { return kCarry.restart(h); }

int wost_solve_progress(wost_handle h, int32_t *spp_done) { return kCarry.progress(h, spp_done); }

int wost_solve_points_dev(wost_handle h, const float *pts_xy_dev, int32_t n, int32_t seed_base, int32_t seed_width, float *field_rgb_dev,
                          void *stream, wost_stats *stats)
{
    return kUniform.solve_points_dev(h, pts_xy_dev, n, seed_base, seed_width, field_rgb_dev, stream, stats);
}

int wost_solve_points(wost_handle h, const float *pts_xy, int32_t n, int32_t seed_base, int32_t seed_width, float *field_rgb, wost_stats *stats)
{
    return kUniform.solve_points(h, pts_xy, n, seed_base, seed_width, field_rgb, stats);
}

int wost_solve_gradient_points(wost_handle h, const float *pts_xy, int32_t n, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width,
                               const wost_gradient_out *out, wost_stats *stats)
{
    return grad_entry(h, grad_call, 2, pts_xy, true, n, seed_base, walk_seed_base, seed_width, out, nullptr, stats);
}

int wost_solve_gradient_points_dev(wost_handle h, const float *pts_xy_dev, int32_t n, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width,
                                   const wost_gradient_out *out, void *stream, wost_stats *stats)
{
    return grad_entry(h, grad_call, 2, pts_xy_dev, false, n, seed_base, walk_seed_base, seed_width, out, stream, stats);
}

int wost_gradient_points_carry(wost_handle h, const float *pts_xy, int32_t n, int32_t batch_walks, int32_t round_stride, int32_t max_rounds,
                               int32_t seed_base, int32_t walk_seed_base, int32_t seed_width)
{
    return kGradList.bind(h, pts_xy, true, n, batch_walks, round_stride, max_rounds, seed_base, walk_seed_base, seed_width, nullptr);
}

int wost_gradient_points_carry_dev(wost_handle h, const float *pts_xy_dev, int32_t n, int32_t batch_walks, int32_t round_stride, int32_t max_rounds,
                                   int32_t seed_base, int32_t walk_seed_base, int32_t seed_width, void *stream)
{
    return kGradList.bind(h, pts_xy_dev, false, n, batch_walks, round_stride, max_rounds, seed_base, walk_seed_base, seed_width, stream);
}

int wost_gradient_points_more(wost_handle h, const uint8_t *select, const wost_gradient_carried_out *out, wost_stats *stats)
{
    return kGradList.more(h, select, true, out, nullptr, stats);
}

int wost_gradient_points_more_dev(wost_handle h, const uint8_t *select_dev, const wost_gradient_carried_out *out_dev, void *stream, wost_stats *stats)
{
    return kGradList.more(h, select_dev, false, out_dev, stream, stats);
}

int wost_gradient_points_carried(wost_handle h, const wost_gradient_carried_out *out) { return kGradList.carried(h, out); }

int wost_gradient_points_adaptive(wost_handle h, const wost_gradient_adaptive *a, const wost_gradient_carried_out *out, wost_stats *stats)
{
    return kGradList.adaptive(h, a, true, out, nullptr, stats);
}

int wost_gradient_points_adaptive_dev(wost_handle h, const wost_gradient_adaptive *a, const wost_gradient_carried_out *out_dev, void *stream,
                                      wost_stats *stats)
{
    return kGradList.adaptive(h, a, false, out_dev, stream, stats);
}

int wost_gradient_points_restart(wost_handle h) { return kGradList.restart(h); }

int wost_gradient_points_progress(wost_handle h, int32_t *n_points, int32_t *rounds_done) { return kGradList.progress(h, n_points, rounds_done); }

int wost_last_launches(wost_handle h, wost_launch_info *out, int32_t capacity, int32_t *count)
{
    if (!h || !count || (capacity > 0 && !out) || capacity < 0) return set_error(WOST_ERR_INVALID, "null argument");
    *count = (int32_t)h->last_launches.size();
    for (int32_t i = 0; i < std::min(*count, capacity); ++i) out[i] = h->last_launches[(size_t)i];
    return WOST_OK;
}

int wost_render_sdf(wost_handle h, int which_mesh, float *out_dist) { return query_render_sdf<Query2>(h, which_mesh, out_dist); }

int wost_render_source(wost_handle h, float *out_rgb) { return query_render_source<Query2>(h, out_rgb); }

int wost_closest_point(wost_handle h, int which_mesh, const float *pts, int32_t n, int32_t *out_idx, float *out_dist,
                       float *out_uv, int32_t *out_side)
{
    return query_closest_point<Query2>(h, which_mesh, pts, n, out_idx, out_dist, out_uv, out_side);
}

int wost_closest_silhouette(wost_handle h, int which_mesh, const float *pts, const float *rmax, int32_t n,
                            float *out_dist)
{
    return query_closest_silhouette<Query2>(h, which_mesh, pts, rmax, n, out_dist);
}

int wost_ray_intersect(wost_handle h, int which_mesh, const float *origins, const float *dirs, const float *tmax,
                       int32_t n, int32_t *out_hit, float *out_t, int32_t *out_idx)
{
    return query_ray_intersect<Query2>(h, which_mesh, origins, dirs, tmax, n, out_hit, out_t, out_idx);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// the exit list (wost_exits_walk & co.; the list, apply and adjoint: wost_exits.hip; the bodies of the entry points: ExitCalls)
// ------------------------------------------------------------------------------------------
namespace wost {

struct ExitWalkParams {
    DevMesh dm, nm;
    DevSettings st;      // (spp: 1)
    DevSource src;
    ExitWalk w;
    int32_t stack_stride;
};

// One lane per walk, in lock step to the walk's end: the depth-0 query of init_points_kernel (closest_point_lockstep, the
// far-point scan included), every later query seeded with the lane's hint as the round kernels seed it -- the plain visits
// within dm.far2, the slack ones beyond, the scan by the wave beyond dm.huge2 (closest_point_scan_huge) --, and between two
// queries the unchanged step_finish with the flags
// of the handle's point solve, not chained.  So walk w takes the steps of wost_solve_points of one sample at its point on the
// stream of pixel walk_seed_base + w, bit for bit; the lane keeps the throughput and the sums as they stood before each step,
// and when the step absorbs -- L.hint the slot, L.px, L.py still the absorbed position -- it forms uv and side as the batch
// query reports them (segment_uv_side) and writes the record.  Cold path beside the scheduled kernels: no queue, no rounds.
template <bool NEUMANN_EMISSIVE, bool NEUMANN_TREE, bool SOURCE>
__global__ __launch_bounds__(256) void exits2_kernel(ExitWalkParams P)
{
    extern __shared__ uint32_t lds_stack[];
    uint32_t *stack = lds_stack + threadIdx.x;
    const LdsColumn stk{stack, (uint32_t)P.stack_stride};
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool owned = t < P.w.count;
    const int32_t w = P.w.first_walk + (owned ? t : 0);
    const bool has_d = P.dm.n_segs > 0;
    float x0 = 0, y0 = 0;
    if (owned) {
        const size_t i = (size_t)(w / P.w.S);
        x0 = P.w.pts[2 * i];
        y0 = P.w.pts[2 * i + 1];
    }
    const bool finite = isfinite(x0) && isfinite(y0);
    bool alive = owned && finite;
    Lane L{};
    L.rng = Pcg{0, 1};
    if (alive) pcg_seed_pixel(L.rng, P.w.walk_seed_base + w, P.w.seed_width);
    Closest cp = closest_point_lockstep(P.dm, x0, y0, alive, stack, P.stack_stride);
    L.x0 = x0; L.y0 = y0; L.px = x0; L.py = y0;
    L.hint = cp.slot;
    L.thp = 1.0f;
    L.d0_d2 = cp.d2; L.d0_slot = cp.slot;
    // the record: a walk that is not absorbed keeps slot -1 and its final sums, a point that is not finite NaN
    int32_t slot = -1, side = 0;
    float uv = finite ? 0.0f : __int_as_float(0x7fc00000), thp = uv, br = uv, bg = uv, bb = uv;
    uint32_t c_steps = 0, c_absorbed = 0, c_truncated = 0, c_nhits = 0;
    const uint32_t c_started = alive ? 1u : 0u;
    while (__ballot(alive)) {
        if (alive) {
            thp = L.thp; br = L.sr; bg = L.sg; bb = L.sb;
            ++c_steps;
            const uint32_t status = step_finish<NEUMANN_EMISSIVE, NEUMANN_TREE, SOURCE>(P.dm, P.nm, P.st, L, cp, stk, P.src, false);
            c_absorbed += (status >> 1) & 1u;
            c_truncated += (status >> 2) & 1u;
            c_nhits += (status >> 3) & 1u;
            if (status & STEP_ABSORBED) {
                slot = L.hint;
                segment_uv_side(P.dm, slot, L.px, L.py, uv, side);
            } else if (status & STEP_ENDED) {
                thp = L.thp; br = L.sr; bg = L.sg; bb = L.sb;
            }
            if (status & STEP_ENDED) alive = false;
        }
        bool huge = false;
        if (alive && has_d) {
            cp = slot_candidate(P.dm, L.hint, L.px, L.py);
            if (cp.d2 > P.dm.huge2) {
                huge = true;
            } else {
                Trav T = trav_begin(cp);
                if (cp.d2 > P.dm.far2) {
                    while (trav_visit<true>(P.dm, L.px, L.py, T, stk)) {
                    }
                } else {
                    while (trav_visit<false>(P.dm, L.px, L.py, T, stk)) {
                    }
                }
                cp = T.best;
            }
        }
        closest_point_scan_huge(P.dm, L.px, L.py, huge, cp);
    }
    if (owned) {
        const ExitRecords &R = P.w.rec;
        R.prim()[w] = slot >= 0 ? P.dm.segOrig[slot] : -1;
        R.slot()[w] = slot;
        R.side()[w] = side;
        R.uv(0)[w] = uv;
        R.thp()[w] = thp;
        R.base(2, 0)[w] = br; R.base(2, 1)[w] = bg; R.base(2, 2)[w] = bb;
    }
    wave_add_counters(P.w.counters, c_steps, c_started, c_absorbed, c_truncated, c_nhits);
}

}  // namespace wost

// what the 2-D context adds: the walk kernel on its meshes and source, with the flags of its point solve (launch_walk)
static ExitCall exit_call(wost_context *c)
{
    ExitCall e{"wost_", 2, c->device, c->n_pixels, c->stream, &c->exits, reinterpret_cast<const int32_t *>(c->dm.view.segVerts), c->dirichlet_verts,
               c->dst.dirichlet_intensity, nullptr};
    e.walk = [c](const ExitWalk &w, hipStream_t stream) {
        const LaunchGeometry g = launch_geometry(c);
        ExitWalkParams P{c->dm.view, c->nm.view, c->dst, c->src, w, 256};
        P.st.spp = 1;
        const dim3 grid((unsigned)((w.count + 255) / 256));
        const size_t lds = (size_t)g.stack_depth * 256 * sizeof(uint32_t);
        auto launch = [&](auto E, auto T, auto S) {
            hipLaunchKernelGGL((exits2_kernel<decltype(E)::value, decltype(T)::value, decltype(S)::value>), grid, dim3(256), lds, stream, P);
        };
        auto with_src = [&](auto E, auto T) { g.has_src ? launch(E, T, std::true_type{}) : launch(E, T, std::false_type{}); };
        auto with_tree = [&](auto E) { g.ntree ? with_src(E, std::true_type{}) : with_src(E, std::false_type{}); };
        g.emissive ? with_tree(std::true_type{}) : with_tree(std::false_type{});
        WOST_TRY(hipGetLastError());
        return WOST_OK;
    };
    e.prep = [c](const GradPrep &p, hipStream_t stream) { return grad_prep2(c->dm.view, c->nm.view, p, stream); };
    e.eps = c->dst.eps;
    e.has_source = c->src.rgb != nullptr;
    e.source_term = c->exits_grad_source;
    e.ball = [c](const GradBall &p, hipStream_t stream) { return grad_ball2(c->src, p, stream); };
    return e;
}

static const ExitCalls<wost_context> kExits{exit_call, 2};

extern "C" {

int wost_exits_walk(wost_handle h, const float *pts_xy, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width, wost_stats *stats)
{
    return kExits.walk(h, pts_xy, true, n, walks, walk_seed_base, seed_width, nullptr, stats);
}

int wost_exits_walk_dev(wost_handle h, const float *pts_xy_dev, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width, void *stream,
                        wost_stats *stats)
{
    return kExits.walk(h, pts_xy_dev, false, n, walks, walk_seed_base, seed_width, stream, stats);
}

int wost_exits_records(wost_handle h, const wost_exit_records *out) { return kExits.records(h, out); }

int wost_exits_apply(wost_handle h, const float *colors, int32_t K, float *field_rgb, float *stderr_rgb)
{
    return kExits.apply(h, colors, K, field_rgb, stderr_rgb, true, nullptr);
}

int wost_exits_apply_dev(wost_handle h, const float *colors_dev, int32_t K, float *field_rgb_dev, float *stderr_rgb_dev, void *stream)
{
    return kExits.apply(h, colors_dev, K, field_rgb_dev, stderr_rgb_dev, false, stream);
}

int wost_exits_adjoint(wost_handle h, const float *dfield, int32_t K, float *dcolors) { return kExits.adjoint(h, dfield, K, dcolors, true, nullptr); }

int wost_exits_adjoint_dev(wost_handle h, const float *dfield_dev, int32_t K, float *dcolors_dev, void *stream)
{
    return kExits.adjoint(h, dfield_dev, K, dcolors_dev, false, stream);
}

int wost_exits_progress(wost_handle h, int32_t *n_points, int32_t *walks) { return kExits.progress(h, n_points, walks); }

int wost_exits_walk_gradient(wost_handle h, const float *pts_xy, int32_t n, int32_t walks, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width,
                             wost_stats *stats)
{
    return kExits.walk_gradient(h, pts_xy, true, n, walks, ExitSeeds{seed_base, walk_seed_base, seed_width}, nullptr, stats);
}

int wost_exits_walk_gradient_dev(wost_handle h, const float *pts_xy_dev, int32_t n, int32_t walks, int32_t seed_base, int32_t walk_seed_base,
                                 int32_t seed_width, void *stream, wost_stats *stats)
{
    return kExits.walk_gradient(h, pts_xy_dev, false, n, walks, ExitSeeds{seed_base, walk_seed_base, seed_width}, stream, stats);
}

int wost_exits_gradient_records(wost_handle h, const wost_exit_gradient_records *out) { return kExits.gradient_records(h, out); }

int wost_exits_apply_gradient(wost_handle h, const float *colors, int32_t K, float *grad, float *grad_stderr, float *field_rgb)
{
    return kExits.apply_gradient(h, colors, K, grad, grad_stderr, field_rgb, true, nullptr);
}

int wost_exits_apply_gradient_dev(wost_handle h, const float *colors_dev, int32_t K, float *grad_dev, float *grad_stderr_dev, float *field_rgb_dev,
                                  void *stream)
{
    return kExits.apply_gradient(h, colors_dev, K, grad_dev, grad_stderr_dev, field_rgb_dev, false, stream);
}

int wost_exits_gradient_terms(wost_handle h, double *T, double *seT, double *U) { return kExits.gradient_terms(h, T, seT, U); }

int wost_exits_adjoint_gradient(wost_handle h, const float *dgrad, int32_t K, float *dcolors)
{
    return kExits.adjoint_gradient(h, dgrad, K, dcolors, true, nullptr);
}

int wost_exits_adjoint_gradient_dev(wost_handle h, const float *dgrad_dev, int32_t K, float *dcolors_dev, void *stream)
{
    return kExits.adjoint_gradient(h, dgrad_dev, K, dcolors_dev, false, stream);
}

int wost_exits_index(wost_handle h) { return kExits.index(h); }

int wost_exits_index_info(wost_handle h, int64_t *n_incidences, int64_t *longest_bin) { return kExits.index_info(h, n_incidences, longest_bin); }

int wost_exits_index_records(wost_handle h, int64_t *bin_begin, int32_t *inc) { return kExits.index_records(h, bin_begin, inc); }

int wost_exits_adjoint_ordered(wost_handle h, const float *dfield, int32_t K, float *dcolors)
{
    return kExits.adjoint_ordered(h, dfield, K, dcolors, true, nullptr);
}

int wost_exits_adjoint_ordered_dev(wost_handle h, const float *dfield_dev, int32_t K, float *dcolors_dev, void *stream)
{
    return kExits.adjoint_ordered(h, dfield_dev, K, dcolors_dev, false, stream);
}

int wost_exits_adjoint_gradient_ordered(wost_handle h, const float *dgrad, int32_t K, float *dcolors)
{
    return kExits.adjoint_gradient_ordered(h, dgrad, K, dcolors, true, nullptr);
}

int wost_exits_adjoint_gradient_ordered_dev(wost_handle h, const float *dgrad_dev, int32_t K, float *dcolors_dev, void *stream)
{
    return kExits.adjoint_gradient_ordered(h, dgrad_dev, K, dcolors_dev, false, stream);
}

}  // extern "C"
