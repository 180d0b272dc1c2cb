// wost_hip3d.hip -- the 3-D uniform Walk-on-Stars path on MI355X, gfx950 only.
//
// Holds: the 3-D walk and query kernels; the solve driver (run_solve3) and its plan; what the 3-D context adds to the shared
// bodies of the entry points (wost_uniform.h, wost_carry.h, wost_grad.h) and the wost3_ entry points themselves, which forward
// to those bodies.  The context is in wost_internal3.h, the mesh upload in wost_build3.hip.
//
// UniformIntegrator<3> of the reference: the DIM == 3 branches of integrator/uniform/integrator.cu
// (:128-211 separateEvaluationPoint with triangles and barycentric uv :150-168, :224-231
// handleBoundary, :336-444 sampleNeumann with three draws, :465-525 oneStepWalk), EvaluationGrid<3>
// (core/evaluation_grid.h:43-70), uniformSampleSphere<3> / Hemisphere<3> (util/sampling.h:20-27,57-66),
// frameFromNormal(Vector3f) (util/transformation.h:62-67, util/math_utils.h:141-151) and
// HarmonicGreenBall<3>::eval (util/green.h:82-90), behind wost3_* of include/wost.h.
//
// Design: the same regenerating walker as the 2-D round kernel -- one lane owns one PIXEL and walks
// its samples one after the other on the pixel's PCG stream (the reference's per-pixel order) --
// but a whole solve is ONE launch: a lane runs its pixel to the end.  Closest-point queries descend
// an implicit 4-ary LBVH over the triangles (3-D Morton order, axis-aligned child boxes, 96-byte
// nodes, near-first with the per-lane LDS stack and the key format of the 2-D tree, wost_device.h).
// Neumann meshes of up to WOST3_FLAT_MAX triangles (a box, a clipped plane) are walked with wave-uniform flat
// loops; larger ones descend the same kind of tree for the silhouette and ray queries (the triangle sampling of an
// EMISSIVE Neumann mesh stays a flat loop, as in 2-D).  Source term: a dense grid, trilinear.  Arithmetic contract: DESIGN.md 2.3 (the CPU restatement the tests compare against
// follows the same contract operation for operation).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/wost.h"
#include "lbvh.h"
#include "wost_device.h"
#include "wost_internal.h"
#include "wost_device3.h"
#include "wost_internal3.h"

namespace wost {

struct Walk3Params {
    DevMesh3 dm, nm;
    DevSettings st;
    DevProbe3 probe;
    DevSource3 src;
    const uint8_t *mask;
    float *field;              // solution / spp at field[(pix - field_base) * 3]
    int32_t field_base, pixel_begin, pixel_end;
    int32_t shard_index, shard_count;
    Stats3Dev *stats;
    uint32_t *cursor;          // next unread pixel slot of the launch
    int32_t tiled;             // the range is a whole frame made of 8x8 tiles: slots follow the tiles
    int32_t wait_weight, trav_burst;
    // NTREE kernels: the Neumann-side tree queries of a step answered by the wave as a whole (closest_silhouette3_wave,
    // ray_closest3_wave); pool_cap tasks per pool and wave, behind the stack columns of the block in LDS
    int32_t coop, pool_cap, stack_words, ray_slot_trigger, cp_slot_trigger;
    // a point solve (wost3_solve_points, the POINTS instantiations): slot s is point pixel_begin + s of `points` (x, y, z) on the
    // stream of pixel seed_base + that index in a frame seed_width wide -- no tiles, no shards, no mask; nullptr = the pixels of the frame
    // (at the end: the frame instantiations read every other field where they always did)
    const float *points;
    int32_t seed_base, seed_width;
    // a continued frame solve (wost3_solve_more & co., the CARRY instantiations): a pixel with carry_n[pid] > 0 samples behind it
    // starts from its carried generator state and raw sums; a resolved pixel leaves both under its pixel id and its field entry is
    // sum / carry_total (the kernel that closes the call writes the pixel's own: wost_carry.hip); st.spp is this call's count and a
    // lane counts the call's samples from 0.  ids != nullptr: the call walks a selection -- slot s is pixel ids[s] of n_ids, every
    // one owned and unmasked.  (At the end, like the points.)  POINTS and CARRY together: a call on the handle's carried point
    // list (wost3_points_more & co.) -- the buffers are the list's, indexed like `points`; ids lists the selected, finite points.
    uint64_t *carry_rng;
    float *carry_sum;
    int32_t carry_done, carry_total;
    const uint32_t *carry_n;
    const int32_t *ids;
    int32_t n_ids;
};

// One lane = one pixel, all its samples one after the other on the pixel's PCG stream (the reference's per-pixel
// order) -- scheduled like the 2-D round kernel: a lane is descending the Dirichlet tree (TRAV), waits with a finished
// query for the rest of its step (WAIT), or wants the next pixel of the solve (REFILL); every trip of the loop runs
// the body more lanes are ready for, persistent blocks drain one pixel cursor.  (The first version ran every lane's
// query to completion in lock step, one launch of pixel-many lanes: 4.7e8 walk-steps/s on a 1280-triangle sphere.)
struct Lane3 {
    int pid, sample, depth;
    V3 p, p_eval, nn;
    float thp;
    bool on_n;
    int32_t hint, hint0;
    Pcg rng;
    float sol[3];
    Closest d0;          // the query of the evaluation point, the same for every sample of the pixel
    bool d0_valid;
    uint32_t c_steps, c_started, c_absorbed, c_truncated, c_nhits;
};

// the rest of a step once the closest Dirichlet triangle is known (`cp`, ignored without that mesh); true = the walk
// has ended (absorbed, no boundary at all), false = L.p is the next point
#ifdef WOST3_PROFILE
#define PROF3_T0() unsigned long long prof_t = __builtin_readcyclecounter()
#define PROF3(k) do { const unsigned long long prof_n = __builtin_readcyclecounter(); if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) atomicAdd(&g_prof3[k], prof_n - prof_t); prof_t = prof_n; } while (0)
#else
#define PROF3_T0() do {} while (0)
#define PROF3(k) do {} while (0)
#endif

// One walk step in three parts around its two tree queries -- the closest silhouette edge after part A, the walker's
// ray after part B.  The kernel answers them on the spot (step3).  Making them states of the lane machine like the
// closest-point descent (one node visit per trip: sil3_visit / ray3_visit, a trip running the body most lanes are
// ready for) was built on these parts and measured: bit-exact, but SLOWER on a 1280-triangle shell (zero flux 660 ->
// 770 ms, emissive 1570 -> 1950 ms at the best scheduler constants of each): four kinds of lanes per wave fill a body
// worse than the longest-lane wait inside the step costs, and the kernel holds both query states (165 VGPRs).
// A: the Dirichlet side.  true = absorbed.
__device__ __forceinline__ bool step3_a(const Walk3Params &P, Lane3 &L, Closest cp, float &R_D)
{
    const bool has_d = P.dm.n_tris > 0;
    const float eps = P.st.eps;
    V3 &p = L.p;
    float &thp = L.thp;
    float (&sol)[3] = L.sol;
    int32_t &hint = L.hint;
    R_D = WOST_INF;
    if (has_d) {
        hint = cp.slot;
        if (L.depth == 0) L.hint0 = cp.slot;
        const float4 a = P.dm.tri[3 * (size_t)cp.slot], b = P.dm.tri[3 * (size_t)cp.slot + 1], c = P.dm.tri[3 * (size_t)cp.slot + 2];
        const V3 p0 = v3(a.x, a.y, a.z), e0 = v3(b.x, b.y, b.z) - p0, e1 = v3(c.x, c.y, c.z) - p0;
        const int side = tri_side(p0, cross3(e0, e1), p);
        float u, v;
        tri_uv(p0, e0, e1, p, u, v);
        R_D = sqrtf(cp.d2);
        if (R_D < eps && u > 0.0f && v > 0.0f && u + v < 1.0f) {
            float col[3];
            const int32_t *tv = P.dm.triVerts + 3 * (size_t)cp.slot;
            surface_color3(P.dm.colors, tv[0], tv[1], tv[2], side, u, v, col);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                col[k] *= P.st.dirichlet_intensity;
                col[k] *= thp;
                sol[k] = col[k] + sol[k];
            }
            ++L.c_absorbed;
            return true;
        }
    }
    return false;
}

// B: the star radius, the source and Neumann samples, the direction of the step -- in three parts around the two rays those
// samples ask for (the source sample's line to the boundary, the boundary sample's shadow ray), so that the kernel can answer
// them by the wave like the walker's own ray (step3_b answers them on the spot).  The draws of a lane keep their order.
struct Step3B {
    float R_B;
    V3 sdir;                 // source sample: direction, its density, the boundary factor
    float dir_pdf, salpha;
    int oi;                  // boundary sample: triangle, density, the point, its distance, the shadow ray (o, rd, cd)
    float pdf, r, cd;
    V3 sp, o, rd;
};

// B0: the radius; the direction of the source sample.  true = no boundary at all (the walk ends)
template <bool SOURCE>
__device__ __forceinline__ bool step3_b0(const Walk3Params &P, Lane3 &L, float R_D, float R_N, Step3B &B)
{
    float R_B = fmaxf(WOST_R_B_FLOOR, fminf(R_D, R_N));
    R_B *= WOST_R_B_SHRINK;
    B.R_B = R_B;
    if (isinf(R_B)) return true;
    // ---- sampleSource (reference integrator/uniform/integrator.cu:235-316, DIM == 3) ----
    if (SOURCE) {
        B.salpha = 1.0f;
        const float u1 = pcg_next_float(L.rng), u2 = pcg_next_float(L.rng);
        float c, s;
        sincos_2pi(u2, c, s);
        if (L.on_n) {
            const float z = u1, r = sqrtf(fmaxf(0.0f, 1.0f - z * z));
            B.sdir = frame_to_world(L.nn, r * c, r * s, z);
            B.dir_pdf = 1.0f / WOST_2PI;
            B.salpha = 0.5f;
        } else {
            const float z = 1 - 2 * u1, r = sqrtf(1 - z * z);
            B.sdir = v3(r * c, r * s, z);
            B.dir_pdf = 1.0f / WOST_4PI;
        }
    }
    return false;
}
// the source sample's line: from p + eps sdir along sdir, at most R_B long (asked for when the scene has a Neumann mesh)
__device__ __forceinline__ V3 step3_source_origin(const Walk3Params &P, const Lane3 &L, const Step3B &B)
{
    const float eps = P.st.eps;
    return v3(L.p.x + eps * B.sdir.x, L.p.y + eps * B.sdir.y, L.p.z + eps * B.sdir.z);
}

// B1: the source sample with its line answered (hit, t); the boundary sample.  true = the shadow ray (B.o, B.rd, B.cd - eps) is asked for
template <bool EMISSIVE, bool SOURCE, bool NTREE>
__device__ __forceinline__ bool step3_b1(const Walk3Params &P, Lane3 &L, Step3B &B, bool src_hit, float src_t)
{
    const bool has_n = P.nm.n_tris > 0;
    const float eps = P.st.eps, R_B = B.R_B;
    const V3 p = L.p;
    const float thp = L.thp;
    float (&sol)[3] = L.sol;
    Pcg &rng = L.rng;
    PROF3_T0();
    if (SOURCE) {
        // how far the straight line stays inside the star-shaped region (:279-292)
        float dist = R_B;
        if (has_n && src_hit) dist = fminf(src_t, dist);
        const V3 sdir = B.sdir;
        // HarmonicGreenBall<3>::sample (util/green.h:101-116): closed form, two draws
        const float g1 = pcg_next_float(rng), g2 = pcg_next_float(rng);
        float gc, gs;
        sincos_2pi(g2, gc, gs);
        float r = (1.0f + sqrtf(1.0f - cbrt01(g1 * g1)) * gc) * R_B / 2.0f;
        r = fmaxf(1e-4f, r);                                            // ELAINA_GREEN_FUNC_R_CLAMP
        if (r > R_B) r = R_B / 2.0f;
        if (r <= dist) {
            float f[3];
            source3_eval(P.src, v3(p.x + r * sdir.x, p.y + r * sdir.y, p.z + r * sdir.z), f);
            const float norm = R_B * R_B / 6.0f;
            const float c1 = (1.0f / WOST_4PI) / (r * r), c2 = B.dir_pdf / (r * r);     // conditionalSampleSpherePDF<3>
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float col = thp * f[k] * norm * c1 / c2 / B.salpha;
                sol[k] = col + sol[k];
            }
        }
    }
    PROF3(1);
    // ---- sampleNeumann: three draws whether or not the boundary emits ----
    bool shadow = false;
    if (has_n) {
        const float u0 = pcg_next_float(rng), u1 = pcg_next_float(rng), u2 = pcg_next_float(rng);
        if (EMISSIVE) {
            float pdf;
            const int oi = (NTREE && P.nm.obox_levels > 0) ? sample_in_sphere3_tree(P.nm, p, R_B, u0, pdf) : sample_in_sphere3_flat(P.nm, p, R_B, u0, pdf);
            if (oi != -1 && pdf > 0) {
                const DevTri &S = P.nm.flat[oi];
                const V3 s0 = ld3(S.p0), s1 = ld3(S.p1), s2 = ld3(S.p2);
                const float su = sqrtf(u1), b1 = u2 * su, b0 = 1.0f - su, b2 = 1.0f - b0 - b1;
                const V3 sp = v3((s0.x * b0 + s1.x * b1) + s2.x * b2, (s0.y * b0 + s1.y * b1) + s2.y * b2,
                                 (s0.z * b0 + s1.z * b1) + s2.z * b2);
                const V3 rv = sp - p;
                const float r = sqrtf(dot3(rv, rv));
                if (r < R_B && r > 0) {
                    V3 o = p;
                    if (L.on_n) o = v3(p.x + eps * L.nn.x, p.y + eps * L.nn.y, p.z + eps * L.nn.z);
                    V3 rd = sp - o;
                    const float cd = sqrtf(dot3(rd, rd));
                    if (cd > 0) { rd.x /= cd; rd.y /= cd; rd.z /= cd; }
                    B.oi = oi; B.pdf = pdf; B.r = r; B.cd = cd; B.sp = sp; B.o = o; B.rd = rd;
                    shadow = true;
                }
            }
        }
    }
    return shadow;
}

// B2: the boundary sample when its shadow ray found nothing (`lit`); the direction of the step.  The walker's ray starts at
// `cur` along `dir` and is at most B.R_B long.
template <bool EMISSIVE>
__device__ __forceinline__ void step3_b2(const Walk3Params &P, Lane3 &L, const Step3B &B, bool lit, V3 &dir_out, V3 &cur_out)
{
    const float eps = P.st.eps;
    const V3 p = L.p;
    const bool on_n = L.on_n;
    const V3 nn = L.nn;
    float (&sol)[3] = L.sol;
    PROF3_T0();
    if (EMISSIVE && lit) {
        const DevTri &S = P.nm.flat[B.oi];
        const V3 s0 = ld3(S.p0), s1 = ld3(S.p1), s2 = ld3(S.p2);
        int side = tri_side(s0, ld3(S.nraw), p);
        float uu, vv;
        tri_uv(s0, s1 - s0, s2 - s0, B.sp, uu, vv);
        if (on_n) {
            const float dn = dot3(ld3(S.n), nn);
            side = (0.0f < dn) - (dn < 0.0f);
        }
        if (side != 0) {
            float col[3];
            const int32_t *tv = P.nm.flatVerts + 3 * (size_t)B.oi;
            surface_color3(P.nm.colors, tv[0], tv[1], tv[2], side, uu, vv, col);
            const float alpha = on_n ? 0.5f : 1.0f;
            const float G = (1.0f / B.r - 1.0f / B.R_B) / WOST_4PI;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                col[k] *= P.st.neumann_intensity;
                col[k] *= L.thp * G / alpha / B.pdf;
                sol[k] = -col[k] + sol[k];
            }
        }
    }
    PROF3(2);
    // ---- oneStepWalk ----
    V3 dir, cur = p;
    {
        const float u1 = pcg_next_float(L.rng), u2 = pcg_next_float(L.rng);
        float c, s;
        sincos_2pi(u2, c, s);
        if (on_n) {
            const float z = u1, r = sqrtf(fmaxf(0.0f, 1.0f - z * z));
            dir = frame_to_world(nn, r * c, r * s, z);
            cur = v3(p.x + eps * nn.x, p.y + eps * nn.y, p.z + eps * nn.z);
        } else {
            const float z = 1 - 2 * u1, r = sqrtf(1 - z * z);
            dir = v3(r * c, r * s, z);
        }
    }
    dir_out = dir; cur_out = cur;
}

// B with both rays answered by the lane itself.  true = no boundary at all (the walk ends)
template <bool EMISSIVE, bool SOURCE, bool NTREE>
__device__ __forceinline__ bool step3_b(const Walk3Params &P, Lane3 &L, float R_D, float R_N, const LdsColumn &stk, float &R_B_out, V3 &dir_out, V3 &cur_out)
{
    Step3B B;
    if (step3_b0<SOURCE>(P, L, R_D, R_N, B)) return true;
    bool src_hit = false;
    float src_t = 0.0f;
    if (SOURCE && P.nm.n_tris > 0) {
        int hi;
        src_hit = ray_closest3<NTREE>(P.nm, step3_source_origin(P, L, B), B.sdir, B.R_B, src_t, hi, stk);
    }
    bool lit = step3_b1<EMISSIVE, SOURCE, NTREE>(P, L, B, src_hit, src_t);
    if (EMISSIVE && lit) lit = !ray_any3<NTREE>(P.nm, B.o, B.rd, B.cd - P.st.eps, stk);
    step3_b2<EMISSIVE>(P, L, B, lit, dir_out, cur_out);
    R_B_out = B.R_B;
    return false;
}

// C: where the ray ended.
__device__ __forceinline__ void step3_c(const Walk3Params &P, Lane3 &L, float R_B, V3 dir, V3 cur, bool hit, float t, int hi)
{
    V3 nxt = v3(L.p.x + R_B * dir.x, L.p.y + R_B * dir.y, L.p.z + R_B * dir.z);
    V3 hn = v3(0.0f, 0.0f, 0.0f);
    if (hit) {
        hn = ld3(P.nm.flat[hi].n);
        if (dot3(hn, dir) > 0) hn = v3(-hn.x, -hn.y, -hn.z);
        nxt = v3(cur.x + t * dir.x, cur.y + t * dir.y, cur.z + t * dir.z);
        ++L.c_nhits;
    }
    // uniformSampleSphere / Hemisphere pdf and the boundary factor of the step that was taken from L.on_n
    const float pdf = L.on_n ? 1.0f / WOST_2PI : 1.0f / WOST_4PI, alpha = L.on_n ? 0.5f : 1.0f;
    L.thp = L.thp / pdf / alpha / WOST_4PI;
    L.p = nxt; L.on_n = hit; L.nn = hn;
}

// the whole step with both queries answered on the spot; true = the walk has ended
template <bool EMISSIVE, bool SOURCE, bool NTREE>
__device__ __forceinline__ bool step3(const Walk3Params &P, Lane3 &L, Closest cp, const LdsColumn &stk)
{
    float R_D, R_B;
    if (step3_a(P, L, cp, R_D)) return true;
    float R_N = WOST_INF;
    if (P.nm.n_tris > 0) R_N = closest_silhouette3<NTREE>(P.nm, L.p, R_D, stk);
    V3 dir, cur;
    if (step3_b<EMISSIVE, SOURCE, NTREE>(P, L, R_D, R_N, stk, R_B, dir, cur)) return true;
    bool hit = false;
    float t = 0.0f;
    int hi = -1;
    if (P.nm.n_tris > 0) hit = ray_closest3<NTREE>(P.nm, cur, dir, R_B, t, hi, stk);
    step3_c(P, L, R_B, dir, cur, hit, t, hi);
    return false;
}

constexpr int kWalk3Threads = 256;

// WAVE = true: the closest-point queries are answered by the wave as a whole as well (closest_triangle_pool) -- every trip of
// the loop is then "all queries of the wave, then one step for every walker": no lane waits for another's descent.
// POINTS = true: the launch of a point solve (wost3_solve_points) -- a refill takes a caller's point instead of a pixel of the frame.
// A template flag, not a test of P.points: with the test every frame instantiation held two more registers (EXPERIMENTS).
// CARRY = true: the launch of a continued solve (wost3_solve_more, Walk3Params::carry_rng); with POINTS, of a call on the carried
// point list (wost3_points_more).
template <bool EMISSIVE, bool SOURCE, bool NTREE, bool WAVE = false, bool POINTS = false, bool CARRY = false>
#ifndef WOST3_WAVES
#define WOST3_WAVES 1       // waves per SIMD walk3_kernel is compiled for (tuning builds override it)
#endif
__global__ __launch_bounds__(kWalk3Threads, WOST3_WAVES) void walk3_kernel(Walk3Params P)
{
    extern __shared__ uint32_t lds_stack[];
    const LdsColumn stk(lds_stack + threadIdx.x, blockDim.x);
    // the task pools of this wave (closest_silhouette3_wave & co.), behind the stack columns
    uint32_t *const pool_mem = lds_stack + P.stack_words + (threadIdx.x >> 6) * (2 * P.pool_cap + kPool3OwnerWords);
    const WavePool3 W{pool_mem + kPool3OwnerWords, pool_mem + kPool3OwnerWords + P.pool_cap, pool_mem, P.pool_cap};
#ifdef WOST3_PROFILE
    const unsigned long long prof_begin = __builtin_readcyclecounter();
#endif
    const int lane = threadIdx.x & 63;
    const bool has_d = P.dm.n_tris > 0;
    enum { MODE_TRAV = 1, MODE_QUERY = 2, MODE_WAIT = 3, MODE_DONE = 4, MODE_REFILL = 5, MODE_HUGE = 7 };
    int mode = MODE_REFILL;
    Lane3 L{};
    L.rng = Pcg{0, 1};
    Trav T = trav_begin(Closest{WOST_INF, -1});
    uint32_t pool_next = 0, pool_end = 0;
    uint32_t t_steps = 0, t_started = 0, t_absorbed = 0, t_truncated = 0, t_nhits = 0;
    const uint32_t n_slots = CARRY && P.ids ? (uint32_t)P.n_ids : (uint32_t)(P.pixel_end - P.pixel_begin);

    // start the query of a step (or serve it from the cache of the evaluation point)
    auto begin_step = [&]() {
        ++L.c_steps;
        if (!has_d) {
            T.best = Closest{WOST_INF, -1};
            mode = MODE_WAIT;
        } else if (L.depth == 0 && L.d0_valid) {
            T.best = L.d0;
            mode = MODE_WAIT;
        } else {
            T = trav_begin(Closest{WOST_INF, -1});
            if (L.hint >= 0 && P.dm.triOrig[L.hint] != WOST_FAR_INDEX) {
                const float4 a = P.dm.tri[3 * (size_t)L.hint], b = P.dm.tri[3 * (size_t)L.hint + 1], c = P.dm.tri[3 * (size_t)L.hint + 2];
                T.best = Closest{tri_d2(v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), v3(c.x, c.y, c.z), L.p), L.hint};
                T.best_orig = P.dm.triOrig[L.hint];
            }
            // a walker that strayed so far that the whole mesh ties within rounding: answered by the wave (main loop)
            mode = T.best.d2 > P.dm.huge2 ? MODE_HUGE : (WAVE ? MODE_QUERY : MODE_TRAV);
        }
    };
    auto begin_sample = [&]() {
        L.p = L.p_eval;
        L.thp = 1.0f;
        L.on_n = false;
        L.nn = v3(0.0f, 0.0f, 0.0f);
        ++L.c_started;
        L.hint = L.hint0;
        L.depth = 0;
        begin_step();
    };

    for (;;) {
        const unsigned long long need = __ballot(mode == MODE_REFILL);
        if (need) {
            const uint32_t needed = (uint32_t)__popcll(need), avail = pool_end - pool_next;
            uint32_t fresh_base = 0;
            if (needed > avail) {
                if (lane == 0) fresh_base = atomicAdd(P.cursor, 64u);
                fresh_base = __shfl(fresh_base, 0);
            }
            const uint32_t rank = (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
            const uint32_t s2 = rank < avail ? pool_next + rank : fresh_base + (rank - avail);
            if (needed > avail) {
                pool_next = fresh_base + (needed - avail);
                pool_end = fresh_base + 64u;
            } else {
                pool_next += needed;
            }
            if (mode == MODE_REFILL) {
                if (s2 >= n_slots) {
                    mode = MODE_DONE;
                } else if (POINTS) {
                    // a caller's point.  One with a non-finite coordinate is never walked -- no NaN walker in a persistent
                    // launch -- and its field entry is NaN; the lane asks again on the next trip
                    const int pid = CARRY && P.ids != nullptr ? P.ids[s2] : P.pixel_begin + (int)s2;
                    const V3 q = v3(P.points[3 * (size_t)pid], P.points[3 * (size_t)pid + 1], P.points[3 * (size_t)pid + 2]);
                    const bool finite = isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
                    if (!finite || P.st.spp <= 0) {
                        float *f = P.field + 3 * (size_t)(pid - P.field_base);
                        const float z = finite ? 0.0f / (float)P.st.spp : __int_as_float(0x7fc00000);
                        f[0] = z; f[1] = z; f[2] = z;
                    } else {
                        t_steps += L.c_steps; t_started += L.c_started; t_absorbed += L.c_absorbed; t_truncated += L.c_truncated; t_nhits += L.c_nhits;
                        L = Lane3{};
                        L.pid = pid;
                        L.rng = Pcg{0, 1};
                        pcg_seed_pixel(L.rng, P.seed_base + pid, P.seed_width);
                        if (CARRY && P.carry_n[pid] > 0u) {
                            L.rng.state = P.carry_rng[pid];
                            const float *cs = P.carry_sum + 3 * (size_t)pid;
                            L.sol[0] = cs[0]; L.sol[1] = cs[1]; L.sol[2] = cs[2];
                        }
                        L.p_eval = q;
                        L.hint = L.hint0 = -1;
                        L.sample = 0;
                        begin_sample();
                    }
                } else {
                    // slots walk the frame in 8x8 tiles when the range is the whole tiled frame (neighbouring walkers in a wave)
                    const bool listed = CARRY && P.ids != nullptr;
                    int pid = listed ? P.ids[s2] : P.pixel_begin + (int)s2;
                    if (!listed && P.tiled) {
                        const int tiles_x = P.st.width >> 3, tile = pid >> 6, in_tile = pid & 63;
                        pid = ((tile / tiles_x) * 8 + (in_tile >> 3)) * P.st.width + (tile % tiles_x) * 8 + (in_tile & 7);
                    }
                    const int px = pid % P.st.width, py = pid / P.st.width;
                    const int tile = (py >> 3) * ((P.st.width + 7) >> 3) + (px >> 3);
                    if (listed || (tile % P.shard_count) == P.shard_index) {
                        const bool masked = !listed && P.mask != nullptr && P.mask[pid] == 0;
                        if (masked || P.st.spp <= 0) {
                            float *f = P.field + 3 * (size_t)(pid - P.field_base);
                            const float spp = (float)P.st.spp;
                            f[0] = 0.0f / spp; f[1] = 0.0f / spp; f[2] = 0.0f / spp;
                        } else {
                            // fold the counters of the previous pixel into the lane totals (16-bit-safe: per pixel)
                            t_steps += L.c_steps; t_started += L.c_started; t_absorbed += L.c_absorbed; t_truncated += L.c_truncated; t_nhits += L.c_nhits;
                            L = Lane3{};
                            L.pid = pid;
                            L.rng = Pcg{0, 1};
                            pcg_seed_pixel(L.rng, pid, P.st.width);
                            if (CARRY && P.carry_n[pid] > 0u) {
                                L.rng.state = P.carry_rng[pid];
                                const float *cs = P.carry_sum + 3 * (size_t)pid;
                                L.sol[0] = cs[0]; L.sol[1] = cs[1]; L.sol[2] = cs[2];
                            }
                            L.p_eval = eval_point3(P.probe, px, py, P.st.width, P.st.height);
                            L.hint = L.hint0 = -1;
                            L.sample = 0;
                            begin_sample();
                        }
                    }
                    // a pixel of another shard or a masked one: the lane asks again on the next trip
                }
            }
        }
        {
            unsigned long long hb = __ballot(mode == MODE_HUGE);
            while (hb) {
                const int src = __builtin_ctzll(hb);
                const Closest r = closest_triangle_wave(P.dm, v3(__shfl(L.p.x, src), __shfl(L.p.y, src), __shfl(L.p.z, src)));
                if (lane == src) {
                    T.best = r;
                    mode = MODE_WAIT;
                }
                hb &= hb - 1;
            }
        }
        if (WAVE) {
            const bool asks = mode == MODE_QUERY;
            if (__ballot(asks)) {
                const Closest r = closest_triangle_pool(P.dm, L.p, T.best, asks, W, stk, P.cp_slot_trigger);
                if (asks) {
                    T.best = r;
                    mode = MODE_WAIT;
                }
            }
        }
        const int n_trav = __popcll(__ballot(mode == MODE_TRAV));
        const int n_wait = __popcll(__ballot(mode == MODE_WAIT));
        if (n_trav + n_wait == 0) {
            if (__ballot(mode == MODE_REFILL)) continue;
            break;
        }
        PROF3_T0();
        if (n_wait * P.wait_weight >= n_trav * 8) {
#ifdef WOST3_PROFILE
            if (lane == 0) { atomicAdd(&g_prof3[8], 1ull); atomicAdd(&g_prof3[9], (unsigned long long)n_wait); }
#endif
            const bool stepping = mode == MODE_WAIT;
            bool ended = false;
            if (stepping && has_d && L.depth == 0 && !L.d0_valid) {
                L.d0 = T.best;
                L.d0_valid = true;
            }
            if (NTREE && P.coop) {
                // the step in its three parts (step3), the two tree queries between them answered by all 64 lanes together
                float R_D = WOST_INF, R_B = 0.0f;
                V3 dir = v3(0.0f, 0.0f, 0.0f), cur = dir;
                bool mid = false, go = false;
                if (stepping) {
                    ended = step3_a(P, L, T.best, R_D);
                    mid = !ended;
                }
                const float R_N = closest_silhouette3_wave(P.nm, L.p, R_D, mid, W, stk);
                // part B around the rays of its samples, those answered by the wave as well (a lane's shadow ray through a tree
                // of its own was the longest wait of an emissive step)
                if ((EMISSIVE || SOURCE) && P.coop > 1) {
                    Step3B B;
                    B.sdir = B.o = B.rd = v3(0.0f, 0.0f, 0.0f);
                    B.R_B = B.cd = 0.0f;
                    if (mid) {
                        ended = step3_b0<SOURCE>(P, L, R_D, R_N, B);
                        go = !ended;
                    }
                    bool src_hit = false, lit = false;
                    float src_t = 0.0f;
                    if (SOURCE) {
                        int shi;
                        src_hit = ray_closest3_wave(P.nm, step3_source_origin(P, L, B), B.sdir, B.R_B, go, src_t, shi, W, stk, P.ray_slot_trigger);
                    }
                    if (go) lit = step3_b1<EMISSIVE, SOURCE, NTREE>(P, L, B, src_hit, src_t);
                    if (EMISSIVE) {
                        float st;
                        int shi;
                        const bool occluded = ray_closest3_wave(P.nm, B.o, B.rd, B.cd - P.st.eps, lit, st, shi, W, stk, P.ray_slot_trigger);
                        lit = lit && !occluded;
                    }
                    if (go) step3_b2<EMISSIVE>(P, L, B, lit, dir, cur);
                    R_B = B.R_B;
                } else if (mid) {
                    // (WOST3_COOP=1: the rays of the samples by the lane itself, as in rounds 3)
                    ended = step3_b<EMISSIVE, SOURCE, NTREE>(P, L, R_D, R_N, stk, R_B, dir, cur);
                    go = !ended;
                }
                float t = 0.0f;
                int hi = -1;
                const bool hit = ray_closest3_wave(P.nm, cur, dir, R_B, go, t, hi, W, stk, P.ray_slot_trigger);
                if (go) step3_c(P, L, R_B, dir, cur, hit, t, hi);
            } else if (stepping) {
                ended = step3<EMISSIVE, SOURCE, NTREE>(P, L, T.best, stk);
            }
            if (stepping) {
                if (!ended) {
                    ++L.depth;
                    if (L.depth == P.st.max_depth) {
                        ++L.c_truncated;
                        ended = true;
                    }
                }
                if (!ended) {
                    begin_step();
                } else if (++L.sample < P.st.spp) {
                    begin_sample();
                } else {
                    float *f = P.field + 3 * (size_t)(L.pid - P.field_base);
                    if (CARRY) {
                        P.carry_rng[L.pid] = L.rng.state;
                        float *cs = P.carry_sum + 3 * (size_t)L.pid;
                        cs[0] = L.sol[0]; cs[1] = L.sol[1]; cs[2] = L.sol[2];
                    }
                    const float spp = (float)(CARRY ? P.carry_total : P.st.spp);
                    f[0] = L.sol[0] / spp; f[1] = L.sol[1] / spp; f[2] = L.sol[2] / spp;
                    mode = MODE_REFILL;
                }
            }
            PROF3(4);
        } else {
            for (int b = 0; b < P.trav_burst; ++b) {
                if (mode == MODE_TRAV) {
                    if (!trav_visit3(P.dm, L.p, T, stk)) mode = MODE_WAIT;
                }
            }
            PROF3(5);
#ifdef WOST3_PROFILE
            if (lane == 0) { atomicAdd(&g_prof3[10], 1ull); atomicAdd(&g_prof3[11], (unsigned long long)n_trav); }
#endif
        }
    }
#ifdef WOST3_PROFILE
    if (lane == 0) atomicAdd(&g_prof3[6], __builtin_readcyclecounter() - prof_begin);
#endif
    t_steps += L.c_steps; t_started += L.c_started; t_absorbed += L.c_absorbed; t_truncated += L.c_truncated; t_nhits += L.c_nhits;
    uint32_t v[5] = {t_steps, t_started, t_absorbed, t_truncated, t_nhits};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        uint32_t x = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
        v[k] = x;
    }
    if (lane == 0) {
        Stats3Dev *st = P.stats + (blockIdx.x & (kStat3Copies - 1));
        if (v[0]) atomicAdd(&st->steps, (unsigned long long)v[0]);
        if (v[1]) atomicAdd(&st->started, (unsigned long long)v[1]);
        if (v[2]) atomicAdd(&st->absorbed, (unsigned long long)v[2]);
        if (v[3]) atomicAdd(&st->truncated, (unsigned long long)v[3]);
        if (v[4]) atomicAdd(&st->nhits, (unsigned long long)v[4]);
    }
}

// ---- batch queries (tests, SDF-style renders) ----------------------------------------------------
__global__ __launch_bounds__(256) void closest_point3_kernel(DevMesh3 m, const float *pts, int n, int32_t *out_idx, float *out_dist,
                                                             float *out_uv, int32_t *out_side)
{
    extern __shared__ uint32_t lds_stack[];
    const LdsColumn stk(lds_stack + threadIdx.x, blockDim.x);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 q = v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    const Closest cp = closest_triangle(m, q, -1, stk);
    float u, v;
    int32_t side;
    triangle_uv_side(m, cp.slot, q, u, v, side);
    if (out_idx) out_idx[i] = m.triOrig[cp.slot];
    if (out_dist) out_dist[i] = sqrtf(cp.d2);
    if (out_uv) {
        out_uv[2 * i] = u;
        out_uv[2 * i + 1] = v;
    }
    if (out_side) out_side[i] = side;
}

// debug channels at the evaluation points of the frame
__global__ __launch_bounds__(256) void render3_sdf_kernel(DevMesh3 m, DevProbe3 probe, int width, int height, int silhouette, float *out)
{
    extern __shared__ uint32_t lds_stack[];
    const LdsColumn stk(lds_stack + threadIdx.x, blockDim.x);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width * height) return;
    const V3 q = eval_point3(probe, i % width, i / width, width, height);
    float d = WOST_INF;
    if (m.n_tris > 0) {
        if (!silhouette) d = sqrtf(closest_triangle(m, q, -1, stk).d2);
        else d = m.n_tris > WOST3_FLAT_MAX ? closest_silhouette3_tree(m, q, WOST_INF, stk) : closest_silhouette3_flat(m, q, WOST_INF);
    }
    out[i] = d;
}

__global__ __launch_bounds__(256) void render3_source_kernel(DevSource3 src, DevProbe3 probe, int width, int height, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width * height) return;
    float f[3] = {0.0f, 0.0f, 0.0f};
    if (src.rgb) source3_eval(src, eval_point3(probe, i % width, i / width, width, height), f);
    out[3 * (size_t)i] = f[0]; out[3 * (size_t)i + 1] = f[1]; out[3 * (size_t)i + 2] = f[2];
}

template <bool NTREE>
__global__ __launch_bounds__(256) void silhouette3_kernel(DevMesh3 m, const float *pts, const float *rmax, int n, float *out)
{
    extern __shared__ uint32_t lds_stack[];
    const LdsColumn stk(lds_stack + threadIdx.x, blockDim.x);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = m.n_tris > 0 ? closest_silhouette3<NTREE>(m, v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), rmax ? rmax[i] : WOST_INF, stk) : WOST_INF;
}

template <bool NTREE>
__global__ __launch_bounds__(256) void ray3_kernel(DevMesh3 m, const float *o, const float *d, const float *tmax, int n, int32_t *out_hit,
                                                   float *out_t, int32_t *out_idx)
{
    extern __shared__ uint32_t lds_stack[];
    const LdsColumn stk(lds_stack + threadIdx.x, blockDim.x);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float t;
    int idx;
    const bool hit = ray_closest3<NTREE>(m, v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), tmax[i], t, idx, stk);
    out_hit[i] = hit ? 1 : 0;
    out_t[i] = t;
    out_idx[i] = idx;
}

}  // namespace wost

using namespace wost;

static void destroy3(wost3_context *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (void *p : c->dm.allocs) (void)hipFree(p);
    for (void *p : c->nm.allocs) (void)hipFree(p);
    if (c->src.rgb) (void)hipFree(const_cast<float *>(c->src.rgb));
    if (c->stats) (void)hipFree(c->stats);
    if (c->cursor) (void)hipFree(c->cursor);
    destroy_base(c);
    delete c;
}

// ---- the solve driver.  Everything that is fixed for one solve of n pixels: walk3_plan() fills it once per solve and is the only place that reads the
// driver's environment switches -- at solve time, not at handle creation: they may change between two solves on one handle.
struct Walk3Plan {
    bool emissive, source, ntree, wave;      // walk3_kernel's template arguments; wave: the closest-point queries by the wave as well (WOST3_WAVE=0: the lane machine)
    // Neumann mesh on the tree: its silhouette and ray queries are answered by the wave as a whole, through task pools in LDS behind the stack
    // columns.  coop 2: the rays of the source and boundary samples through the pools as well (1: by the lane, 0: the per-lane queries)
    int coop, pool_cap, ray_slot_trigger, cp_slot_trigger;      // WOST3_COOP / POOL_CAP / RAY_TRIGGER / CP_TRIGGER
    int wait_weight, trav_burst;             // WOST3_WAIT_WEIGHT / TRAV_BURST
    int stack_words; size_t lds;             // the stack columns of a block, in words; its LDS, the pools included
    unsigned grid;                           // persistent blocks (WOST3_BLOCKS_PER_CU, WOST3_MAX_BLOCKS)
};

static Walk3Plan walk3_plan(const wost3_context *c, int n)
{
    const int bs = kWalk3Threads, big = INT_MAX;
    const int lv = std::max(c->dm.view.n_tris > 0 ? c->dm.view.levels : 1, c->nm.view.n_tris > 0 ? c->nm.view.levels : 1);
    Walk3Plan pl{};
    pl.emissive = c->nm.view.n_tris > 0 && c->nm.view.emissive; pl.source = c->src.rgb != nullptr; pl.ntree = c->nm.view.n_tris > WOST3_FLAT_MAX;
    // a step that answers its Neumann queries on the tree is long and divergent: it waits until eight ninths of the
    // busy walkers of the wave stand at it (tools/probes/bench3d_shell.py: 1.8x over the Dirichlet-only setting on a 1280-triangle shell)
    pl.wait_weight = env_int("WOST3_WAIT_WEIGHT", pl.ntree ? 1 : c->wait_weight, 1, big);
    pl.trav_burst = env_int("WOST3_TRAV_BURST", c->trav_burst, 1, big);
    pl.cp_slot_trigger = env_int("WOST3_CP_TRIGGER", 64, 1, 64);
    pl.ray_slot_trigger = env_int("WOST3_RAY_TRIGGER", 32, 1, 64);
    pl.pool_cap = env_int("WOST3_POOL_CAP", 512, 96, 4096);      // (64 roots must fit)
    pl.coop = pl.ntree ? env_int("WOST3_COOP", 2, 0, 2) : 0;
    if (c->nm.view.levels > 11) pl.coop = 0;      // (node and slot indices of a task: 26 bits, 4^(levels + 1) slots)
    pl.wave = c->dm.view.n_tris > 0 && c->dm.view.levels <= 11 && env_int("WOST3_WAVE", 1, -big, big) != 0;
    pl.stack_words = (3 * lv + 1) * bs;
    pl.lds = (size_t)pl.stack_words * sizeof(uint32_t);
    const size_t lds_pools = pool3_lds_bytes(bs / 64, pl.pool_cap);
    if (pl.lds + lds_pools > 64 * 1024) { pl.wave = false; pl.coop = 0; }      // (trees of millions of triangles: the stack columns alone fill the block's LDS)
    if (pl.wave || pl.coop) pl.lds += lds_pools;
    // persistent blocks: as many as the chip holds (LDS stacks and registers allow about four per CU), or fewer for small frames
    int n_cus = 256;
    (void)hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, c->device);
    pl.grid = (unsigned)std::min((n + bs - 1) / bs, n_cus * env_int("WOST3_BLOCKS_PER_CU", 4, 1, big));
    // developer knob for tests: at most this many blocks, so that every lane takes many pixels one after another (refills)
    if (const int cap = env_int("WOST3_MAX_BLOCKS", 0, 0, big)) pl.grid = std::min(pl.grid, (unsigned)cap);
    return pl;
}

// the kernel of the solve: all sixteen walk3_kernel<EMISSIVE, SOURCE, NTREE, WAVE> there are, the sixteen of a point solve, the
// sixteen of a continued frame solve and the sixteen of a call on a carried point list beside them
template <bool E, bool S, bool PTS, bool CARRY>
static const void *walk3_kernel_of(bool ntree, bool wave)
{
    if (ntree) return wave ? reinterpret_cast<const void *>(walk3_kernel<E, S, true, true, PTS, CARRY>) : reinterpret_cast<const void *>(walk3_kernel<E, S, true, false, PTS, CARRY>);
    return wave ? reinterpret_cast<const void *>(walk3_kernel<E, S, false, true, PTS, CARRY>) : reinterpret_cast<const void *>(walk3_kernel<E, S, false, false, PTS, CARRY>);
}
template <bool PTS, bool CARRY = false>
static const void *walk3_kernel_of(const Walk3Plan &pl)
{
    if (pl.emissive) return pl.source ? walk3_kernel_of<true, true, PTS, CARRY>(pl.ntree, pl.wave) : walk3_kernel_of<true, false, PTS, CARRY>(pl.ntree, pl.wave);
    return pl.source ? walk3_kernel_of<false, true, PTS, CARRY>(pl.ntree, pl.wave) : walk3_kernel_of<false, false, PTS, CARRY>(pl.ntree, pl.wave);
}

// The first step of a solve, what a lane's refill reads: the pixels [pixel_begin, pixel_end) of the frame and a shard of its tiles, or
// (points != nullptr) the points [pixel_begin, pixel_end) of a caller's list with their seeds.
// A frame step with carry_more > 0 is a call of a continued solve (wost3_solve_more & co.): carry_more samples on top of those in
// the handle's carried buffers -- the launch runs with spp = carry_more, whatever the handle's own setting -- on the carry_n_ids
// pixels of the device list carry_ids (nullptr: every pixel of the shard).  A point step with carry_more > 0 is the same on the
// handle's carried point list (wost3_points_more & co.): the buffers are the list's, the ids are indices into the list.
struct FirstStep3 {
    int32_t pixel_begin, pixel_end, shard_index, shard_count;
    const float *points;
    int32_t seed_base, seed_width;
    int32_t carry_done = 0, carry_more = 0;
    const int32_t *carry_ids = nullptr;
    int32_t carry_n_ids = 0;
    int32_t spp = 0;         // > 0: the samples of a step that carries nothing, whatever the handle's setting (the walks of a gradient call: one each)
};

static int run_solve3(wost3_context *c, const FirstStep3 &fs, float *field_dev, int32_t field_base, hipStream_t stream, wost_stats *stats)
{
    const int32_t pixel_begin = fs.pixel_begin, pixel_end = fs.pixel_end, shard_index = fs.shard_index, shard_count = fs.shard_count;
    const auto t0 = std::chrono::high_resolution_clock::now();
    WOST_TRY(hipSetDevice(c->device));
    WOST_TRY(hipMemsetAsync(c->stats, 0, kStat3Copies * sizeof(Stats3Dev), stream));
    WOST_TRY(hipMemsetAsync(c->cursor, 0, sizeof(uint32_t), stream));
    // (the lanes a launch needs: those of the selection where a continued call has one)
    const int n = fs.carry_more > 0 && fs.carry_ids ? fs.carry_n_ids : pixel_end - pixel_begin;
    float ms = 0.0f;
    if (n > 0) {
        const Walk3Plan pl = walk3_plan(c, n);
        Walk3Params P{};
        P.dm = c->dm.view; P.nm = c->nm.view; P.st = c->dst; P.probe = c->probe; P.mask = c->mask; P.src = c->src;
        P.field = field_dev; P.field_base = field_base; P.pixel_begin = pixel_begin; P.pixel_end = pixel_end;
        P.shard_index = shard_index; P.shard_count = shard_count; P.stats = c->stats; P.cursor = c->cursor;
        P.tiled = (!fs.points && pixel_begin == 0 && pixel_end == (int32_t)c->n_pixels && ((c->settings.width | c->settings.height) & 7) == 0) ? 1 : 0;
        P.points = fs.points; P.seed_base = fs.seed_base; P.seed_width = fs.seed_width;
        const bool carried = fs.carry_more > 0;
        if (!carried && fs.spp > 0) P.st.spp = fs.spp;
        if (carried) {
            const CarryState &cs = fs.points ? c->list.carry : c->carry;
            P.st.spp = fs.carry_more;
            P.carry_rng = cs.rng; P.carry_sum = cs.sum; P.carry_done = fs.carry_done; P.carry_total = fs.carry_done + fs.carry_more;
            P.carry_n = cs.n; P.ids = fs.carry_ids; P.n_ids = fs.carry_n_ids;
        }
        P.wait_weight = pl.wait_weight; P.trav_burst = pl.trav_burst; P.coop = pl.coop; P.pool_cap = pl.pool_cap; P.stack_words = pl.stack_words;
        P.ray_slot_trigger = pl.ray_slot_trigger; P.cp_slot_trigger = pl.cp_slot_trigger;
        void *args[] = {&P};
        WOST_TRY(hipEventRecord(c->ev0, stream));
        (void)hipLaunchKernel(fs.points ? (carried ? walk3_kernel_of<true, true>(pl) : walk3_kernel_of<true>(pl)) : carried ? walk3_kernel_of<false, true>(pl) : walk3_kernel_of<false>(pl), dim3(pl.grid), dim3(kWalk3Threads), args, pl.lds, stream);
        WOST_TRY(hipGetLastError());
        WOST_TRY(hipEventRecord(c->ev1, stream));
    }
    std::vector<Stats3Dev> copies(kStat3Copies);
    WOST_TRY(hipMemcpyAsync(copies.data(), c->stats, kStat3Copies * sizeof(Stats3Dev), hipMemcpyDeviceToHost, stream));
    WOST_TRY(hipStreamSynchronize(stream));
    if (n > 0) WOST_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
#ifdef WOST3_PROFILE
    {
        unsigned long long prof[16], zero[16] = {0};
        WOST_TRY(hipMemcpyFromSymbol(prof, HIP_SYMBOL(g_prof3), sizeof(prof)));
        WOST_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_prof3), zero, sizeof(zero)));
        std::fprintf(stderr, "[wost3 profile] wave cycles: silhouette %llu source %llu neumann-sample %llu walk-ray %llu | step trips %llu (cycles %llu, lanes %llu) trav trips %llu (cycles %llu, lanes %llu) | kernel total %llu, %.1f ms\n",
                     prof[0], prof[1], prof[2], prof[3], prof[8], prof[4], prof[9], prof[10], prof[5], prof[11], prof[6], ms);
        std::fprintf(stderr, "[wost3 profile] silhouette queries %llu: inner visits %llu, leaf visits %llu\n", prof[14], prof[12], prof[13]);
    }
#endif
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        for (const Stats3Dev &k : copies) {
            stats->walk_steps += k.steps; stats->walks_started += k.started; stats->walks_absorbed += k.absorbed;
            stats->walks_truncated += k.truncated; stats->neumann_hits += k.nhits;
        }
        stats->kernel_ms = ms;
        stats->kernel_launches = n > 0 ? 1 : 0;
        stats->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
    }
    return WOST_OK;
}

// ---- the frame and point solves (the bodies of the entry points: UniformCalls, wost_uniform.h) ----
static int frame_solve3(wost3_context *c, int32_t pixel_begin, int32_t pixel_end, int32_t shard_index, int32_t shard_count, float *field_dev,
                        int32_t field_base, hipStream_t stream, wost_stats *stats)
{
    return run_solve3(c, FirstStep3{pixel_begin, pixel_end, shard_index, shard_count, nullptr, 0, 0}, field_dev, field_base, stream, stats);
}
// (one launch, however long the list)
static int point_solve3(wost3_context *c, const float *pts_dev, int32_t n, int32_t seed_base, int32_t seed_width, float *field_dev, hipStream_t stream,
                        wost_stats *stats)
{
    return run_solve3(c, FirstStep3{0, n, 0, 1, pts_dev, seed_base, seed_width}, field_dev, 0, stream, stats);
}

static const UniformCalls<wost3_context> kUniform3{3, frame_solve3, point_solve3};

// ---- the continued frame solve (wost_solve_more & co. in 3-D: the same drivers, wost_carry.hip, and the same bodies of the
// entry points, CarryCalls of wost_carry.h) ----
// a walk of the carried solve: one launch, its lanes on the pixels of the id list where the call has a selection
static CarryWalk carry_walk3(wost3_context *c, int32_t shard_index, int32_t shard_count)
{
    return [c, shard_index, shard_count](int32_t more_spp, const uint8_t *sel, const int32_t *ids, uint32_t n_sel, float *field_dev, hipStream_t stream,
                                         wost_stats *stats) {
        FirstStep3 fs{0, (int32_t)c->n_pixels, shard_index, shard_count, nullptr, 0, 0};
        fs.carry_done = c->carry.done; fs.carry_more = more_spp;
        if (sel) { fs.carry_ids = ids; fs.carry_n_ids = (int32_t)n_sel; }
        return run_solve3(c, fs, field_dev, 0, stream, stats);
    };
}

static const CarryCalls<wost3_context> kCarry3{"wost3_", carry_walk3, nullptr};

// ---- the carried point list (wost3_points_carry & co.; the bodies of the entry points: PointCalls, wost_carry.h) ----
// a walk of the list: one launch, its lanes on the points of the id list where the call has a selection
static CarryWalk points_walk3(PointListCtx<wost3_context> *x, int32_t, int32_t)
{
    wost3_context *c = x->h;
    return [c](int32_t more_spp, const uint8_t *sel, const int32_t *ids, uint32_t n_sel, float *field_dev, hipStream_t stream, wost_stats *stats) {
        const PointList &l = c->list;
        FirstStep3 fs{0, l.n, 0, 1, l.pts, l.seed_base, l.seed_width};
        fs.carry_done = l.carry.done; fs.carry_more = more_spp;
        if (sel) { fs.carry_ids = ids; fs.carry_n_ids = (int32_t)n_sel; }
        return run_solve3(c, fs, field_dev, 0, stream, stats);
    };
}

static const PointCalls<wost3_context> kPoints3{{"wost3_points_", points_walk3, nullptr}, 3};

// ---- the gradient at the caller's points (the driver and its kernels: wost_grad.hip; the body of the entry points: grad_entry) ----
// what the 3-D context adds: the kernel in front on its meshes, a point step of one sample per walk, and the in-ball kernel on
// its source grid
static GradCall grad_call3(wost3_context *c)
{
    GradCall g{"wost3_", 3, c->device, c->dst.spp, c->n_pixels, c->dst.eps, c->src.rgb != nullptr, c->grad_source, c->stream, &c->grad, nullptr, nullptr,
               nullptr};
    g.prep = [c](const GradPrep &p, hipStream_t stream) { return grad_prep3(c->dm.view, c->nm.view, p, stream); };
    g.walk = [c](const float *first_pts, int32_t n_walks, int32_t seed_base, int32_t seed_width, float *w_rgb, hipStream_t stream, wost_stats *stats) {
        FirstStep3 fs{0, n_walks, 0, 1, first_pts, seed_base, seed_width};
        fs.spp = 1;
        return run_solve3(c, fs, w_rgb, 0, stream, stats);
    };
    g.ball = [c](const GradBall &p, hipStream_t stream) { return grad_ball3(c->src, p, stream); };
    return g;
}

// ---- the carried gradient list (wost3_gradient_points_carry & co.; the bodies of the entry points: GradListCalls, wost_grad.h) ----
static const GradListCalls<wost3_context> kGradList3{grad_call3, 3};

// ---- what wost3_create adds to the shared part (create_handle, wost_uniform.h): the probe, the meshes, the source grid and the
// counters of the one launch ----
static int fill3(wost3_context *c, const wost3_scene_desc &scene)
{
    c->probe.scale = scene.probe_scale;
    for (int k = 0; k < 3; ++k) { c->probe.pos[k] = scene.probe_pos[k]; c->probe.up[k] = scene.probe_up[k]; c->probe.right[k] = scene.probe_right[k]; }
    int rc = upload_mesh3(scene.dirichlet, c->dm);
    if (rc == WOST_OK) rc = upload_mesh3(scene.neumann, c->nm);
    if (rc == WOST_OK) rc = upload_mask(c, scene.mask);
    if (rc != WOST_OK) return rc;
    c->dirichlet_verts = scene.dirichlet.n_tris > 0 ? scene.dirichlet.n_verts : 0;
    if (scene.source.nx > 0) {
        const wost3_source_desc &sd = scene.source;
        if (sd.ny <= 0 || sd.nz <= 0 || !sd.rgb) return set_error(WOST_ERR_INVALID, "source grid: bad size or null samples");
        const size_t bytes = (size_t)sd.nx * sd.ny * sd.nz * 3 * sizeof(float);
        float *d = nullptr;
        WOST_TRY(hipMalloc((void **)&d, bytes));
        c->src = DevSource3{d, sd.nx, sd.ny, sd.nz, sd.index_scale[0], sd.index_scale[1], sd.index_scale[2], sd.index_offset[0],
                            sd.index_offset[1], sd.index_offset[2], sd.intensity};
        WOST_TRY(hipMemcpy(d, sd.rgb, bytes, hipMemcpyHostToDevice));
    }
    if ((rc = create_frame(c)) != WOST_OK) return rc;
    WOST_TRY(hipMalloc((void **)&c->stats, kStat3Copies * sizeof(Stats3Dev)));
    WOST_TRY(hipMalloc((void **)&c->cursor, sizeof(uint32_t)));
    return WOST_OK;
}

// ---- the launches of the batch queries (their bodies: query_*, wost_uniform.h).  The silhouette and ray queries of a Neumann
// mesh above the flat limit descend its tree (NTREE); render_sdf tells the kernel which of the two distances it renders ----
namespace {
struct Query3 {
    static constexpr int dim = 3, uv = 2;
    static int32_t count(const DevMesh3 &m) { return m.n_tris; }
    static dim3 grid(int n) { return dim3((n + 255) / 256); }
    static void closest_point(wost3_context *h, const DevMesh3 &m, size_t lds, const float *pts, int n, int32_t *idx, float *dist, float *uv, int32_t *side)
    {
        hipLaunchKernelGGL(closest_point3_kernel, grid(n), dim3(256), lds, h->stream, m, pts, n, idx, dist, uv, side);
    }
    static void silhouette(wost3_context *h, const DevMesh3 &m, size_t lds, const float *pts, const float *rmax, int n, float *out)
    {
        if (m.n_tris > WOST3_FLAT_MAX) hipLaunchKernelGGL((silhouette3_kernel<true>), grid(n), dim3(256), lds, h->stream, m, pts, rmax, n, out);
        else hipLaunchKernelGGL((silhouette3_kernel<false>), grid(n), dim3(256), lds, h->stream, m, pts, rmax, n, out);
    }
    static void ray(wost3_context *h, const DevMesh3 &m, size_t lds, const float *o, const float *d, const float *tmax, int n, int32_t *hit, float *t,
                    int32_t *idx)
    {
        if (m.n_tris > WOST3_FLAT_MAX) hipLaunchKernelGGL((ray3_kernel<true>), grid(n), dim3(256), lds, h->stream, m, o, d, tmax, n, hit, t, idx);
        else hipLaunchKernelGGL((ray3_kernel<false>), grid(n), dim3(256), lds, h->stream, m, o, d, tmax, n, hit, t, idx);
    }
    static hipError_t sdf_out(wost3_context *, Batch &b, int n, float **out) { return b.out(out, n); }
    static void sdf(wost3_context *h, const DevMesh3 &m, int which_mesh, size_t lds, int n, float *out)
    {
        hipLaunchKernelGGL(render3_sdf_kernel, grid(n), dim3(256), lds, h->stream, m, h->probe, h->settings.width, h->settings.height,
                           which_mesh == WOST_MESH_NEUMANN ? 1 : 0, out);
    }
    static void source(wost3_context *h, int n, float *out)
    {
        hipLaunchKernelGGL(render3_source_kernel, grid(n), dim3(256), 0, h->stream, h->src, h->probe, h->settings.width, h->settings.height, out);
    }
};
}  // namespace

extern "C" {

int wost3_points_carry(wost3_handle h, const float *pts_xyz, int32_t n, int32_t seed_base, int32_t seed_width)
{
    return kPoints3.bind(h, pts_xyz, true, n, seed_base, seed_width, nullptr);
}

int wost3_points_carry_dev(wost3_handle h, const float *pts_xyz_dev, int32_t n, int32_t seed_base, int32_t seed_width, void *stream)
{
    return kPoints3.bind(h, pts_xyz_dev, false, n, seed_base, seed_width, stream);
}

int wost3_points_more(wost3_handle h, int32_t more_spp, const uint8_t *select, float *field_rgb, wost_stats *stats)
{
    return kPoints3.more(h, more_spp, select, field_rgb, stats);
}

int wost3_points_more_dev(wost3_handle h, int32_t more_spp, const uint8_t *select_dev, float *field_rgb_dev, void *stream, wost_stats *stats)
{
    return kPoints3.more_dev(h, more_spp, select_dev, field_rgb_dev, stream, stats);
}

int wost3_points_carried(wost3_handle h, int32_t *spp, int32_t *batches, float *sum_rgb, float *stderr_rgb)
{
    return kPoints3.carried(h, spp, batches, sum_rgb, stderr_rgb);
}

int wost3_points_adaptive(wost3_handle h, const wost_adaptive *a, float *field_rgb, float *stderr_rgb, int32_t *spp_map, wost_stats *stats)
{
    return kPoints3.adaptive(h, a, field_rgb, stderr_rgb, spp_map, stats);
}

int wost3_points_adaptive_dev(wost3_handle h, const wost_adaptive *a, float *field_rgb_dev, void *stream, wost_stats *stats)
{
    return kPoints3.adaptive_dev(h, a, field_rgb_dev, stream, stats);
}

int wost3_points_restart(wost3_handle h) { return kPoints3.restart(h); }

int wost3_points_progress(wost3_handle h, int32_t *n_points, int32_t *spp_done) { return kPoints3.progress(h, n_points, spp_done); }

int wost3_create(const wost3_scene_desc *scene, const wost_settings *settings, int device, wost3_handle *out)
{
    return create_handle(scene, settings, device, out, false, destroy3, fill3);
}

int wost3_destroy(wost3_handle h)
{
    destroy3(h);
    return WOST_OK;
}

int wost3_set_option(wost3_handle h, const char *key, double value)
{
    if (!h || !key) return set_error(WOST_ERR_INVALID, "null argument");
    const std::string k(key);
    if (k == "grad_source") return grad_source_option(value, &h->grad_source);
    if (k == "exits_grad_source") return exits_grad_source_option(value, &h->exits_grad_source);
    return set_error(WOST_ERR_INVALID, "unknown option: " + k);
}

int wost3_solve(wost3_handle h, int32_t pixel_begin, int32_t pixel_end, float *field_rgb, wost_stats *stats)
{
    return kUniform3.solve(h, pixel_begin, pixel_end, field_rgb, stats);
}

int wost3_solve_sharded(wost3_handle h, int32_t shard_index, int32_t shard_count, float *field_rgb_dev, void *stream, wost_stats *stats)
{
    return kUniform3.solve_sharded(h, shard_index, shard_count, field_rgb_dev, stream, stats);
}

int wost3_solve_more_where(wost3_handle h, int32_t more_spp, const uint8_t *select, float *field_rgb, wost_stats *stats)
{
    return kCarry3.more_where(h, more_spp, select, field_rgb, stats);
}

int wost3_solve_more(wost3_handle h, int32_t more_spp, float *field_rgb, wost_stats *stats)
{
    return kCarry3.more_where(h, more_spp, nullptr, field_rgb, stats);
}

int wost3_solve_more_where_sharded(wost3_handle h, int32_t shard_index, int32_t shard_count, int32_t more_spp, const uint8_t *select_dev,
                                   float *field_rgb_dev, void *stream, wost_stats *stats)
{
    return kCarry3.more_where_sharded(h, shard_index, shard_count, more_spp, select_dev, field_rgb_dev, stream, stats);
}

int wost3_solve_more_sharded(wost3_handle h, int32_t shard_index, int32_t shard_count, int32_t more_spp, float *field_rgb_dev, void *stream,
                             wost_stats *stats)
{
    return kCarry3.more_where_sharded(h, shard_index, shard_count, more_spp, nullptr, field_rgb_dev, stream, stats);
}

int wost3_solve_adaptive_sharded(wost3_handle h, int32_t shard_index, int32_t shard_count, const wost_adaptive *a, float *field_rgb_dev, void *stream,
                                 wost_stats *stats)
{
    return kCarry3.adaptive_sharded(h, shard_index, shard_count, a, field_rgb_dev, stream, stats);
}

int wost3_solve_adaptive(wost3_handle h, const wost_adaptive *a, float *field_rgb, float *stderr_rgb, int32_t *spp_map, wost_stats *stats)
{
    return kCarry3.adaptive(h, a, field_rgb, stderr_rgb, spp_map, stats);
}

int wost3_solve_carried(wost3_handle h, int32_t *spp, int32_t *batches, float *sum_rgb, float *stderr_rgb)
{
    return kCarry3.carried(h, spp, batches, sum_rgb, stderr_rgb);
}

int wost3_solve_restart(wost3_handle h) { return kCarry3.restart(h); }

int wost3_solve_progress(wost3_handle h, int32_t *spp_done) { return kCarry3.progress(h, spp_done); }

int wost3_solve_points_dev(wost3_handle h, const float *pts_xyz_dev, int32_t n, int32_t seed_base, int32_t seed_width, float *field_rgb_dev,
                           void *stream, wost_stats *stats)
{
    return kUniform3.solve_points_dev(h, pts_xyz_dev, n, seed_base, seed_width, field_rgb_dev, stream, stats);
}

int wost3_solve_points(wost3_handle h, const float *pts_xyz, int32_t n, int32_t seed_base, int32_t seed_width, float *field_rgb, wost_stats *stats)
{
    return kUniform3.solve_points(h, pts_xyz, n, seed_base, seed_width, field_rgb, stats);
}

int wost3_solve_gradient_points(wost3_handle h, const float *pts_xyz, int32_t n, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width,
                                const wost_gradient_out *out, wost_stats *stats)
{
    return grad_entry(h, grad_call3, 3, pts_xyz, true, n, seed_base, walk_seed_base, seed_width, out, nullptr, stats);
}

int wost3_solve_gradient_points_dev(wost3_handle h, const float *pts_xyz_dev, int32_t n, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width,
                                    const wost_gradient_out *out, void *stream, wost_stats *stats)
{
    return grad_entry(h, grad_call3, 3, pts_xyz_dev, false, n, seed_base, walk_seed_base, seed_width, out, stream, stats);
}

int wost3_gradient_points_carry(wost3_handle h, const float *pts_xyz, int32_t n, int32_t batch_walks, int32_t round_stride, int32_t max_rounds,
                                int32_t seed_base, int32_t walk_seed_base, int32_t seed_width)
{
    return kGradList3.bind(h, pts_xyz, true, n, batch_walks, round_stride, max_rounds, seed_base, walk_seed_base, seed_width, nullptr);
}

int wost3_gradient_points_carry_dev(wost3_handle h, const float *pts_xyz_dev, int32_t n, int32_t batch_walks, int32_t round_stride, int32_t max_rounds,
                                    int32_t seed_base, int32_t walk_seed_base, int32_t seed_width, void *stream)
{
    return kGradList3.bind(h, pts_xyz_dev, false, n, batch_walks, round_stride, max_rounds, seed_base, walk_seed_base, seed_width, stream);
}

int wost3_gradient_points_more(wost3_handle h, const uint8_t *select, const wost_gradient_carried_out *out, wost_stats *stats)
{
    return kGradList3.more(h, select, true, out, nullptr, stats);
}

int wost3_gradient_points_more_dev(wost3_handle h, const uint8_t *select_dev, const wost_gradient_carried_out *out_dev, void *stream, wost_stats *stats)
{
    return kGradList3.more(h, select_dev, false, out_dev, stream, stats);
}

int wost3_gradient_points_carried(wost3_handle h, const wost_gradient_carried_out *out) { return kGradList3.carried(h, out); }

int wost3_gradient_points_adaptive(wost3_handle h, const wost_gradient_adaptive *a, const wost_gradient_carried_out *out, wost_stats *stats)
{
    return kGradList3.adaptive(h, a, true, out, nullptr, stats);
}

int wost3_gradient_points_adaptive_dev(wost3_handle h, const wost_gradient_adaptive *a, const wost_gradient_carried_out *out_dev, void *stream,
                                       wost_stats *stats)
{
    return kGradList3.adaptive(h, a, false, out_dev, stream, stats);
}

int wost3_gradient_points_restart(wost3_handle h) { return kGradList3.restart(h); }

int wost3_gradient_points_progress(wost3_handle h, int32_t *n_points, int32_t *rounds_done) { return kGradList3.progress(h, n_points, rounds_done); }

int wost3_closest_point(wost3_handle h, int which_mesh, const float *pts, int32_t n, int32_t *out_idx, float *out_dist, float *out_uv,
                        int32_t *out_side)
{
    return query_closest_point<Query3>(h, which_mesh, pts, n, out_idx, out_dist, out_uv, out_side);
}

int wost3_closest_silhouette(wost3_handle h, int which_mesh, const float *pts, const float *rmax, int32_t n, float *out_dist)
{
    return query_closest_silhouette<Query3>(h, which_mesh, pts, rmax, n, out_dist);
}

int wost3_render_sdf(wost3_handle h, int which_mesh, float *out_dist) { return query_render_sdf<Query3>(h, which_mesh, out_dist); }

int wost3_render_source(wost3_handle h, float *out_rgb) { return query_render_source<Query3>(h, out_rgb); }

int wost3_ray_intersect(wost3_handle h, int which_mesh, const float *origins, const float *dirs, const float *tmax, int32_t n,
                        int32_t *out_hit, float *out_t, int32_t *out_idx)
{
    return query_ray_intersect<Query3>(h, which_mesh, origins, dirs, tmax, n, out_hit, out_t, out_idx);
}

}  // extern "C"

// ---- the exit list (wost3_exits_walk & co.; the list, apply and adjoint: wost_exits.hip; the bodies of the entry points: ExitCalls) ----
namespace wost {

struct ExitWalk3Params {
    Walk3Params P;       // the scene and the settings as step3 reads them (spp: 1); nothing of the frame, the queue or the carry
    ExitWalk w;
};

// One lane per walk, in lock step to the walk's end, as exits2_kernel: the depth-0 query without a hint, the steps of the
// gradient's kernel in front (closest_triangle_lockstep: the scan by the wave where root_beyond_huge3 finds the boxes of the
// root's children all beyond dm.huge2, the descent otherwise), every later query seeded with the lane's hint as walk3_kernel's begin_step seeds
// it and scanned beyond dm.huge2 (closest_triangle_scan_huge), and between two queries the unchanged step3 with the flags of
// the handle's point solve.  When step3_a absorbs (the lane's absorbed count moves; L.hint is the slot, L.p still the absorbed
// position) the lane forms side, u and v as the batch query reports them (triangle_uv_side) and writes the record.
// (One wave per SIMD asked for, as walk3_kernel: the instantiations take 114 to 133 registers.  The cap of 100 scalar registers:
// with the default of 102 the instantiation with every flag set keeps a private segment of 36 bytes per lane for scalar spills
// that end up in register lanes -- never addressed, but reserved per lane at launch; under the cap every instantiation reports
// none, for 4 to 37 more scalar spills to lanes.)
template <bool EMISSIVE, bool SOURCE, bool NTREE>
__global__ __launch_bounds__(kWalk3Threads, 1) __attribute__((amdgpu_num_sgpr(100))) void exits3_kernel(ExitWalk3Params X)
{
    extern __shared__ uint32_t lds_stack[];
    const LdsColumn stk(lds_stack + threadIdx.x, blockDim.x);
    const Walk3Params &P = X.P;
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool owned = t < X.w.count;
    const int32_t w = X.w.first_walk + (owned ? t : 0);
    const bool has_d = P.dm.n_tris > 0;
    V3 q = v3(0.0f, 0.0f, 0.0f);
    if (owned) q = ld3(X.w.pts + 3 * (size_t)(w / X.w.S));
    const bool finite = isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
    bool alive = owned && finite;
    Lane3 L{};
    L.rng = Pcg{0, 1};
    if (alive) pcg_seed_pixel(L.rng, X.w.walk_seed_base + w, X.w.seed_width);
    L.p_eval = q; L.p = q;
    L.thp = 1.0f;
    L.hint = L.hint0 = -1;
    L.c_started = alive ? 1u : 0u;
    // the record: a walk that is not absorbed keeps slot -1 and its final sums, a point that is not finite NaN
    int32_t slot = -1, side = 0;
    float u = finite ? 0.0f : __int_as_float(0x7fc00000), v = u, thp = u, base[3] = {u, u, u};
    // ---- the closest Dirichlet triangle of the evaluation point: no hint ----
    // (closest_triangle_lockstep, written out: through the call two instantiations come out of register allocation with a
    // private segment or a wave per SIMD less -- EXPERIMENTS 51)
    Trav T = trav_begin(Closest{WOST_INF, -1});
    bool huge = false;
    if (alive && has_d) {
        huge = root_beyond_huge3(P.dm, q);
        if (!huge) {
            while (trav_visit3(P.dm, q, T, stk)) {
            }
        }
    }
    unsigned long long hb = __ballot(huge);
    while (hb) {
        const int src = __builtin_ctzll(hb);
        const Closest r = closest_triangle_wave(P.dm, v3(__shfl(q.x, src), __shfl(q.y, src), __shfl(q.z, src)));
        if (lane == src) T.best = r;
        hb &= hb - 1;
    }
    while (__ballot(alive)) {
        // ---- the step ----
        if (alive) {
            thp = L.thp;
#pragma unroll
            for (int k = 0; k < 3; ++k) base[k] = L.sol[k];
            ++L.c_steps;
            const uint32_t absorbed_before = L.c_absorbed;
            bool ended = step3<EMISSIVE, SOURCE, NTREE>(P, L, T.best, stk);
            if (L.c_absorbed != absorbed_before) {
                slot = L.hint;
                triangle_uv_side(P.dm, slot, L.p, u, v, side);
            } else {
                if (!ended) {
                    ++L.depth;
                    if (L.depth == P.st.max_depth) {
                        ++L.c_truncated;
                        ended = true;
                    }
                }
                if (ended) {
                    thp = L.thp;
#pragma unroll
                    for (int k = 0; k < 3; ++k) base[k] = L.sol[k];
                }
            }
            if (ended) alive = false;
        }
        // ---- the closest Dirichlet triangle of the next point, seeded with the hint as begin_step seeds it ----
        T = trav_begin(Closest{WOST_INF, -1});
        huge = false;
        if (alive && has_d) {
            if (L.hint >= 0 && P.dm.triOrig[L.hint] != WOST_FAR_INDEX) {
                const float4 a = P.dm.tri[3 * (size_t)L.hint], b = P.dm.tri[3 * (size_t)L.hint + 1], c = P.dm.tri[3 * (size_t)L.hint + 2];
                T.best = Closest{tri_d2(v3(a.x, a.y, a.z), v3(b.x, b.y, b.z), v3(c.x, c.y, c.z), L.p), L.hint};
                T.best_orig = P.dm.triOrig[L.hint];
                huge = T.best.d2 > P.dm.huge2;
            }
            if (!huge) {
                while (trav_visit3(P.dm, L.p, T, stk)) {
                }
            }
        }
        closest_triangle_scan_huge(P.dm, L.p, huge, T.best);
    }
    if (owned) {
        const ExitRecords &R = X.w.rec;
        R.prim()[w] = slot >= 0 ? P.dm.triOrig[slot] : -1;
        R.slot()[w] = slot;
        R.side()[w] = side;
        R.uv(0)[w] = u; R.uv(1)[w] = v;
        R.thp()[w] = thp;
#pragma unroll
        for (int k = 0; k < 3; ++k) R.base(3, k)[w] = base[k];
    }
    wave_add_counters(X.w.counters, L.c_steps, L.c_started, L.c_absorbed, L.c_truncated, L.c_nhits);
}

}  // namespace wost

// what the 3-D context adds: the walk kernel on its meshes and source, with the flags of its point solve (walk3_plan)
static ExitCall exit_call3(wost3_context *c)
{
    ExitCall e{"wost3_", 3, c->device, c->n_pixels, c->stream, &c->exits, c->dm.view.triVerts, c->dirichlet_verts, c->dst.dirichlet_intensity, nullptr};
    e.walk = [c](const ExitWalk &w, hipStream_t stream) {
        const Walk3Plan pl = walk3_plan(c, w.count);
        ExitWalk3Params X{};
        X.P.dm = c->dm.view; X.P.nm = c->nm.view; X.P.st = c->dst; X.P.src = c->src;
        X.P.st.spp = 1;
        X.w = w;
        const dim3 grid((unsigned)((w.count + kWalk3Threads - 1) / kWalk3Threads));
        const size_t lds = (size_t)pl.stack_words * sizeof(uint32_t);
        auto launch = [&](auto E, auto S, auto T) {
            hipLaunchKernelGGL((exits3_kernel<decltype(E)::value, decltype(S)::value, decltype(T)::value>), grid, dim3(kWalk3Threads), lds, stream, X);
        };
        auto with_tree = [&](auto E, auto S) { pl.ntree ? launch(E, S, std::true_type{}) : launch(E, S, std::false_type{}); };
        auto with_src = [&](auto E) { pl.source ? with_tree(E, std::true_type{}) : with_tree(E, std::false_type{}); };
        pl.emissive ? with_src(std::true_type{}) : with_src(std::false_type{});
        WOST_TRY(hipGetLastError());
        return WOST_OK;
    };
    e.prep = [c](const GradPrep &p, hipStream_t stream) { return grad_prep3(c->dm.view, c->nm.view, p, stream); };
    e.eps = c->dst.eps;
    e.has_source = c->src.rgb != nullptr;
    e.source_term = c->exits_grad_source;
    e.ball = [c](const GradBall &p, hipStream_t stream) { return grad_ball3(c->src, p, stream); };
    return e;
}

static const ExitCalls<wost3_context> kExits3{exit_call3, 3};

extern "C" {

int wost3_exits_walk(wost3_handle h, const float *pts_xyz, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width, wost_stats *stats)
{
    return kExits3.walk(h, pts_xyz, true, n, walks, walk_seed_base, seed_width, nullptr, stats);
}

int wost3_exits_walk_dev(wost3_handle h, const float *pts_xyz_dev, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width, void *stream,
                         wost_stats *stats)
{
    return kExits3.walk(h, pts_xyz_dev, false, n, walks, walk_seed_base, seed_width, stream, stats);
}

int wost3_exits_records(wost3_handle h, const wost_exit_records *out) { return kExits3.records(h, out); }

int wost3_exits_apply(wost3_handle h, const float *colors, int32_t K, float *field_rgb, float *stderr_rgb)
{
    return kExits3.apply(h, colors, K, field_rgb, stderr_rgb, true, nullptr);
}

int wost3_exits_apply_dev(wost3_handle h, const float *colors_dev, int32_t K, float *field_rgb_dev, float *stderr_rgb_dev, void *stream)
{
    return kExits3.apply(h, colors_dev, K, field_rgb_dev, stderr_rgb_dev, false, stream);
}

int wost3_exits_adjoint(wost3_handle h, const float *dfield, int32_t K, float *dcolors) { return kExits3.adjoint(h, dfield, K, dcolors, true, nullptr); }

int wost3_exits_adjoint_dev(wost3_handle h, const float *dfield_dev, int32_t K, float *dcolors_dev, void *stream)
{
    return kExits3.adjoint(h, dfield_dev, K, dcolors_dev, false, stream);
}

int wost3_exits_progress(wost3_handle h, int32_t *n_points, int32_t *walks) { return kExits3.progress(h, n_points, walks); }

int wost3_exits_walk_gradient(wost3_handle h, const float *pts_xyz, int32_t n, int32_t walks, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width,
                              wost_stats *stats)
{
    return kExits3.walk_gradient(h, pts_xyz, true, n, walks, ExitSeeds{seed_base, walk_seed_base, seed_width}, nullptr, stats);
}

int wost3_exits_walk_gradient_dev(wost3_handle h, const float *pts_xyz_dev, int32_t n, int32_t walks, int32_t seed_base, int32_t walk_seed_base,
                                  int32_t seed_width, void *stream, wost_stats *stats)
{
    return kExits3.walk_gradient(h, pts_xyz_dev, false, n, walks, ExitSeeds{seed_base, walk_seed_base, seed_width}, stream, stats);
}

int wost3_exits_gradient_records(wost3_handle h, const wost_exit_gradient_records *out) { return kExits3.gradient_records(h, out); }

int wost3_exits_apply_gradient(wost3_handle h, const float *colors, int32_t K, float *grad, float *grad_stderr, float *field_rgb)
{
    return kExits3.apply_gradient(h, colors, K, grad, grad_stderr, field_rgb, true, nullptr);
}

int wost3_exits_apply_gradient_dev(wost3_handle h, const float *colors_dev, int32_t K, float *grad_dev, float *grad_stderr_dev, float *field_rgb_dev,
                                   void *stream)
{
    return kExits3.apply_gradient(h, colors_dev, K, grad_dev, grad_stderr_dev, field_rgb_dev, false, stream);
}

int wost3_exits_gradient_terms(wost3_handle h, double *T, double *seT, double *U) { return kExits3.gradient_terms(h, T, seT, U); }

int wost3_exits_adjoint_gradient(wost3_handle h, const float *dgrad, int32_t K, float *dcolors)
{
    return kExits3.adjoint_gradient(h, dgrad, K, dcolors, true, nullptr);
}

int wost3_exits_adjoint_gradient_dev(wost3_handle h, const float *dgrad_dev, int32_t K, float *dcolors_dev, void *stream)
{
    return kExits3.adjoint_gradient(h, dgrad_dev, K, dcolors_dev, false, stream);
}

int wost3_exits_index(wost3_handle h) { return kExits3.index(h); }

int wost3_exits_index_info(wost3_handle h, int64_t *n_incidences, int64_t *longest_bin) { return kExits3.index_info(h, n_incidences, longest_bin); }

int wost3_exits_index_records(wost3_handle h, int64_t *bin_begin, int32_t *inc) { return kExits3.index_records(h, bin_begin, inc); }

int wost3_exits_adjoint_ordered(wost3_handle h, const float *dfield, int32_t K, float *dcolors)
{
    return kExits3.adjoint_ordered(h, dfield, K, dcolors, true, nullptr);
}

int wost3_exits_adjoint_ordered_dev(wost3_handle h, const float *dfield_dev, int32_t K, float *dcolors_dev, void *stream)
{
    return kExits3.adjoint_ordered(h, dfield_dev, K, dcolors_dev, false, stream);
}

int wost3_exits_adjoint_gradient_ordered(wost3_handle h, const float *dgrad, int32_t K, float *dcolors)
{
    return kExits3.adjoint_gradient_ordered(h, dgrad, K, dcolors, true, nullptr);
}

int wost3_exits_adjoint_gradient_ordered_dev(wost3_handle h, const float *dgrad_dev, int32_t K, float *dcolors_dev, void *stream)
{
    return kExits3.adjoint_gradient_ordered(h, dgrad_dev, K, dcolors_dev, false, stream);
}

}  // extern "C"
