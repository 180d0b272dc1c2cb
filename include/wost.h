/*
 * wost.h -- C-ABI of the MI355X-native Walk-on-Stars hot path (libwost_hip.so).
 *
 * This is the drop-in boundary for the ONE path this repository accelerates: the
 * wavefront walk loop of Elaina's uniform integrator and the snch-lbvh queries it
 * calls.  The reference has no FFI; what `run_expr` touches is the C++ class shape
 * of `UniformIntegrator<2>` / `Problem<2>` (reference exec.cu:77-78,145-215).  The
 * host-side mirror of those classes (elaina_amd/host/) calls only the functions
 * declared here.  Plain pointers and sizes, no C++/torch types, no exceptions
 * across the boundary, caller owns every host buffer, callee owns device memory,
 * one handle per GPU, handles are independent.
 *
 * Every entry point returns WOST_OK (0) or a negative error code; the message of
 * the last error on the calling thread is available from wost_last_error().
 * There is NO CPU fallback: without a usable HIP device wost_create() fails.
 */
#ifndef WOST_H
#define WOST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WOST_OK 0
#define WOST_ERR_INVALID -1      /* bad argument                                 */
#define WOST_ERR_DEVICE -2       /* HIP runtime error / no device                */
#define WOST_ERR_UNSUPPORTED -3  /* valid request this build does not cover      */
#define WOST_ERR_NOMEM -4

/* which mesh a query refers to */
#define WOST_MESH_DIRICHLET 0
#define WOST_MESH_NEUMANN 1

/* Host description of one boundary mesh (2-D polylines).
 * Replaces: lbvh::scene_loader<2> + lbvh::scene<2>(vb,ve,ib,ie) + compute_silhouettes()
 * + build_bvh() (reference core/problem.cu:27-60) and the per-vertex colour pairs of
 * loadVertexColorFileImpl (core/problem.cu:99-133). */
typedef struct wost_mesh_desc {
    int32_t n_verts;
    int32_t n_segs;        /* 0 => this boundary type is disabled (problem.h:104-111)   */
    const float *verts;    /* n_verts * 2, (x, y)                                        */
    const int32_t *segs;   /* n_segs * 2, 0-based (i0, i1); direction p0 -> p1           */
    const float *colors;   /* n_verts * 6: (left r,g,b, right r,g,b); NULL => all zero   */
} wost_mesh_desc;

/* Source term f of  laplace(u) = -f  (SURVEY 8f.2).  Replaces the nanovdb Vec3f grid of
 * Problem<2>::loadSource (core/problem.cu:136-149) as the integrator reads it
 * (worldToIndex + order-1 SampleFromVoxels at z = 0, integrator/uniform/integrator.cu:303-306): a
 * dense 2-D grid of RGB samples at integer index coordinates, index = world * index_scale +
 * index_offset, bilinear, zero outside.  nx == 0 disables the source term. */
typedef struct wost_source_desc {
    int32_t nx, ny;
    const float *rgb;            /* ny * nx * 3, x fastest                                      */
    float index_scale[2], index_offset[2];
    float intensity;             /* source_intensity (core/problem.cu:179)                      */
} wost_source_desc;

/* Replaces Problem<2> as seen by the integrator (core/problem.h:104-171) and the
 * probe EvaluationGrid<2>::ProbeData (core/evaluation_grid.h:16-23). */
typedef struct wost_scene_desc {
    wost_mesh_desc dirichlet;
    wost_mesh_desc neumann;
    float dirichlet_intensity;   /* problem.h:155 */
    float neumann_intensity;     /* problem.h:159 */
    float probe_scale;           /* evaluation_grid.h:18 */
    float probe_pos[2];          /* evaluation_grid.h:19 */
    float probe_up[2];           /* evaluation_grid.h:20 */
    const uint8_t *mask;         /* width*height bytes, 0 = pixel masked out; NULL = all on
                                    (problem.h:163; the reference's fixed 1024^2 default mask,
                                    core/problem.cu:245-247, is sized to the frame here)     */
    wost_source_desc source;     /* zero-initialised = no source term                          */
} wost_scene_desc;

/* Replaces UniformIntegratorSettings (integrator/uniform/integrator.h:27-48); the
 * metric-dump keys are host-side concerns and do not cross the boundary. */
typedef struct wost_settings {
    int32_t width;         /* frameSize[0] */
    int32_t height;        /* frameSize[1] */
    int32_t spp;           /* samplesPerPixel */
    int32_t max_depth;     /* maxWalkingDepth */
    float eps_shell;       /* epsilonShell */
} wost_settings;

typedef struct wost_stats {
    uint64_t walk_steps;       /* sum over depths of the evaluation-queue size   */
    uint64_t walks_started;
    uint64_t walks_absorbed;   /* ended in the epsilon shell                                  */
    uint64_t walks_truncated;  /* reached max_depth                                           */
    uint64_t neumann_hits;     /* steps that landed on the Neumann boundary                   */
    uint64_t inner_visits;     /* LBVH inner nodes expanded by the walk's closest-point queries */
    uint64_t leaf_visits;      /* LBVH leaves (4 segments each) evaluated by those queries    */
    uint64_t trav_trips;       /* wave-level scheduler diagnostics: traversal-phase trips ...  */
    uint64_t step_trips;       /* ... and step-phase trips, summed over waves                 */
    double solve_ms;           /* host wall time of the call, like UniformIntegrator::solve() */
    double kernel_ms;          /* sum of HIP-event durations of the walk kernel launches      */
    uint32_t kernel_launches;  /* number of walk-kernel launches (rounds)                     */
    uint32_t reserved;
} wost_stats;

typedef struct wost_context *wost_handle;

/* Upload the scene, build both LBVHs, allocate walk-state queues for the frame.
 * Replaces Problem<2>::loadConfig geometry upload + UniformIntegrator<2> ctor
 * (integrator/uniform/integrator.cu:626-633 -> initializeImpl :18-62). */
int wost_create(const wost_scene_desc *scene, const wost_settings *settings, int device,
                wost_handle *out);

/* UniformIntegrator<2>::solve() (integrator/uniform/integrator.cu:666-672 -> solveImpl
 * :529-623) for the pixels [pixel_begin, pixel_end) of the frame, row-major pixelId as in
 * the reference.  field_rgb receives (pixel_end - pixel_begin) * 3 floats = solution / spp,
 * i.e. the RGB of the Film after the resolve pass (:614-621).  Results depend only on
 * (pixelId, frame width, geometry, settings), never on the range, so shards concatenate
 * to exactly the full-frame result. */
int wost_solve(wost_handle h, int32_t pixel_begin, int32_t pixel_end, float *field_rgb,
               wost_stats *stats);

/* Same walk, sharded by 64-pixel tiles for multi-GPU load balance: this call owns the tiles
 * t with t % shard_count == shard_index.  field_rgb_dev is a DEVICE buffer of
 * width*height*3 floats that the caller has zero-filled; only owned pixels are written, so
 * a sum-reduce over ranks (RCCL) yields the full field.  `stream` is a hipStream_t (NULL =
 * default stream); the call returns after the stream work has completed. */
int wost_solve_sharded(wost_handle h, int32_t shard_index, int32_t shard_count,
                       float *field_rgb_dev, void *stream, wost_stats *stats);

/* The solve at n evaluation points of the caller (pts_xy: n * 2 floats) instead of the pixels of the frame.  The reference has
 * no counterpart: its EvaluationGrid is the only probe (core/evaluation_grid.h).  Point i is solved with the handle's settings
 * and meshes exactly as a pixel is; its samples share one PCG32 stream seeded as the reference seeds pixel seed_base + i of a
 * frame seed_width wide (integrator/uniform/integrator.cu:71-77), and field_rgb[3 i ..] receives solution / spp.  So
 *   - the frame's own evaluation points in row-major order with seed_base = 0 and seed_width = width reproduce wost_solve
 *     bit for bit, and
 *   - the result of a point does not depend on how a list is cut into calls, as long as seed_base moves with the cut.
 * The frame's mask does not apply (it is a property of the frame); spp = 0 behaves as in the frame.  seed_base >= 0,
 * seed_width > 0 and seed_base + n <= 2^28 (the frame cap of wost_create; the seed is the reference's int product).  A list
 * longer than the frame runs in chunks of width * height points on the handle's queues; wost_stats sums the chunks and
 * wost_last_launches lists their launches in order.  n == 0: WOST_OK and zeroed stats.
 * wost_solve_points: host arrays; a non-finite coordinate is refused (WOST_ERR_INVALID names the first bad index, nothing is
 * launched).  wost_solve_points_dev: DEVICE arrays and the caller's stream as in wost_solve_sharded (NULL = default stream);
 * the call returns after the stream work has completed; a point with a non-finite coordinate is never walked, its field
 * entry is NaN. */
int wost_solve_points(wost_handle h, const float *pts_xy, int32_t n, int32_t seed_base, int32_t seed_width,
                      float *field_rgb, wost_stats *stats);
int wost_solve_points_dev(wost_handle h, const float *pts_xy_dev, int32_t n, int32_t seed_base, int32_t seed_width,
                          float *field_rgb_dev, void *stream, wost_stats *stats);

/* The continued frame solve: a handle can carry ONE frame solve -- for every pixel the PCG32 state after its samples so far,
 * its three raw fp32 sums, its own sample and batch counts and the batch statistics of the error estimate below (52 bytes per
 * pixel, allocated and zeroed on the first call), the samples asked for so far and the shard they belong to.  wost_solve_more runs the samples [done, done + more_spp) of every unmasked pixel on top of that state, stores it
 * back, and field_rgb (width * height * 3 host floats) receives sum / (done + more_spp); done grows by more_spp.  A pixel's
 * samples share one PCG32 stream and are added to fp32 sums in order, so after any sequence of calls the field is that of
 * wost_solve over the full frame with spp = done, bit for bit.  Masked pixels are 0 and carry nothing.  The reference writes
 * such frames while its samples accumulate (integrator/uniform/integrator.cu:578-609).
 *   - more_spp >= 1 and done + more_spp <= 2^20 - 1 (the cap of the "spp" option); anything else is refused with the bound named
 *     and the carried solve untouched.  The handle's own spp setting is neither read nor changed.
 *   - wost_stats and wost_last_launches describe this call alone; over the calls walk_steps, walks_started, walks_absorbed,
 *     walks_truncated and neumann_hits sum to those of the single solve.
 *   - wost_solve, wost_solve_sharded, the point solves and wost_set_option leave the carried solve alone; launch options may
 *     change between two calls (the bits do not depend on them).
 *   - wost_solve_more_sharded follows wost_solve_sharded: a zero-filled DEVICE field, only owned pixels written, the caller's
 *     stream.  The first call of a carried solve binds it to (shard_index, shard_count) -- wost_solve_more binds (0, 1) -- and
 *     a later call with another shard is refused with WOST_ERR_INVALID and a message that names the carried shard.
 *   - wost_solve_restart forgets the carried solve (done = 0, no shard); wost_solve_progress reports done.
 *   - a call that fails after device work has begun drops the carried solve (done = 0) and says so in wost_last_error.
 * Not carried: the guided integrators; a carried solve cannot be saved.  (A caller's points: the carried point list below.) */
int wost_solve_more(wost_handle h, int32_t more_spp, float *field_rgb, wost_stats *stats);
int wost_solve_more_sharded(wost_handle h, int32_t shard_index, int32_t shard_count, int32_t more_spp,
                            float *field_rgb_dev, void *stream, wost_stats *stats);
int wost_solve_restart(wost_handle h);
int wost_solve_progress(wost_handle h, int32_t *spp_done);

/* Continuing a SELECTION of pixels, the per-pixel state, and solves that stop by a per-pixel error estimate.
 * Every pixel of a carried solve has its own sample count n and batch count K: a batch is one continued call that walked the
 * pixel.  A pixel taken up at any count continues its own PCG32 stream and fp32 sums, so its field entry, sum / n, is that of
 * wost_solve at spp = n, bit for bit, whatever the other pixels did.
 *   - wost_solve_more_where: wost_solve_more on the pixels whose byte in select (width * height host bytes) is nonzero; NULL
 *     means every pixel and is wost_solve_more.  Masked pixels stay 0 and carry nothing even when selected; the pixels of
 *     another shard are not this handle's.  field_rgb receives every pixel's sum / n (0 where n is 0); wost_stats counts the
 *     walks of the selected pixels alone.  An empty selection returns WOST_OK with zeroed stats and the field of the carried
 *     state, and launches no walk.  wost_solve_more_where_sharded takes the selection from DEVICE bytes (select_dev) and is
 *     bound to its shard like wost_solve_more_sharded.
 *   - wost_solve_progress keeps its meaning: the sum of more_spp over the calls since the restart -- the count of a pixel that
 *     every call selected -- and the bound 2^20 - 1 applies to it.  The per-pixel counts come from wost_solve_carried.
 *   - the error estimate (batch means): with b_k the sum a pixel gained in its batch k of m_k samples, q = sum_k b_k^2 / m_k,
 *     N = n, S = sum: v = max(q - S * S / N, 0), se = sqrt(v / ((K - 1) * N)) per channel, in fp32 in this order; +inf while
 *     K < 2.  It is the standard error of the pixel's mean S / N when the batches are independent and equally distributed.
 *   - wost_solve_carried copies the state to host arrays of width * height (spp, batches) and width * height * 3 (sum_rgb,
 *     stderr_rgb) entries; any of them may be NULL.  A pixel that is unowned, masked or never walked has 0, 0, 0 sums and +inf.
 *   - wost_solve_adaptive is this loop on the carried solve, as it stands when the call begins: select the pixels that are
 *     owned, unmasked, NOT converged and have n + batch_spp <= max_spp; while any is selected, run batch_spp samples on them
 *     (a wost_solve_more_where on the device selection) and select again.  Converged: K >= min_batches and in every channel
 *     se <= max(abs_tol, rel_tol * |S / N|); a NaN is never converged.  Per round the host reads back one count.  A second
 *     call with tighter tolerances or a larger max_spp resumes.  wost_stats sums the rounds (solve_ms: the whole call) and
 *     wost_last_launches lists all rounds' launches in order.  stderr_rgb and spp_map (host, may be NULL) receive se and n.
 *     Refused before the handle is read: batch_spp < 1, min_batches < 2, max_spp < batch_spp, a tolerance that is negative or
 *     not finite.  Stopping by the estimate biases the result (pixels whose early batches agree by chance stop early), and
 *     batch means under-estimates the error of a pixel with rare bright contributions: see DESIGN 4.3d. */
typedef struct wost_adaptive {
    int32_t batch_spp, min_batches, max_spp;
    float abs_tol, rel_tol;
} wost_adaptive;
int wost_solve_more_where(wost_handle h, int32_t more_spp, const uint8_t *select, float *field_rgb, wost_stats *stats);
int wost_solve_more_where_sharded(wost_handle h, int32_t shard_index, int32_t shard_count, int32_t more_spp,
                                  const uint8_t *select_dev, float *field_rgb_dev, void *stream, wost_stats *stats);
int wost_solve_carried(wost_handle h, int32_t *spp, int32_t *batches, float *sum_rgb, float *stderr_rgb);
int wost_solve_adaptive(wost_handle h, const wost_adaptive *a, float *field_rgb, float *stderr_rgb, int32_t *spp_map,
                        wost_stats *stats);
int wost_solve_adaptive_sharded(wost_handle h, int32_t shard_index, int32_t shard_count, const wost_adaptive *a,
                                float *field_rgb_dev, void *stream, wost_stats *stats);

/* The carried point list: the continued, selective and adaptive solves above on n evaluation points of the caller instead of the
 * pixels of the frame.  wost_points_carry binds a list to the handle: the library copies the points (pts_xy: n * 2 floats) and
 * owns the copy; n == 0 (pts_xy may be NULL) releases the list.  wost_points_carry_dev takes DEVICE points and copies them on the
 * caller's stream (NULL = default stream); it returns when the copy is complete.
 *   Point identity.  Point i is walked with the handle's settings and meshes exactly as a pixel is; its samples share the PCG32
 *     stream of pixel seed_base + i of a frame seed_width wide -- the rule of wost_solve_points.  The frame's mask, tiles and
 *     shards do not apply (they are properties of the frame).  The handle's own spp setting is neither read nor changed.
 *   Bits.  A point continues its own stream and fp32 sums whenever a call takes it up, so after any sequence of calls a point
 *     with n_i samples behind it has the field entry sum / n_i, which is that of wost_solve_points on a handle with spp = n_i, bit
 *     for bit, whatever the other points did; the entry is 0 while n_i = 0.  Over the calls walk_steps, walks_started,
 *     walks_absorbed, walks_truncated and neumann_hits sum to those of the single point solves.  The result of a point does not
 *     depend on how a list is cut into lists, as long as seed_base moves with the cut.
 *   State.  Every point carries the 52 bytes of a pixel of the carried frame solve; its n, K and standard error follow the formulas
 *     above (batch means, fp32, in that order, +inf while K < 2), and the same kernel closes every call.
 *   - wost_points_more: more_spp samples on the listed points whose byte in select (n host bytes) is nonzero; NULL = every point.
 *     field_rgb (n * 3 host floats) receives every point's sum / n_i.  more_spp >= 1, and the sum of more_spp over the calls since
 *     the bind or the restart is at most 2^20 - 1 (wost_points_progress reports it, beside the length of the list); anything else
 *     is refused with the state untouched.  An empty selection returns WOST_OK with zeroed stats and the field of the state, and
 *     launches no walk: wost_last_launches is empty.  wost_points_more_dev: select_dev and field_rgb_dev are DEVICE arrays, the
 *     work runs on the caller's stream and is complete when the call returns.
 *   - wost_points_carried copies the state to host arrays of n (spp, batches) and n * 3 (sum_rgb, stderr_rgb) entries; any of them
 *     may be NULL.
 *   - wost_points_adaptive is the loop of wost_solve_adaptive over the listed points: the same convergence test, the same room
 *     test n_i + batch_spp <= max_spp, one count read back per round, resumption by a second call, and the same refusals before
 *     the handle is read.  stderr_rgb and spp_map (host, may be NULL) receive se and n_i.
 *   - wost_stats describes the call (an adaptive call sums its rounds; solve_ms covers the whole call) and wost_last_launches
 *     lists the launches of the call in order, walk_steps_done cumulative.  A list longer than the frame runs in chunks of
 *     width * height points, cut by index; a chunk in which nothing is selected launches no walk.  The bound of the 16-bit lane
 *     counters on a persistent launch applies to more_spp * max_depth, as in a continued frame call.
 *   One list per handle, beside the carried frame solve: the list has its own state, its own device field and its own copy of the
 *     points.  wost_solve, wost_solve_sharded, wost_solve_points[_dev], the whole wost_solve_more family (wost_solve_restart
 *     included) and wost_set_option leave the list alone, and the wost_points_* calls leave the carried frame solve alone.
 *     wost_points_restart keeps the list and forgets its samples.  Binding a new list replaces the old one, state included; a
 *     bind that is refused leaves the old list as it was.  wost_destroy frees everything.
 *   Arguments of a bind, checked in this order before the handle is read or a device is asked for: a null handle; n < 0; n > 0
 *     with null points; seed_width <= 0; seed_base < 0 or seed_base + n > 2^28.  A more / adaptive / carried call without a bound
 *     list is WOST_ERR_INVALID with a message that says so.  A call that fails after device work has begun drops the samples
 *     (not the list) and says so in wost_last_error.
 *   Non-finite coordinates.  wost_points_carry scans the list and refuses it (WOST_ERR_INVALID names the first bad index).  After
 *     wost_points_carry_dev such a point is never walked and never selected, by a caller's map or by the tolerance: it keeps
 *     n = 0, K = 0, zero sums and +inf standard error, and its field entry is NaN after every call, as wost_solve_points_dev
 *     answers it.
 * Not carried: the guided integrators; a list cannot be saved, and one list is not split into shards -- a multi-GPU caller cuts
 * the list itself and moves seed_base with the cut. */
int wost_points_carry(wost_handle h, const float *pts_xy, int32_t n, int32_t seed_base, int32_t seed_width);
int wost_points_carry_dev(wost_handle h, const float *pts_xy_dev, int32_t n, int32_t seed_base, int32_t seed_width, void *stream);
int wost_points_more(wost_handle h, int32_t more_spp, const uint8_t *select, float *field_rgb, wost_stats *stats);
int wost_points_more_dev(wost_handle h, int32_t more_spp, const uint8_t *select_dev, float *field_rgb_dev, void *stream,
                         wost_stats *stats);
int wost_points_carried(wost_handle h, int32_t *spp, int32_t *batches, float *sum_rgb, float *stderr_rgb);
int wost_points_adaptive(wost_handle h, const wost_adaptive *a, float *field_rgb, float *stderr_rgb, int32_t *spp_map,
                         wost_stats *stats);
int wost_points_adaptive_dev(wost_handle h, const wost_adaptive *a, float *field_rgb_dev, void *stream, wost_stats *stats);
int wost_points_restart(wost_handle h);
int wost_points_progress(wost_handle h, int32_t *n_points, int32_t *spp_done);

/* The gradient at the caller's points: grad u at n points (pts_xy: n * 2 floats) by the walk-on-spheres estimator
 *     grad u(x) = (d / R) E[ n u(x + R n) ]      (u harmonic in the ball B(x, R), n uniform on the unit sphere, d = DIM = 2 or 3)
 * with S = the handle's spp walks per point.  The reference has no counterpart.
 *   - Radius.  dD, dN: the distances wost_closest_point answers for the point on the Dirichlet and the Neumann mesh, the same bits
 *     (+inf for a mesh the scene does not have); R = min(dD, 0.875f * dN), so the first ball never touches the Neumann boundary.
 *     A point is degenerate when R <= eps_shell or R is not finite.
 *   - Directions.  S consecutive draws from the PCG32 stream of pixel seed_base + i in a frame seed_width wide: in 2-D one float
 *     u and n = (cos, sin)(2 pi u), in 3-D u1, u2 and the walk's own uniform direction (z = 1 - 2 u1, r = sqrt(1 - z z),
 *     n = (r cos, r sin, z)(2 pi u2)).
 *   - First points.  y_s = fmaf(R, n_s, x) per component (a degenerate point: y_s = x), and walk (i, s) is wost_solve_points of ONE
 *     sample at y_s on the stream of pixel walk_seed_base + i * S + s in a frame seed_width wide; its result is W_s (RGB).
 *   - Per point, axis k and channel c: mean_c = sum_s W_sc / S, t_s = n_sk (W_sc - mean_c),
 *         grad = d / (R (S - 1)) sum_s t_s          (the sample mean is a control variate; S - 1 keeps the estimate unbiased)
 *         grad_stderr = (d / R) sqrt( sum_s (t_s - mean t)^2 / (S - 1) / S )
 *     and field_rgb = mean.  A degenerate point has NaN grad and grad_stderr and still its mean.  The fp32 sums are taken in an
 *     order of the library's choice.
 *   - A list is walked in blocks of floor(width * height / S) points; a point's outputs do not depend on the cut, and a caller who
 *     cuts a list at point a moves seed_base by a and walk_seed_base by a * S and gets the same bits.  wost_stats sums the blocks
 *     (walks_started is n * S for finite points; kernel_ms includes the two kernels around the walks); wost_last_launches
 *     describes the walks of the LAST block only.
 *   - Not covered by default: a scene with a source term (the in-ball term of the gradient is not built into the default
 *     estimator): WOST_ERR_UNSUPPORTED, unless the handle's option "grad_source" is 1 (below).  Neumann
 *     data needs nothing extra.  The frame's mask does not apply.  The carried frame solve, the carried point list and the options
 *     of the handle are left alone.
 *   Arguments, checked in this order before the handle is read or a device is asked for: null h / pts / out / out->grad; n < 0;
 *     seed_width <= 0; seed_base < 0 or walk_seed_base < 0; seed_base + n > 2^28; the host forms then scan for a non-finite
 *     coordinate (WOST_ERR_INVALID names the first bad point); n == 0: WOST_OK and zeroed stats.  With the handle: S < 2;
 *     S > width * height; walk_seed_base + n * S > 2^28; [seed_base, seed_base + n) overlapping [walk_seed_base, walk_seed_base +
 *     n * S): WOST_ERR_INVALID, the message names the quantity.  A refused call writes no output.
 * wost_solve_gradient_points: host arrays.  wost_solve_gradient_points_dev: DEVICE arrays in pts and out, the caller's stream as
 * in wost_solve_points_dev; the call returns after the stream work has completed; a point with a non-finite coordinate is never
 * walked, all its outputs are NaN.
 *
 * The gradient on a scene with a source term (DESIGN 4.3f "The in-ball term").  For laplace(u) = -f in the ball B(x, R)
 *     grad u(x) = (d / R) E[ n u(x + R n) ] + int_B grad_x G(x, y) f(y) dy,     u(x) = E[ u(x + R n) ] + int_B G(x, y) f(y) dy
 * with grad_x G = (y - x) / (2 pi) (1 / r^2 - 1 / R^2), G = ln(R / r) / (2 pi) in 2-D and grad_x G = (y - x) / (4 pi) (1 / r^3 -
 * 1 / R^3), G = (1 / r - 1 / R) / (4 pi) in 3-D.  The option "grad_source" of the handle (wost_set_option, wost3_set_option;
 * exactly 0, the default, or 1 -- anything else is WOST_ERR_INVALID naming the key) adds the two integrals: with 0 a scene with
 * a source term is refused as above, with 1 it is taken.  On a scene without a source term the option changes nothing: every
 * output keeps its bits, nothing extra is drawn, allocated or launched.  The carried gradient list records the option when it
 * is bound, and every later round uses the recorded value.  Option 1, a scene with a source term, a non-degenerate finite
 * selected point i with radius R, S walks:
 *   1. Walks.  Radius, directions, first points, walks and the walk part of the reduction are exactly those above: the first S
 *     (2-D) or 2 S (3-D) draws of the stream of pixel seed_base + i are unchanged, and so are first_pts.
 *   2. In-ball samples.  S of them, drawn from the SAME stream AFTER the direction draws.  Sample s takes, in this order, a
 *     direction m (2-D: one float through sincos_2pi; 3-D: u1, u2 formed into m exactly as a walk's direction n above), then one
 *     float rho in [0, 1).  Then, every line a single fp32 operation in the written order (no fused multiply-add: numpy float32
 *     reproduces the bits):
 *         r = rho * R;   p_k = r * m_k;   yp_k = x_k + p_k,  ym_k = x_k - p_k
 *         fp = source(yp), fm = source(ym)      (the walk step's bilinear / trilinear grid sample, intensity included)
 *         ds_c = 0.5f * (fp_c - fm_c),   ms_c = 0.5f * (fp_c + fm_c)
 *         wg = 1 - rho * rho  (2-D),  1 - (rho * rho) * rho  (3-D)
 *         wu = rho > 0 ? -(rho * logf(rho)) : 0  (2-D, the deterministic logf of the walk step),  rho - rho * rho  (3-D)
 *     The antithetic pair yp, ym is the analogue of the sample-mean control variate: the constant part of f drops out of the
 *     gradient term exactly.
 *   3. Reduction, in fp64 from those fp32 values as the walk part, rounded once:  a_s,kc = wg_s m_sk ds_sc,
 *         T_kc = (R / S) sum_s a_s,kc          seT_kc = R sqrt( sum_s (a_s - mean a)^2 / (S - 1) / S )
 *         U_c = (R^2 / S) sum_s wu_s ms_sc
 *         grad = (float)(grad_walk + T)     grad_stderr = (float)sqrt(se_walk^2 + seT^2)     field_rgb = (float)(mean + U)
 *     The two parts use disjoint draws, so their variances add; field_rgb stays an estimate of u(x).
 *   4. Excluded points.  A degenerate point takes no in-ball samples and draws none: grad and grad_stderr are NaN and field_rgb
 *     is its mean (its walks start at x and already carry the source).  An unselected point and a point with a non-finite
 *     coordinate behave as above.
 *   5. Cuts and carried lists.  A cut list gives the same bits as before: per-point outputs depend only on the point's own
 *     streams.  In a carried list a batch of round r is still row i of the single call at the round's seeds, bit for bit, in-ball
 *     term included; the state (G, Q, F of rounded batch results) and the adaptive rule are unchanged.
 *   6. Statistics.  walks_started and the other counters do not change; kernel_ms includes the in-ball kernel. */
typedef struct wost_gradient_out {   /* host pointers for the host form, device pointers for the _dev form; only grad is required */
    float *grad;          /* n * DIM * 3: grad[(i*DIM + k)*3 + c] = d u_c / d x_k at point i                      */
    float *grad_stderr;   /* n * DIM * 3 or NULL: the standard error of each entry                                */
    float *field_rgb;     /* n * 3 or NULL: the mean of the point's walks                                         */
    float *radius;        /* n or NULL: the ball radius R_i                                                       */
    float *first_pts;     /* n * S * DIM or NULL: the S first points of point i, walk s at (i*S + s)*DIM          */
} wost_gradient_out;
int wost_solve_gradient_points(wost_handle h, const float *pts_xy, int32_t n, int32_t seed_base, int32_t walk_seed_base,
                               int32_t seed_width, const wost_gradient_out *out, wost_stats *stats);
int wost_solve_gradient_points_dev(wost_handle h, const float *pts_xy_dev, int32_t n, int32_t seed_base, int32_t walk_seed_base,
                                   int32_t seed_width, const wost_gradient_out *out, void *stream, wost_stats *stats);

/* The carried gradient list: the gradient above at n points of the caller, continued in batches of S walks on a
 * selection of the points, with a per-entry error bar and a loop that stops by it.  wost_gradient_points_carry binds a list to the
 * handle: the library copies the points (pts_xy: n * 2 floats) and owns the copy; n == 0 (pts_xy may be NULL) releases the list.
 * wost_gradient_points_carry_dev takes DEVICE points and copies them on the caller's stream (NULL = default stream); both return
 * when the list stands.  S = batch_walks; the handle's own spp setting is neither read nor changed.  The bind computes the radius
 * R_i of every point once, with the bits of wost_solve_gradient_points.
 *   Walkable points.  A point that is degenerate (R <= eps_shell or R not finite) or has a non-finite coordinate (only the _dev
 *     bind lets one in) is NEVER walked by the calls below: it keeps K = 0, NaN grad, grad_stderr and field_rgb, and its radius.
 *     This differs on purpose from the single call, which still walks a degenerate point for its mean: a list exists to spend
 *     walks where they improve an estimate, and such a point has none.
 *   Rounds and seeds.  The list counts rounds r = 0, 1, ...: a round is one wost_gradient_points_more call, or one trip of the
 *     adaptive loop, that selects at least one walkable point.  In round r a selected point i gets one batch, which is row i of
 *     wost_solve_gradient_points(pts, n, seed_base + r * round_stride, walk_seed_base + r * round_stride * S, seed_width) on a
 *     handle with spp = S, bit for bit: its directions come from the stream of pixel seed_base + r * round_stride + i, its walk s
 *     runs on the stream of pixel walk_seed_base + (r * round_stride + i) * S + s.  A point's batch does not depend on which other
 *     points were selected, and a list cut at point a and bound with seed_base + a, walk_seed_base + a * S and the same
 *     round_stride gives the same bits -- which is how a list is cut over ranks.  The points are walked in blocks of
 *     floor(width * height / S); a block without a selected point launches nothing; per round the host reads back the selected
 *     points per block.
 *   State.  Per point K_i, R_i and fp64 sums.  With g_k the batch's grad rounded to fp32 (what the single call returns) and m_k
 *     its fp32 field_rgb: per entry G += (double)g_k and Q += (double)g_k * (double)g_k, per channel F += (double)m_k, in round
 *     order.  Outputs: grad = (float)(G / K), field_rgb = (float)(F / K), grad_stderr = (float)sqrt(max(Q - G G / K, 0) /
 *     ((K - 1) K)) (batch means), +inf while K < 2.  A walkable point with K = 0 answers NaN grad and field_rgb.
 *   - wost_gradient_points_more: one batch on the listed points whose byte in select (n host bytes) is nonzero and that are
 *     walkable; NULL = every walkable point.  out (host arrays; only grad is required) receives the state after the call.  An
 *     empty selection returns WOST_OK with zeroed stats and the state's outputs, launches no walk and consumes no round.  A call
 *     at r == max_rounds is refused with the state untouched.  wost_gradient_points_more_dev: select_dev and the arrays of out are
 *     DEVICE arrays, the work runs on the caller's stream and is complete when the call returns.
 *   - wost_gradient_points_carried: the state into host arrays.
 *   - wost_gradient_points_adaptive: select the walkable points that are not converged and have room (K + 1 <= max_batches);
 *     while any is selected and r < max_rounds, run one batch on them and select again.  Converged: K >= min_batches and for
 *     every entry grad_stderr <= max(abs_tol, rel_tol * |grad|), evaluated in fp32 on the ROUNDED outputs, so a caller can
 *     reproduce the decision from what wost_gradient_points_carried returns; a NaN is never converged.  Running out of rounds
 *     ends the loop with WOST_OK.  A second call with tighter tolerances or a larger max_batches resumes.  Refused before the
 *     handle is read: min_batches < 2, max_batches < 1, a tolerance that is negative or not finite.  Stopping by the estimate
 *     biases the result, as in wost_solve_adaptive.
 *   - wost_gradient_points_restart forgets sums, K and r; the same calls then give the same bits again.
 *     wost_gradient_points_progress reports the length of the list and the rounds done.
 *   - wost_stats sums the blocks and rounds of the call (walks_started is S x the batches walked; kernel_ms includes the kernels
 *     around the walks); wost_last_launches describes the walks of the last block walked.
 *   One gradient list per handle, beside the carried frame solve and the carried point list.  It shares the scratch of
 *     wost_solve_gradient_points, and a single gradient call between two rounds changes nothing in the list.  The frame solves,
 *     the point solves, the carried frame solve, the carried point list and wost_set_option leave the gradient list alone, and
 *     the gradient list leaves all of them alone.  A refused bind leaves the old list as it was; wost_destroy frees it.
 *   Arguments of a bind, checked in this order before the handle is read or a device is asked for: a null handle; n < 0; n > 0
 *     with null points; seed_width <= 0; a negative seed; batch_walks < 2; round_stride < n; max_rounds < 1; seed_base +
 *     (max_rounds - 1) * round_stride + n > 2^28; walk_seed_base + ((max_rounds - 1) * round_stride + n) * S > 2^28 (in 64 bits);
 *     the two seed ranges overlapping; in the host form, the first non-finite point.  With the handle: S > width * height
 *     (WOST_ERR_INVALID); a scene with a source term (WOST_ERR_UNSUPPORTED, as the single call answers).  A more / adaptive /
 *     carried / restart call with no list bound is WOST_ERR_INVALID with a message that says so; a call that fails after device
 *     work has begun drops the samples (not the list) and says so in wost_last_error.
 * Not carried: the guided integrators; a list cannot be saved, and one list is not split into shards. */
typedef struct wost_gradient_carried_out {   /* host pointers for the host forms, device pointers for the _dev forms; only grad is required */
    float *grad;          /* n * DIM * 3, the layout of wost_gradient_out                                          */
    float *grad_stderr;   /* n * DIM * 3 or NULL                                                                  */
    float *field_rgb;     /* n * 3 or NULL: the mean of the point's batch means                                   */
    float *radius;        /* n or NULL: the ball radius R_i                                                       */
    int32_t *batches;     /* n or NULL: K_i                                                                       */
} wost_gradient_carried_out;
typedef struct wost_gradient_adaptive {
    int32_t min_batches, max_batches;
    float abs_tol, rel_tol;
} wost_gradient_adaptive;
int wost_gradient_points_carry(wost_handle h, const float *pts_xy, int32_t n, int32_t batch_walks, int32_t round_stride, int32_t max_rounds,
                               int32_t seed_base, int32_t walk_seed_base, int32_t seed_width);
int wost_gradient_points_carry_dev(wost_handle h, const float *pts_xy_dev, int32_t n, int32_t batch_walks, int32_t round_stride,
                                   int32_t max_rounds, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width, void *stream);
int wost_gradient_points_more(wost_handle h, const uint8_t *select, const wost_gradient_carried_out *out, wost_stats *stats);
int wost_gradient_points_more_dev(wost_handle h, const uint8_t *select_dev, const wost_gradient_carried_out *out_dev, void *stream,
                                  wost_stats *stats);
int wost_gradient_points_carried(wost_handle h, const wost_gradient_carried_out *out);
int wost_gradient_points_adaptive(wost_handle h, const wost_gradient_adaptive *a, const wost_gradient_carried_out *out, wost_stats *stats);
int wost_gradient_points_adaptive_dev(wost_handle h, const wost_gradient_adaptive *a, const wost_gradient_carried_out *out_dev, void *stream,
                                      wost_stats *stats);
int wost_gradient_points_restart(wost_handle h);
int wost_gradient_points_progress(wost_handle h, int32_t *n_points, int32_t *rounds_done);

/* Exit lists: walk once, then the solution for any Dirichlet data and its derivative by that data.  A walk reads
 * no Dirichlet colour before the step that absorbs it, and that step adds  colour * dirichlet_intensity * thp  to the walk's
 * sum: everything else -- the path, the throughput thp, what the source and the Neumann samples added -- depends on the geometry,
 * the Neumann data, the source and the two intensities, which stay the handle's.  wost_exits_walk walks S = walks walks at each
 * of n points of the caller (pts_xy: n * 2 floats) and keeps one record per walk; the list belongs to the handle.  The reference
 * has no counterpart.
 *   Walks.  Walk (i, s) is wost_solve_points of ONE sample at point i on the stream of pixel walk_seed_base + i * S + s in a
 *     frame seed_width wide, with the handle's max_depth, eps_shell, meshes, source and intensities -- the walk convention of
 *     wost_solve_gradient_points.  The handle's spp setting is neither read nor changed.  The list is walked in launches of
 *     width * height walks, so S is not bound by the frame; a list cut at point a and walked with walk_seed_base + a * S gives
 *     the same records.  wost_stats: the five counters as that point solve counts them (walks_started is n * S for finite
 *     points), kernel_ms the launches' device time, kernel_launches their number; the other counters are zero.
 *     wost_last_launches is left as it was.
 *   Records, per walk, entry i * S + s:
 *       prim      the absorbing segment by its index in the caller's segs array; -1 for a walk that was not absorbed -- truncated
 *                 at max_depth, escaped (no boundary within reach), or a scene without a Dirichlet mesh
 *       uv        the fp32 projection ratio of the absorbing step, the same bits; side: its side (-1, 0, +1), the same bits
 *       thp       the throughput at absorption
 *       base_rgb  the walk's three sums just before the Dirichlet term is added; for a walk that was not absorbed, its final sums
 *     A walk that was not absorbed has uv = 0, side = 0 and its final thp.  A point with a non-finite coordinate (only the _dev
 *     form lets one in) is never walked: prim = -1, uv, thp and base_rgb NaN.
 *   Apply.  K >= 1 sets of per-vertex colours in the layout of wost_mesh_desc.colors (colors: K * n_verts * 6 floats, n_verts the
 *     Dirichlet mesh's).  Per walk, set k and channel c, with v0, v1 the vertices of segment prim and off = 0 for side >= 0, else
 *     3, every line a single fp32 operation (no fused multiply-add: numpy float32 reproduces the bits):
 *         col = colors[k][v0][off + c] * (1 - uv) + colors[k][v1][off + c] * uv
 *         col = col * dirichlet_intensity;   col = col * thp;   W = col + base_c
 *     and W = base_c for a walk that was not absorbed: with the handle's own colours W is the result of that walk's point solve,
 *     bit for bit.  Per point, in fp64 from the fp32 W, rounded once:
 *         field_rgb[k][i][c] = (float)(sum_s W / S)
 *         stderr_rgb[k][i][c] = (float)sqrt( sum_s (W - mean)^2 / (S - 1) / S ),   +inf when S = 1        (stderr_rgb may be NULL)
 *     The fp64 sums are taken in an order of the library's choice.
 *   Adjoint.  field is linear in colors; given dfield (K * n * 3) the transposed map into dcolors (K * n_verts * 6):
 *         dcolors[k][v][off + c] = sum over the absorbed walks (i, s) with v a vertex of their segment, on that side, of
 *                                  (dfield[k][i][c] / S) * dirichlet_intensity * thp * w_v
 *     w_v = 1 - uv for v0 and uv for v1, formed in fp32 as apply forms them; every factor is promoted to fp64, the products are
 *     taken from left to right and summed in fp64, and the sum is rounded to fp32 once.  A vertex no walk exits at gets exactly
 *     0.  The summation order is the library's (atomic adds) and may differ from run to run: an entry of M terms is within
 *     M * 2^-52 * sum |terms| + 2^-24 |value| of the exact sum of those terms.  A scene without a Dirichlet mesh has no colours
 *     to differentiate by: WOST_ERR_UNSUPPORTED.
 *   - wost_exits_walk: host points; a non-finite coordinate is refused.  wost_exits_walk_dev: DEVICE points and the caller's
 *     stream (NULL = default stream); both return when the list stands.  n == 0 (pts may be NULL) releases the list.  A new walk
 *     replaces the list only once it stands whole; a call that is refused or fails leaves the old list as it was and writes
 *     nothing; an allocation that fails is WOST_ERR_NOMEM.  wost_destroy frees the list.
 *   - wost_exits_records: the records into host arrays of n * S entries (uv: n * S * (DIM - 1), base_rgb: n * S * 3); any
 *     pointer of wost_exit_records may be NULL.
 *   - wost_exits_apply, wost_exits_adjoint: host arrays.  wost_exits_apply_dev, wost_exits_adjoint_dev: DEVICE arrays, the work
 *     runs on the caller's stream and is complete when the call returns.
 *   - wost_exits_progress: the points of the list and S (0, 0: none is bound).
 *   One exit list per handle, beside the carried frame solve, the carried point list and the gradient list: the frame solves, the
 *     point solves, the carried solves, the gradient calls and wost_set_option leave the list alone, and the list leaves all of
 *     them alone.  No mesh table of the handle is written: the colours are arguments.
 *   Arguments of a walk, checked in this order before the handle is read or a device is asked for: a null handle; n < 0, or n > 0
 *     with null points; walks < 1; seed_width <= 0; walk_seed_base < 0; walk_seed_base + n * walks > 2^28 (in 64 bits); in the
 *     host form, the first non-finite point (the message names its index).  Of apply and adjoint: a null handle, a null array,
 *     K < 1, no list bound -- each WOST_ERR_INVALID with a message that says so.
 * Not built: adding walks to a list, shards of one list, saving a list, the guided integrators, the C++ host mirror, and Neumann
 * or source data as variables. */
typedef struct wost_exit_records {   /* host arrays; any may be NULL */
    int32_t *prim;        /* n * S                                                                                 */
    float *uv;            /* n * S * (DIM - 1): in 3-D u and v of walk w at 2 w, 2 w + 1                           */
    int32_t *side;        /* n * S                                                                                 */
    float *thp;           /* n * S                                                                                 */
    float *base_rgb;      /* n * S * 3                                                                             */
} wost_exit_records;
int wost_exits_walk(wost_handle h, const float *pts_xy, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width,
                    wost_stats *stats);
int wost_exits_walk_dev(wost_handle h, const float *pts_xy_dev, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width,
                        void *stream, wost_stats *stats);
int wost_exits_records(wost_handle h, const wost_exit_records *out);
int wost_exits_apply(wost_handle h, const float *colors, int32_t K, float *field_rgb, float *stderr_rgb);
int wost_exits_apply_dev(wost_handle h, const float *colors_dev, int32_t K, float *field_rgb_dev, float *stderr_rgb_dev, void *stream);
int wost_exits_adjoint(wost_handle h, const float *dfield, int32_t K, float *dcolors);
int wost_exits_adjoint_dev(wost_handle h, const float *dfield_dev, int32_t K, float *dcolors_dev, void *stream);
int wost_exits_progress(wost_handle h, int32_t *n_points, int32_t *walks);

/* Exit lists of the gradient: the exit list of the FIRST POINTS of wost_solve_gradient_points, kept with the
 * directions and the radii, so that grad u, its standard error and the mean at the caller's points follow for any Dirichlet data
 * without another walk, and so does the derivative of that gradient by the data.  The estimator is linear in the walks' results,
 *     grad_kc = d / (R (S - 1)) sum_s n_sk (W_sc - mean_c)  =  d / (R (S - 1)) sum_s (n_sk - nbar_k) W_sc,
 * and every W_s is base + colour * dirichlet_intensity * thp of that walk's exit record.  The reference has no counterpart.
 *   1. The list.  wost_exits_walk_gradient binds THE exit list of the handle (there is one): n points, S = walks walks each.  It
 *     replaces a plain list, and a plain wost_exits_walk replaces it.  Radius, directions and first points are those of
 *     wost_solve_gradient_points(pts, n, seed_base, walk_seed_base, seed_width) on a handle with spp = S, items 1-3 of its
 *     contract, bit for bit (the same kernel in front).  Walk (i, s) is an exit-list walk that starts at the first point y_is on
 *     the stream of pixel walk_seed_base + i * S + s: its record is what wost_exits_walk records for a point at y_is with walks = 1
 *     on that pixel.  The handle's spp setting is neither read nor changed, and S is not bound by the frame.  A degenerate point
 *     (R <= eps_shell or R not finite) has y = x, as in the single call.  A point with a non-finite coordinate (only the _dev
 *     form lets one in) is never walked: its radius, directions and first points are NaN (wost_exits_gradient_records), its
 *     records those of such a point in a plain list.  wost_exits_records, wost_exits_apply, wost_exits_adjoint and
 *     wost_exits_progress work on such a list as on any other: the field they see is the mean of the walks from the first points.
 *     A list cut at point a and walked with seed_base + a and walk_seed_base + a * S gives the same rows.
 *   2. Apply.  K >= 1 sets of colours as wost_exits_apply takes them.  Per walk W is formed exactly as there (the same fp32
 *     operations).  Per point and set field_rgb, grad and grad_stderr follow item 4 of the gradient's contract: the sums run in
 *     fp64 from the fp32 W and directions, each result is rounded to fp32 once, the variance is the two-pass one.  A degenerate
 *     point gets NaN grad and grad_stderr and still its mean.  WITH THE HANDLE'S OWN COLOURS THE THREE OUTPUTS ARE THOSE OF
 *     wost_solve_gradient_points AT spp = S, BIT FOR BIT, and with any other colours those of a handle created with them.
 *     Layouts: grad, grad_stderr: K * n * DIM * 3, entry [k][i][axis][c] as in wost_gradient_out; field_rgb: K * n * 3.
 *   3. Adjoint.  grad is affine in colors; given dgrad (K * n * DIM * 3) the transposed map of its linear part into dcolors
 *     (K * n_verts * 6):
 *         dcolors[k][v][off + c] = sum over the absorbed walks (i, s) of non-degenerate points with v a vertex of their
 *                                  primitive, on that side, of   q * dirichlet_intensity * thp * w_v
 *         q = sum_axis dgrad[k][i][axis][c] * (DIM / (R_i (S - 1))) * (n_s,axis - nbar_i,axis),     nbar_i = sum_s n_s / S
 *     w_v is formed in fp32 as apply forms it; every factor is promoted to fp64, summed in fp64 and the sum is rounded to fp32
 *     once.  A vertex no walk exits at gets exactly 0; degenerate and non-finite points add nothing, and their dgrad is not read.
 *     The summation order is the library's (atomic adds, and the order of the nbar sum) and may differ from run to run: an entry
 *     of M terms is within (M + S + 12) * 2^-52 * sum 2 |a| + 2^-24 |value| of the exact sum, a the term without its direction
 *     factor.  A scene without a Dirichlet mesh: WOST_ERR_UNSUPPORTED.  The derivative of field_rgb is wost_exits_adjoint on the
 *     same list.
 *   4. The in-ball term on a scene with a source term ("The gradient on a scene with a source term" above).  The
 *     handle's option "exits_grad_source" (wost_set_option, wost3_set_option; exactly 0, the default, or 1) is the door: with 0
 *     a walk on such a scene is refused, with 1 it runs and THE LIST CARRIES THE TERM.  T, seT and U of that section do not depend
 *     on the Dirichlet data, so the walk computes them once: after the kernels in front, in blocks of max(1, floor(width *
 *     height / S)) points, the S in-ball samples per point of wost_solve_gradient_points (the same kernel, the same streams,
 *     behind the direction draws) and a reduction that keeps per point, in fp64 and unrounded,
 *         T_kc = (R / S) sum_s a_s,   seT_kc = R sqrt(sum_s (a_s - mean a)^2 / (S - 1) / S),   U_c = (R^2 / S) sum_s wu_s ms_sc
 *     as that call forms them; a degenerate or non-finite point takes no samples and keeps +0.0 in all 6 DIM + 3.  Apply joins
 *     them to every one of the K sets before the one rounding, in that call's order:  grad = walk part + T,  grad_stderr =
 *     sqrt(walk part^2 + seT^2),  field_rgb = mean + U  (a degenerate point: NaN, NaN and its mean without U).  WITH THE HANDLE'S
 *     OWN COLOURS THE THREE OUTPUTS ARE THOSE OF wost_solve_gradient_points AT spp = S WITH "grad_source" 1, BIT FOR BIT, and
 *     with other colours those of a handle created with them -- S is still not bound by the frame.  The term is constant in the
 *     colours: wost_exits_adjoint_gradient, wost_exits_index and the ordered adjoints are what they are without it, and
 *     wost_exits_apply on such a list is the mean of the walks from the first points, without U.  The mode is the list's,
 *     recorded at the walk: a later change of the option does not reach a bound list.  On a scene without a source term the
 *     option changes nothing -- the same records, outputs and kernel_launches, no allocation and no launch more.  The term costs
 *     8 * (6 * DIM + 3) bytes per point in the list; the samples of a block pass through a temporary of the call's own,
 *     (DIM + 8) * max(width * height, S) floats, freed before it returns, so wost_solve_gradient_points and the carried gradient
 *     list between walk and apply change nothing, nor does the walk change anything for them.  wost_stats of such a walk: the
 *     five counters as without the term (the in-ball samples are no walks); kernel_ms includes the new launches;
 *     kernel_launches = ceil(n / (width * height)) + 2 * ceil(n / B) + ceil(n * S / (width * height)), B the block above.
 *   - wost_exits_gradient_terms: the term of the bound list into host arrays, T and seT n * DIM * 3 doubles, entry [i][axis][c],
 *     U n * 3; any pointer may be NULL.  Refused, in this order: a null handle; no list bound; a plain list (the message names
 *     wost_exits_walk_gradient); a list without the term (WOST_ERR_INVALID; the message names exits_grad_source).  With all
 *     three pointers NULL it answers whether the bound list carries the term.
 *   - wost_exits_walk_gradient: host points; a non-finite coordinate is refused.  wost_exits_walk_gradient_dev: DEVICE points and
 *     the caller's stream (NULL = default stream); both return when the list stands.  n == 0 (pts may be NULL) releases the list.
 *     A call that is refused or fails leaves the old list as it was; an allocation that fails is WOST_ERR_NOMEM.  The list costs
 *     4 * (6 + 3 * DIM) bytes per walk and 4 per point.
 *   - wost_exits_gradient_records: radius, directions and first points into host arrays; any pointer may be NULL.
 *   - wost_exits_apply_gradient, wost_exits_adjoint_gradient: host arrays; grad_stderr and field_rgb may be NULL.  The _dev
 *     forms: DEVICE arrays, the work runs on the caller's stream and is complete when the call returns.
 *   - wost_stats of the walk: the five counters as the plain exit walk counts them; kernel_ms includes the kernels in front;
 *     kernel_launches = ceil(n / (width * height)) + ceil(n * S / (width * height)): the kernels in front run in launches of at
 *     most width * height points, then the walks as in wost_exits_walk.  wost_last_launches is left as it was.
 *   The carried frame solve, the carried point list, the gradient list, wost_solve_gradient_points (which keeps its own scratch)
 *     and wost_set_option neither touch the list nor are touched by it.
 *   Arguments of a walk, checked in this order before the handle is read or a device is asked for: a null handle; n < 0, or n > 0
 *     with null points; walks < 2; seed_width <= 0; a negative seed; seed_base + n > 2^28; walk_seed_base + n * walks > 2^28 (in
 *     64 bits); [seed_base, seed_base + n) overlapping [walk_seed_base, walk_seed_base + n * walks); in the host form, the first
 *     non-finite point.  With the handle: a scene with a source term is WOST_ERR_UNSUPPORTED whatever the option "grad_source"
 *     says, unless the option "exits_grad_source" is 1 (item 4; the message names it).  Of apply and adjoint: a null
 *     handle, a null required array, K < 1, no list bound, a bound list without directions (WOST_ERR_INVALID; the message names
 *     wost_exits_walk_gradient) -- which wost_exits_gradient_records answers on a plain list too.
 * Not built: adding walks to a list, shards of one list, saving a list, the
 * carried gradient list on top of exit lists, the guided integrators, the C++ host mirror, and Neumann or source data as
 * variables. */
typedef struct wost_exit_gradient_records {   /* host arrays; any may be NULL */
    float *radius;        /* n                                                                                     */
    float *dirs;          /* n * S * DIM: the direction of walk w at w * DIM                                       */
    float *first_pts;     /* n * S * DIM: where walk w started                                                     */
} wost_exit_gradient_records;
int wost_exits_walk_gradient(wost_handle h, const float *pts_xy, int32_t n, int32_t walks, int32_t seed_base, int32_t walk_seed_base,
                             int32_t seed_width, wost_stats *stats);
int wost_exits_walk_gradient_dev(wost_handle h, const float *pts_xy_dev, int32_t n, int32_t walks, int32_t seed_base, int32_t walk_seed_base,
                                 int32_t seed_width, void *stream, wost_stats *stats);
int wost_exits_gradient_records(wost_handle h, const wost_exit_gradient_records *out);
int wost_exits_apply_gradient(wost_handle h, const float *colors, int32_t K, float *grad, float *grad_stderr, float *field_rgb);
int wost_exits_apply_gradient_dev(wost_handle h, const float *colors_dev, int32_t K, float *grad_dev, float *grad_stderr_dev,
                                  float *field_rgb_dev, void *stream);
int wost_exits_gradient_terms(wost_handle h, double *T, double *seT, double *U);
int wost_exits_adjoint_gradient(wost_handle h, const float *dgrad, int32_t K, float *dcolors);
int wost_exits_adjoint_gradient_dev(wost_handle h, const float *dgrad_dev, int32_t K, float *dcolors_dev, void *stream);

/* Exit lists: the index and the ordered adjoint.  wost_exits_adjoint and wost_exits_adjoint_gradient scatter with
 * atomic adds, so their last bits change from run to run.  wost_exits_index transposes the bound list once -- per vertex and
 * side, the walks that exit there -- and the ordered adjoints gather over it in a stated order:
 * dcolors IS A FUNCTION OF THE LIST AND THE ARGUMENT ALONE: THE SAME BITS ON EVERY RUN, EVERY STREAM AND EVERY DEVICE OF THIS
 * KIND.  The reference has no counterpart.
 *   1. The index.  An incidence is  inc = w * DIM + j:  walk w = i * S + s of the list, absorbed (prim >= 0), and corner j of its
 *     primitive.  Its bin is  b = 2 * v + (side < 0 ? 1 : 0)  with v = segs[prim][j] (tris[prim][j]) of the caller: there are
 *     2 * n_verts bins, and a bin holds its incidences ascending in inc.  The index is bin_begin (2 * n_verts + 1 offsets, int64)
 *     and inc (int32, n_incidences = DIM * absorbed walks of them); bin b is inc[bin_begin[b] .. bin_begin[b + 1]).  For a list
 *     of the gradient it also holds, per point and axis, the fp64 mean direction nbar that the sums below use: a lane l of 64
 *     adds the directions of the point's walks s = l, l + 64, ... in that order to a sum that starts at +0.0, the 64 sums are
 *     combined by the butterfly below, and the result is divided by (double)S.  The index is built on the device on the
 *     default stream, without floating-point atomics: it is a function of the records.  It costs 16 * n_verts + 4 *
 *     n_incidences bytes (+ 8 * DIM * n for a list of the gradient); the build's temporaries (about 4 * n * S + 16 *
 *     n_incidences bytes) are freed before it returns.
 *   2. The order.  Entry dcolors[k][v][off + c] (off = 0 for side >= 0, else 3) is the sum over bin b = 2 v + (off ? 1 : 0).
 *     Lane l of 64 takes the bin's incidences at positions l, l + 64, ... of the bin, in that order, and adds the term of each
 *     to an fp64 sum that starts at +0.0.  The term of incidence w * DIM + j, w = i * S + s, with w_v the fp32 weight of corner
 *     j as apply forms it, every factor promoted to fp64 and the products taken from left to right:
 *         wost_exits_adjoint_ordered            dfield[k][i][c] / S * dirichlet_intensity * thp * w_v
 *         wost_exits_adjoint_gradient_ordered   q * dirichlet_intensity * thp * w_v,
 *                                               q = dgrad[k][i][0][c] * scale * cen_0 + dgrad[k][i][1][c] * scale * cen_1 (+ ...),
 *                                               scale = DIM / (R_i * (S - 1)),   cen_a = n_s,a - nbar_i,a,   the axes in that order
 *     An incidence of a degenerate or non-finite point (R <= eps_shell or R not finite) is SKIPPED in the gradient form: it is
 *     not added as zero, and its dgrad is not read.  The 64 sums x_0 .. x_63 are then combined by the butterfly
 *         for off in 32, 16, 8, 4, 2, 1:   x_l = x_l + x_(l xor off)   on all lanes at once
 *     and x_0 is rounded to fp32 once.  An empty bin gives +0.0f.  No contraction anywhere: numpy float64 reproduces the bits
 *     (tests/exits_index_emulation.py does).  The values agree with the unordered calls within those calls' bounds.
 *   - wost_exits_index: builds the index of the bound list; a second call is a no-op that returns WOST_OK.  The index lives and
 *     dies with the list: a walk call that replaces the list or releases it (n == 0) drops the index, a walk that is refused or
 *     fails leaves both as they were, wost_destroy frees it.  An allocation that fails is WOST_ERR_NOMEM, and the list and any
 *     old index stay.  A scene without a Dirichlet mesh: WOST_ERR_UNSUPPORTED.
 *   - wost_exits_index_info: n_incidences and the entries of the longest bin; 0, 0 with WOST_OK when no index stands.
 *   - wost_exits_index_records: the index into host arrays of 2 * n_verts + 1 and n_incidences entries; either may be NULL.
 *   - wost_exits_adjoint_ordered, wost_exits_adjoint_gradient_ordered: the arguments and layouts of wost_exits_adjoint and
 *     wost_exits_adjoint_gradient, host arrays.  The _dev forms: DEVICE arrays, the work runs on the caller's stream and is
 *     complete when the call returns.  One wave per (bin, set): plain loads and stores, no scratch array, no atomic.
 *   The index and the ordered calls leave the list, the unordered calls and every neighbour of the list alone.
 *   Refusals, in this order: a null handle; a null required array; K < 1; no list bound; no index built (WOST_ERR_INVALID, the
 *     message names wost_exits_index); for the gradient form, a list without directions (the message names
 *     wost_exits_walk_gradient); a scene without a Dirichlet mesh (WOST_ERR_UNSUPPORTED).
 * Not built: a bin split across waves (it would change the order above), an ordered apply (apply is deterministic already),
 * and what the exit lists themselves leave out. */
int wost_exits_index(wost_handle h);
int wost_exits_index_info(wost_handle h, int64_t *n_incidences, int64_t *longest_bin);
int wost_exits_index_records(wost_handle h, int64_t *bin_begin, int32_t *inc);
int wost_exits_adjoint_ordered(wost_handle h, const float *dfield, int32_t K, float *dcolors);
int wost_exits_adjoint_ordered_dev(wost_handle h, const float *dfield_dev, int32_t K, float *dcolors_dev, void *stream);
int wost_exits_adjoint_gradient_ordered(wost_handle h, const float *dgrad, int32_t K, float *dcolors);
int wost_exits_adjoint_gradient_ordered_dev(wost_handle h, const float *dgrad_dev, int32_t K, float *dcolors_dev, void *stream);

/* renderDirichletSDF / renderSilhouetteSDF (integrator/common.h:52-123): one query per
 * pixel of the frame, out receives width*height distances. */
int wost_render_sdf(wost_handle h, int which_mesh, float *out_dist);

/* renderSource (integrator/common.h:126-163): intensity * f at every pixel of the frame, out
 * receives width*height*3 floats (zeros without a source term). */
int wost_render_source(wost_handle h, float *out_rgb);

/* lbvh::query_device(bvh, lbvh::nearest(q), distance_calculator()) + checkPointSide +
 * computeProjectionRatio for a batch of host points (call sites
 * integrator/uniform/integrator.cu:138,148-149).  out_idx = original segment index. */
int wost_closest_point(wost_handle h, int which_mesh, const float *pts, int32_t n,
                       int32_t *out_idx, float *out_dist, float *out_uv, int32_t *out_side);

/* lbvh::query_device(bvh, nearest_silhouette(q,false), silhouette_distance_calculator())
 * (integrator.cu:189); rmax (optional, per point) bounds the search radius. */
int wost_closest_silhouette(wost_handle h, int which_mesh, const float *pts, const float *rmax,
                            int32_t n, float *out_dist);

/* lbvh::query_device(bvh, ray_intersect(ray(o,d), tmax), intersect_test()) closest hit
 * (integrator.cu:500-503). */
int wost_ray_intersect(wost_handle h, int which_mesh, const float *origins, const float *dirs,
                       const float *tmax, int32_t n, int32_t *out_hit, float *out_t,
                       int32_t *out_idx);

/* ---- guided path, deterministic distribution layer (first slice of SURVEY 8a row a24) -------
 * Batch entry points over HOST arrays; no handle, `device` selects the GPU. */

/* logModifiedBesselFn(x, 0|1), VonMises::log_eval(cos), VonMises::d_log_eval_d_kappa(cos)
 * (reference util/vonmises.h:75-93,128-163) for n (kappa, cos_theta) pairs; any output may
 * be NULL. */
int wost_vonmises_eval(int device, const float *kappa, const float *cos_theta, int32_t n,
                       float *log_i0, float *log_i1, float *log_pdf, float *dlogpdf_dkappa);

/* rejectionSample(kappa, proposalR, sampler) (util/vonmises.h:95-118): per point a PCG32
 * stream setSeed(seed[i], 1) and per_point consecutive angles in theta[n*per_point]. */
int wost_vonmises_sample(int device, const float *kappa, const uint64_t *seed, int32_t n,
                         int32_t per_point, float *theta);

/* VMM<2,8> built from 32 raw network outputs per point (integrator/guided/distribution.h:
 * 146-168, train.h:50-79): mixture pdf at direction wi[n*2] (pdf may be NULL) and one sampled
 * direction per point with the stream setSeed(seed[i], 1) (distribution.h:186-198;
 * sample_dir may be NULL). */
int wost_vmm_pdf_sample(int device, const float *raw, const float *wi, const uint64_t *seed,
                        int32_t n, float *pdf, float *sample_dir);

/* Training-side gradients: VMM<2,8>::gradients_probability
 * (distribution.h:201-264) chained with compute_dL_doutput_divergence (train.h:492-553) for n
 * samples: raw[n*33] network outputs (8 lobes + selection logit), reference record per sample
 * (dir[n*2], li = mean |solution/thp|, dir_pdf, on_neumann flags (may be NULL), normal[n*2]),
 * loss_scale (the reference uses 128, divided by n inside).  Outputs dL/draw[n*33] and the
 * per-sample likelihood term (may be NULL). */
int wost_vmm_loss_gradients(int device, const float *raw, const float *dir, const float *li,
                            const float *dir_pdf, const uint8_t *on_neumann, const float *normal,
                            int32_t n, float loss_scale, float *dl_draw, float *likelihood);

/* ---- guiding network (SURVEY 8a rows a22/a23 + the optimizer of a27) -------------------------
 * Replaces the tiny-cuda-nn objects of the guided integrator: the NetworkWithInputEncoding
 * variant of util/network.h:21-196 (inference 39-47, forward 49-60, backward 62-92, parameter
 * order 94-136), built in integrator/guided/integrator.cu:1095-1131 from the configuration of
 * data/ladybug/n.json:49-81: DenseGrid encoding (n_levels x n_features_per_level, linear
 * interpolation) -> bias-free ReLU MLP -> n_output raw values per point; Adam nested in a
 * debiased EMA.  Parameter vector order as in util/network.h:99-117 (network first, encoding
 * second): [W1 n_neurons x enc][W2..][Wout pad16(n_output) x n_neurons][grid levels].
 * fp32 arithmetic by default (the bit-exact mode); wost_net_set_option("precision" / "train_precision", 16) selects the
 * reference's half precision for the inference and for the training passes (f16 MFMAs, fp32 master weights). */
typedef struct wost_net_config {
    int32_t n_levels, n_features_per_level, base_resolution;
    float per_level_scale;
    int32_t n_neurons, n_hidden_layers, n_output;
    float learning_rate, beta1, beta2, epsilon, l2_reg, ema_decay;
} wost_net_config;
typedef struct wost_net *wost_net_handle;

/* integrator/guided/integrator.cu:1095-1131 (network + optimizer + trainer construction):
 * allocates parameters on `device` and initialises them from `seed` (util/network.h:113-136;
 * MLP xavier-uniform, grid uniform(-1e-4, 1e-4)).  Shapes: 1-16 levels x 1-8 features with an encoded width <= 64 that is a multiple
 * of 8, 8-64 neurons (a multiple of 8), 1-15 hidden layers, 1-64 outputs, base_resolution >= 1, a finite per_level_scale >= 1, at most
 * 1e9 grid floats; anything else is WOST_ERR_UNSUPPORTED, decided before a device is looked for. */
int wost_net_create(int device, const wost_net_config *cfg, uint64_t seed, wost_net_handle *out);
int wost_net_destroy(wost_net_handle h);
int wost_net_n_params(wost_net_handle h, uint64_t *n_total, uint64_t *n_mlp);
/* which: 0 = training parameters, 1 = inference (EMA) parameters, 2 = gradients of the last
 * wost_net_train_step (scaled by loss_scale). */
int wost_net_get_params(wost_net_handle h, int which, float *host);
/* Gradients are accumulated as 64-bit fixed point (value * 2^36) with integer atomics, so they do
 * not depend on the order of summation.  A multi-GPU caller may supply the accumulation buffer
 * itself (device memory, n_total int64; NULL = internal again), e.g. memory it can hand to a
 * collective. */
int wost_net_set_gradient_buffer(wost_net_handle h, void *dev_int64);
/* sets training and inference parameters, resets the optimizer state */
int wost_net_set_params(wost_net_handle h, const float *host);
/* network->inference (integrator/guided/integrator.cu:560,597; util/network.h:39-47): xy[n*2] in [0,1]^2 -> out[n*n_output];
 * use_inference_params = 1 evaluates the EMA weights (what rendering uses), 0 the training ones.
 * A point outside [0,1]^2 (a walker outside the guiding box) is evaluated too: its cell index floor(scale * x + 0.5) is negative or past
 * the level, and the entry it reads is (cx + cy * res) mod 2^32, then mod the level's padded entry count -- tiny-cuda-nn's 32-bit dense
 * grid_index.  The value is well defined and equal to the CPU restatement's, not an extrapolation of the field (three inputs: the same
 * sum in 64 bits). */
int wost_net_inference(wost_net_handle h, const float *xy, int32_t n, float *out, int use_inference_params);
/* "precision": 32 (default) = fp32 everywhere, bit-exact against the CPU restatement; 16 = the reference's own
 * network precision for inference (tiny-cuda-nn FullyFusedMLP + grid in half, util/network.h:21-196,
 * data/ladybug/n.json:61-67): f16 weights / activations / grid values, fp32 accumulation on
 * v_mfma_f32_16x16x16_f16; the guided solve then runs a whole sample per launch with the network evaluated inside
 * the walk kernel (same field and records as the per-depth launches).
 * "train_precision": 32 (default) or 16 = forward / backward / weight-gradient passes of a training step in that
 * half-precision arithmetic (tiny-cuda-nn trains in half with loss scale 128, guided/parameters.h:13); with 16,
 * wost_net_inference(use_inference_params = 0) evaluates the training weights the way a training step does.
 * Master weights, Adam and the EMA are fp32 in every mode; gradient sums are 64-bit fixed point (reproducible). */
int wost_net_set_option(wost_net_handle h, const char *key, double value);
/* One training step (integrator/guided/integrator.cu:655-662: network->forward, ->backward,
 * trainer->optimizer_step(TRAIN_LOSS_SCALE)): forward with the training parameters, backward of
 * sum_p <dl_dout[p], out[p]>, then (apply_update != 0) one Adam+EMA step on gradient/loss_scale. */
int wost_net_train_step(wost_net_handle h, const float *xy, const float *dl_dout, int32_t n, float loss_scale,
                        int apply_update);

/* ---- guided integrator -------------------------------
 * Replaces GuidedIntegrator<2> as run_expr drives it (reference exec.cu:145-215): the ctor
 * (integrator/guided/integrator.cu:1148-1161), resetNetwork (:1095-1131) and solve()
 * (:1189-1195 -> solveImpl :968-1094).  The first block mirrors GuidedIntegratorSettings
 * (integrator/guided/integrator.h:54-75) plus scene.aabb of the JSON; the second block holds the
 * reference's compile-time constants, exposed so that small frames can be trained in tests. */
typedef struct wost_guided_settings {
    int32_t width, height, spp, max_depth;      /* frameSize, samplesPerPixel, maxWalkingDepth   */
    float eps_shell;                            /* epsilonShell                                  */
    int32_t train_spp_count;                    /* trainSppCount                                 */
    float uniform_fraction_training;            /* uniformFractionInTrainingPhase                */
    float uniform_fraction_guiding;             /* uniformFractionInGuidingPhase                 */
    int32_t max_guided_depth_training;          /* maxGuidedDepthInTrainingPhase                 */
    int32_t max_guided_depth_guiding;           /* maxGuidedDepthInGuidingPhase                  */
    float aabb_min[2], aabb_max[2];             /* scene.aabb (core/problem.cu loadConfig)       */
    int32_t max_train_depth;                    /* 3       integrator.h:237 (<= 4, parameters.h:7) */
    int32_t batch_size;                         /* 524288  parameters.h:11                       */
    int32_t min_batch_size;                     /* 65536   parameters.h:12                       */
    int32_t batches_per_spp;                    /* 5       integrator.h:238                      */
    int32_t train_pixel_stride;                 /* 1       guided.h:104-121                      */
    int32_t train_pixel_offset;                 /* 0; -1 = drawn per solve from the integrator's host sampler when the
                                                   stride is > 1, as the reference does (integrator.cu:126) */
    float loss_scale;                           /* 128     parameters.h:14                       */
} wost_guided_settings;

typedef struct wost_guided_stats {
    uint64_t walk_steps, walks_started, walks_absorbed, walks_truncated, neumann_hits;
    uint64_t guided_steps;       /* steps whose direction was drawn from the mixture              */
    uint64_t train_samples;      /* training records collected over all training passes           */
    uint64_t optimizer_steps;
    double solve_ms;             /* host wall time of wost_guided_solve                           */
    double train_ms;             /* part of it spent building training sets and training          */
    uint32_t kernel_launches;
    uint32_t reserved;           /* trainPixelOffset used by the solve                                */
    uint64_t net_points;         /* network evaluations made for walkers (out-of-shell entries of guided depths) */
    double net_infer_ms;         /* GPU time of the launches that evaluate the network for walkers (HIP events)  */
} wost_guided_stats;

typedef struct wost_guided *wost_guided_handle;

/* Scene upload + LBVH build + network construction (initialised from net_seed). */
int wost_guided_create(const wost_scene_desc *scene, const wost_guided_settings *settings,
                       const wost_net_config *net, uint64_t net_seed, int device, wost_guided_handle *out);
/* The integrator's network, borrowed (valid until wost_guided_destroy): get/set parameters,
 * queryNetwork-style inference (integrator.cu:566-615). */
int wost_guided_network(wost_guided_handle h, wost_net_handle *net);
/* The uploaded scene, borrowed: SDF renders and the batched geometric queries of the guided
 * integrator's scene go through the wost_* entry points above. */
int wost_guided_scene(wost_guided_handle h, wost_handle *scene);
/* queryNetwork (integrator.cu:566-615): raw[n*33] mixture parameters of the inference (EMA)
 * network at world positions pts[n*2] (normalizeSpatialCoord applied inside). */
int wost_guided_query_network(wost_guided_handle h, const float *pts, int32_t n, float *raw);
/* GuidedIntegrator<2>::solve(): all samples, training passes included; field_rgb receives
 * width*height*3 floats = solution / spp.  Starts from the network's current state. */
int wost_guided_solve(wost_guided_handle h, float *field_rgb, wost_guided_stats *stats);
/* Same solve for the 8x8-pixel tiles t with t % shard_count == shard_index (the tiling of
 * wost_solve_sharded).  Every shard trains its OWN copy of the guiding network on the records of
 * its own pixels -- the estimator is unbiased for any network state, so no collective is needed
 * on the data path.  field_rgb_dev: DEVICE buffer of width*height*3 floats; pixels of other
 * shards are written as 0, so a sum-reduce over ranks (RCCL) yields the full field.  Returns
 * after the work has completed. */
int wost_guided_solve_sharded(wost_guided_handle h, int32_t shard_index, int32_t shard_count,
                              float *field_rgb_dev, wost_guided_stats *stats);
/* The guided solve at n evaluation points of the caller (pts_xy: n * 2 floats) instead of the pixels of the frame: wost_solve_points
 * for the guided integrator.  The driver and the kernels are those of wost_guided_solve; only where a walker starts differs.
 *   Point identity.  Point i takes the place of pixel i of a guided solve over n pixels: it is walked with the handle's settings,
 *     meshes, source term, guiding box and network; all its samples share the PCG32 stream seeded as the reference seeds pixel
 *     seed_base + i of a frame seed_width wide; field_rgb[3 i ..] receives solution / spp.  It is a training point iff the sample
 *     is a training sample and (i - trainPixelOffset) % trainPixelStride == 0, with i the index IN THE CALL; trainPixelOffset is
 *     fixed or drawn from the handle's host sampler exactly as a frame solve draws it: one draw per solve.
 *   Frame equivalence.  The frame's own evaluation points in row-major order with seed_base = 0, seed_width = width and
 *     train_spp_count = -1 reproduce wost_guided_solve bit for bit on a frame without a mask: the field, the counters, the training
 *     sets and the trained weights.
 *   train_spp_count.  -1: the handle's setting.  >= 0 overrides it for this call: the first min(spp, train_spp_count) samples
 *     train; 0 = a frozen network, the guiding-phase settings from the first sample on.  < -1: WOST_ERR_INVALID.  The call starts
 *     from the network's current state and leaves the trained state behind, as wost_guided_solve does -- so a handle can train on
 *     a frame once (wost_guided_solve) and then be probed anywhere with train_spp_count = 0.  With 0 the result of a point does
 *     not depend on how a list is cut into calls, as long as seed_base moves with the cut.  With training the list trains ONE
 *     network: every point sees what all points of the call have taught it, so a cut changes the result.
 *   Capacity.  n <= width * height of the handle: the per-pixel state, the record sets and the queues are sized by the frame, and a
 *     guided solve cannot be run in chunks without changing what the network sees.  A longer list is WOST_ERR_INVALID; the message
 *     names the capacity.
 *   The frame's mask, the shards and the intermediate-frame callback do not apply.  The options "pipeline" and "train_group" and the
 *     network's "precision" / "train_precision" are honoured exactly as by the frame solve.  Afterwards wost_guided_train_set returns
 *     the last training pass of the point solve.
 *   Arguments, checked in this order before the handle is read or a device is asked for: a null handle, list or field; n < 0;
 *     seed_width <= 0; seed_base < 0 or seed_base + n > 2^28; train_spp_count < -1.  n == 0: WOST_OK and zeroed stats.
 * wost_guided_solve_points: host arrays; a non-finite coordinate is refused (WOST_ERR_INVALID names the first bad index, nothing
 * is launched).  wost_guided_solve_points_dev: DEVICE arrays, complete when the call is made; the work runs on the handle's own
 * stream and the call returns when it is complete, like wost_guided_solve_sharded; a point with a non-finite coordinate is never
 * walked and never recorded, its field entry is NaN. */
int wost_guided_solve_points(wost_guided_handle h, const float *pts_xy, int32_t n, int32_t seed_base, int32_t seed_width,
                             int32_t train_spp_count, float *field_rgb, wost_guided_stats *stats);
int wost_guided_solve_points_dev(wost_guided_handle h, const float *pts_xy_dev, int32_t n, int32_t seed_base, int32_t seed_width,
                                 int32_t train_spp_count, float *field_rgb_dev, wost_guided_stats *stats);
/* Shared network across shards (optional).  By default every shard trains its own network; with
 * a sync callback the shards train ONE network: before every Adam step the callback must sum the
 * fixed-point gradient buffer over all ranks (WOST_SYNC_SUM_I64_DEVICE: data = device int64[count],
 * e.g. ncclAllReduce(.., ncclInt64, ncclSum, ..) followed by a stream synchronisation), and once per
 * training pass it must reduce the number of usable batches to the minimum over the ranks
 * (WOST_SYNC_MIN_I64_HOST: data = host int64[1]).  Integer sums make the result independent of
 * the reduction order: all ranks hold the same network bit for bit.  At the start of a solve the
 * callback is asked once for the number of ranks (WOST_SYNC_RANKS_I64_HOST: it writes host
 * int64[1]); the summed gradient is divided by it before the Adam step, so that a shared step is
 * the step of ONE batch of ranks x batch_size samples (each rank normalises its loss gradient by
 * its own batch) and the L2 term and epsilon keep their weight for any rank count.  (The op exists since library
 * version 0.2, wost_version(); a callback written against 0.1 answers it with WOST_SYNC_UNSUPPORTED and gets the summed
 * gradient undivided, with a warning on stderr.)
 * The divisor belongs to the solve: afterwards wost_net_train_step on the same network is a plain single-rank step.
 * Return 0 on success, WOST_SYNC_UNSUPPORTED for an op the callback does not know, any other value for a failure:
 * a failure of ANY op -- or a rank count below 1 -- fails the solve with WOST_ERR_DEVICE (a rank that trained on while
 * another one failed would let the "shared" weights diverge silently). */
#define WOST_SYNC_SUM_I64_DEVICE 0
#define WOST_SYNC_MIN_I64_HOST 1
#define WOST_SYNC_RANKS_I64_HOST 2
#define WOST_SYNC_UNSUPPORTED 2      /* return value of a callback for an unknown op */
typedef int (*wost_sync_fn)(void *user, int op, void *data, uint64_t count);
int wost_guided_set_sync(wost_guided_handle h, wost_sync_fn fn, void *user);
/* Intermediate frames (saveSppMetrics* / saveTimeMetrics* of GuidedIntegratorSettings, reference
 * integrator/guided/integrator.cu:1049-1081): during wost_guided_solve the callback receives
 * solution / (sample_id + 1) after sample sample_id when  spp_every > 0 && sample_id % spp_every
 * == 0 && sample_id < spp_until  (reason 0), and when  time_every > 0 && sample_id % time_every
 * == 0  (reason 1, with the milliseconds since the start of the solve).  Return 0 to continue. */
typedef int (*wost_frame_fn)(void *user, int reason, int32_t sample_id, double elapsed_ms, const float *field_rgb);
int wost_guided_set_frame_callback(wost_guided_handle h, wost_frame_fn fn, void *user, int32_t spp_every,
                                   int32_t spp_until, int32_t time_every);
/* The training set built by the most recent training pass, in (pixel, record) order
 * (generate_training_data, train.h:423-471): xy[n*2] normalised positions, dir[n*2],
 * solution[n*3] = |record.solution / record.thp|, dir_pdf[n], normal[n*2], on_neumann[n].
 * Copies min(n, capacity) entries; any output array may be NULL. */
int wost_guided_train_set(wost_guided_handle h, int32_t capacity, int32_t *n, float *xy, float *dir,
                          float *solution, float *dir_pdf, float *normal, uint8_t *on_neumann);
/* Options of a guided handle; unknown keys -> WOST_ERR_INVALID.
 * "pipeline" (0 default / 1): the PIPELINED training order.  The reference trains between the samples
 * (integrator/guided/integrator.cu:968-1094: walk of sample k, trainStep on its records, walk of sample k + 1 with the new
 * weights); with "pipeline" 1 sample k + 1 walks with a frozen copy of the weights that the training pass of sample k - 1
 * left while the pass of sample k runs on a second stream -- no barrier between walking and training.  The estimator
 * stays unbiased for any network state (direction and one-sample-MIS density of a sample come from the same copy, the
 * training records carry the density they were drawn with); the field differs from the exact order's statistically, so
 * this is never the parity mode: default off, and a solve with intermediate frames falls back to the exact order.
 * "train_group" (1 default .. 16): a training launch walks up to that many samples of every pixel, each with its own record
 * set, and their training passes follow the launch (with "pipeline" 1: on the second stream, while the next group walks): the
 * drain of a sample's longest walks is paid once per group.  The groups grow with the training -- the launch that starts at
 * sample s covers min(S, max(1, s / 2)) samples, never more than half of what has been trained before it -- so the first
 * samples, from which the network learns fastest, keep the reference's order.  The same statistical contract as "pipeline";
 * 1 = the reference's order throughout (a training pass between any two samples). */
int wost_guided_set_option(wost_guided_handle h, const char *key, double value);
int wost_guided_destroy(wost_guided_handle h);

/* The launches of the last wost_solve / wost_solve_sharded / wost_solve_points[_dev] of this handle, in order (bench.py prices the dominant one against
 * the roofline; the reference has no counterpart: its solveImpl issues 2 + 5 * depth full-frame launches per sample,
 * integrator/uniform/integrator.cu:529-623).  Writes min(*count, capacity) records.  After wost_solve_gradient_points[_dev]: the
 * walk launches of the call's LAST block of points only. */
typedef struct wost_launch_info {
    int32_t kind;             /* WOST_LAUNCH_* */
    uint32_t walkers;         /* walkers (pixels in flight) the launch started with                                      */
    uint32_t walkers_beside;  /* walkers started with it on other streams: long remainders, strayed walkers               */
    uint32_t grid;            /* workgroups                                                                              */
    double ms;                /* HIP events around it on the solve's stream (what ran beside it ends inside later spans) */
    uint64_t walk_steps_done; /* walk steps of the solve counted when the launch had ended (cumulative, all streams)      */
} wost_launch_info;
enum {
    WOST_LAUNCH_ROUND = 0,       /* walk_round_kernel: every walker up to steps_per_round steps, then compaction          */
    WOST_LAUNCH_QUAD = 1,        /* walk_quad_kernel: the same with four lanes per walker (under-filled launches)         */
    WOST_LAUNCH_ONE = 2,         /* few samples per pixel: resident lanes drain the queue, the whole solve in one launch   */
    WOST_LAUNCH_PERSISTENT = 3,  /* many samples per pixel: resident lanes take whole pixels, longest expected chain first,
                                    until none is unread; what they hold then goes to rounds                              */
    WOST_LAUNCH_WAIT = 4,        /* no launch: the time the solve waited at its end for what ran beside the rounds         */
    WOST_LAUNCH_BESIDE = 5       /* a pass without an ordinary launch: every walker it had started on the other streams
                                    (walkers = 0, grid = 0, walkers_beside > 0)                                            */
};
/* Every record but WOST_LAUNCH_WAIT is one pass of the solve, and wost_stats.kernel_launches counts those passes: a record of kind
 * ROUND, QUAD, ONE or PERSISTENT has walkers > 0 and grid > 0. */
int wost_last_launches(wost_handle h, wost_launch_info *out, int32_t capacity, int32_t *count);

/* Tuning knobs ("steps_per_round", "block_size", "refill", "thin_waves", ...; scheduling only,
 * never the result); unknown keys -> WOST_ERR_INVALID.
 * "persist" (-1 automatic / 0 / 1): the persistent first launch of a solve with many samples per pixel and more walkers than
 * resident lanes (WOST_LAUNCH_PERSISTENT); "persist_order" 0: in queue order instead of longest-first; "long_steps" (a multiple
 * of 8 in 0..32760, default 1024; 0 = none; larger values are refused: the order by estimate tells no estimates apart beyond
 * 32760): pixels that launch hands over with at least that many walk steps expected still run to their
 * end beside the rounds of the others, the first "long_thin" (2048) of them four to a wave, at most "long_cap" (32768);
 * "tail_sort" (1): the first round after it takes its walkers in the order of their expected remainders; "few_order" (1): the
 * one-launch path of few samples per pixel takes the pixels longest-first too; "resident_blocks": workgroups of those launches
 * (0 = what the chip holds); "dry_stop" (1): once the input queue of the persistent launch is dry every wave stops at its next
 * look at the queue's cursor and hands its pixels over (0: only a wave that needs a refill does), "dry_cadence" (a power of two
 * in 1..1024, default 4): near the end of the queue a wave looks again after that many walk steps of its busiest lane;
 * "chain_start" (1): a lane whose walk is absorbed takes the first step of its pixel's next sample, whose closest point is cached,
 * in the same pass over the step code (0: in the wave's next one).  The 2-D uniform walk kernels only, and not the steps a wave
 * takes together for a Neumann mesh on the tree.
 * "root_visit" (1): a lane of the 2-D round kernels that begins a closest-point query visits the root of the Dirichlet tree in
 * the same pass over the step code, the root's record read once per wave (0: in its first traversal burst, as a per-lane fetch).
 * The result and every counter but trav_trips are the same either way.
 * "spp" changes samplesPerPixel of an existing handle (a pixel's first k samples do not depend on
 * the total, so solving with spp = k reproduces the state of a longer solve after k samples: the
 * host mirror uses this for saveSppMetrics frames).
 * "grad_source" (exactly 0, the default, or 1) is no tuning knob: 1 lets the gradient calls take a scene with a source term
 * ("The gradient on a scene with a source term" above).
 * "exits_grad_source" (exactly 0, the default, or 1) is none either: 1 lets wost_exits_walk_gradient take such a scene and carry
 * the in-ball term in the list ("Exit lists of the gradient", item 4); a key of its own, read at the walk alone. */
int wost_set_option(wost_handle h, const char *key, double value);

int wost_destroy(wost_handle h);

/* ---- 3-D: UniformIntegrator<3> on triangle meshes ---------------------------------
 * Replaces Problem<3> geometry upload (core/problem.h:197-260, core/problem.cu:262-270) and
 * UniformIntegrator<3>::solve() -- the DIM == 3 branches of integrator/uniform/integrator.cu
 * (:150-168 triangle side / barycentric uv and the in-shell test, :343-365 three Neumann draws,
 * :465-525 oneStepWalk), EvaluationGrid<3> (core/evaluation_grid.h:43-70), HarmonicGreenBall<3>
 * (util/green.h:77-119), uniformSampleSphere<3> / Hemisphere<3> (util/sampling.h:20-27,57-66) and
 * frameFromNormal(Vector3f) (util/transformation.h:62-67).  colors: per vertex 6 floats, rgb on the
 * side the triangle normal (p1-p0) x (p2-p0) points to, then rgb on the other side
 * (thrust::pair first / second, integrator/common.h:250-257).  Neumann meshes of any size (flat loops up to 64
 * triangles, the LBVH with normal cones beyond), optional source term (wost3_source_desc). */
typedef struct wost3_mesh_desc {
    int32_t n_verts, n_tris;
    const float *verts;       /* n_verts * 3 */
    const int32_t *tris;      /* n_tris * 3, 0-based */
    const float *colors;      /* n_verts * 6 or NULL = zeros */
} wost3_mesh_desc;
/* Source term f of laplace(u) = -f in 3-D (Problem<3>::source_vdb_ptr, core/problem.cu:136-149; sampled at
 * integrator/uniform/integrator.cu:296-304): dense grid of RGB samples at integer index coordinates,
 * index = world * index_scale + index_offset per axis, trilinear, zero outside.  nx == 0 disables the source term. */
typedef struct wost3_source_desc {
    int32_t nx, ny, nz;
    const float *rgb;                        /* nz * ny * nx * 3, x fastest */
    float index_scale[3], index_offset[3];
    float intensity;                         /* source_intensity (core/problem.cu:179) */
} wost3_source_desc;
typedef struct wost3_scene_desc {
    wost3_mesh_desc dirichlet, neumann;      /* n_tris == 0 -> disabled */
    float dirichlet_intensity, neumann_intensity;
    float probe_scale;                       /* EvaluationGrid<3>::ProbeData: point = scale (ndc.x right + ndc.y up) + pos */
    float probe_pos[3], probe_up[3], probe_right[3];
    const uint8_t *mask;                     /* width*height bytes (0 = masked out) or NULL */
    wost3_source_desc source;                /* zero-initialised = no source term */
} wost3_scene_desc;
typedef struct wost3_context *wost3_handle;
int wost3_create(const wost3_scene_desc *scene, const wost_settings *settings, int device, wost3_handle *out);
/* UniformIntegrator<3>::solve() for the pixels [pixel_begin, pixel_end): field_rgb = (n, 3) host floats */
int wost3_solve(wost3_handle h, int32_t pixel_begin, int32_t pixel_end, float *field_rgb, wost_stats *stats);
/* the 8x8 pixel tiles t % shard_count == shard_index into a zero-filled full-frame DEVICE buffer (as wost_solve_sharded) */
int wost3_solve_sharded(wost3_handle h, int32_t shard_index, int32_t shard_count, float *field_rgb_dev, void *stream,
                        wost_stats *stats);
/* The solve at n evaluation points of the caller (pts_xyz: n * 3 floats), which need not lie on one slice: wost_solve_points in
 * 3-D, with the same rules (stream of pixel seed_base + i in a frame seed_width wide, integrator/uniform/integrator.cu:71-77;
 * no mask; seed_base + n <= 2^28; non-finite coordinates refused by the host variant and answered with NaN, unwalked, by the
 * device variant).  The reference has no counterpart: its EvaluationGrid is the only probe (core/evaluation_grid.h).  Lanes
 * hold the walkers, so a list of any length is one launch. */
int wost3_solve_points(wost3_handle h, const float *pts_xyz, int32_t n, int32_t seed_base, int32_t seed_width, float *field_rgb,
                       wost_stats *stats);
int wost3_solve_points_dev(wost3_handle h, const float *pts_xyz_dev, int32_t n, int32_t seed_base, int32_t seed_width,
                           float *field_rgb_dev, void *stream, wost_stats *stats);
/* The continued frame solve in 3-D: wost_solve_more & co. with the same rules (one carried solve per handle, bound to its shard;
 * the field after any sequence of calls is wost3_solve's at spp = done, bit for bit). */
int wost3_solve_more(wost3_handle h, int32_t more_spp, float *field_rgb, wost_stats *stats);
int wost3_solve_more_sharded(wost3_handle h, int32_t shard_index, int32_t shard_count, int32_t more_spp, float *field_rgb_dev,
                             void *stream, wost_stats *stats);
int wost3_solve_restart(wost3_handle h);
int wost3_solve_progress(wost3_handle h, int32_t *spp_done);
/* ... and its selections, per-pixel state and adaptive solves (wost_solve_more_where & co., the same rules) */
int wost3_solve_more_where(wost3_handle h, int32_t more_spp, const uint8_t *select, float *field_rgb, wost_stats *stats);
int wost3_solve_more_where_sharded(wost3_handle h, int32_t shard_index, int32_t shard_count, int32_t more_spp,
                                   const uint8_t *select_dev, float *field_rgb_dev, void *stream, wost_stats *stats);
int wost3_solve_carried(wost3_handle h, int32_t *spp, int32_t *batches, float *sum_rgb, float *stderr_rgb);
int wost3_solve_adaptive(wost3_handle h, const wost_adaptive *a, float *field_rgb, float *stderr_rgb, int32_t *spp_map,
                         wost_stats *stats);
int wost3_solve_adaptive_sharded(wost3_handle h, int32_t shard_index, int32_t shard_count, const wost_adaptive *a,
                                 float *field_rgb_dev, void *stream, wost_stats *stats);
/* The carried point list in 3-D: wost_points_carry & co. with the same rules in every clause (pts_xyz: n * 3 floats, which need not
 * lie on one slice; one list per handle beside the carried frame solve; a point's field after any sequence of calls is
 * wost3_solve_points' at spp = n_i, bit for bit).  Lanes hold the walkers, so a call on a list of any length is one launch, sized
 * by the selection. */
int wost3_points_carry(wost3_handle h, const float *pts_xyz, int32_t n, int32_t seed_base, int32_t seed_width);
int wost3_points_carry_dev(wost3_handle h, const float *pts_xyz_dev, int32_t n, int32_t seed_base, int32_t seed_width, void *stream);
int wost3_points_more(wost3_handle h, int32_t more_spp, const uint8_t *select, float *field_rgb, wost_stats *stats);
int wost3_points_more_dev(wost3_handle h, int32_t more_spp, const uint8_t *select_dev, float *field_rgb_dev, void *stream,
                          wost_stats *stats);
int wost3_points_carried(wost3_handle h, int32_t *spp, int32_t *batches, float *sum_rgb, float *stderr_rgb);
int wost3_points_adaptive(wost3_handle h, const wost_adaptive *a, float *field_rgb, float *stderr_rgb, int32_t *spp_map,
                          wost_stats *stats);
int wost3_points_adaptive_dev(wost3_handle h, const wost_adaptive *a, float *field_rgb_dev, void *stream, wost_stats *stats);
int wost3_points_restart(wost3_handle h);
int wost3_points_progress(wost3_handle h, int32_t *n_points, int32_t *spp_done);
/* The gradient at the caller's points in 3-D: wost_solve_gradient_points with the same rules in every clause (pts_xyz: n * 3
 * floats; DIM = 3, so grad holds n * 9 floats; the distances are wost3_closest_point's; every block is one launch). */
int wost3_solve_gradient_points(wost3_handle h, const float *pts_xyz, int32_t n, int32_t seed_base, int32_t walk_seed_base,
                                int32_t seed_width, const wost_gradient_out *out, wost_stats *stats);
int wost3_solve_gradient_points_dev(wost3_handle h, const float *pts_xyz_dev, int32_t n, int32_t seed_base, int32_t walk_seed_base,
                                    int32_t seed_width, const wost_gradient_out *out, void *stream, wost_stats *stats);
/* The carried gradient list in 3-D: wost_gradient_points_carry & co. with the same rules in every clause (pts_xyz: n * 3 floats;
 * DIM = 3; a batch is a row of wost3_solve_gradient_points). */
int wost3_gradient_points_carry(wost3_handle h, const float *pts_xyz, int32_t n, int32_t batch_walks, int32_t round_stride, int32_t max_rounds,
                                int32_t seed_base, int32_t walk_seed_base, int32_t seed_width);
int wost3_gradient_points_carry_dev(wost3_handle h, const float *pts_xyz_dev, int32_t n, int32_t batch_walks, int32_t round_stride,
                                    int32_t max_rounds, int32_t seed_base, int32_t walk_seed_base, int32_t seed_width, void *stream);
int wost3_gradient_points_more(wost3_handle h, const uint8_t *select, const wost_gradient_carried_out *out, wost_stats *stats);
int wost3_gradient_points_more_dev(wost3_handle h, const uint8_t *select_dev, const wost_gradient_carried_out *out_dev, void *stream,
                                   wost_stats *stats);
int wost3_gradient_points_carried(wost3_handle h, const wost_gradient_carried_out *out);
int wost3_gradient_points_adaptive(wost3_handle h, const wost_gradient_adaptive *a, const wost_gradient_carried_out *out, wost_stats *stats);
int wost3_gradient_points_adaptive_dev(wost3_handle h, const wost_gradient_adaptive *a, const wost_gradient_carried_out *out_dev, void *stream,
                                       wost_stats *stats);
int wost3_gradient_points_restart(wost3_handle h);
int wost3_gradient_points_progress(wost3_handle h, int32_t *n_points, int32_t *rounds_done);
/* Exit lists in 3-D: wost_exits_walk & co. with the same rules in every clause (pts_xyz: n * 3 floats; DIM = 3: prim is the index
 * of the absorbing triangle in the caller's triangle array, uv holds u and v of a walk side by side, the weights of the
 * triangle's three vertices are 1 - u - v, u, v; colours in the layout of wost3_mesh_desc.colors). */
int wost3_exits_walk(wost3_handle h, const float *pts_xyz, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width,
                     wost_stats *stats);
int wost3_exits_walk_dev(wost3_handle h, const float *pts_xyz_dev, int32_t n, int32_t walks, int32_t walk_seed_base, int32_t seed_width,
                         void *stream, wost_stats *stats);
int wost3_exits_records(wost3_handle h, const wost_exit_records *out);
int wost3_exits_apply(wost3_handle h, const float *colors, int32_t K, float *field_rgb, float *stderr_rgb);
int wost3_exits_apply_dev(wost3_handle h, const float *colors_dev, int32_t K, float *field_rgb_dev, float *stderr_rgb_dev, void *stream);
int wost3_exits_adjoint(wost3_handle h, const float *dfield, int32_t K, float *dcolors);
int wost3_exits_adjoint_dev(wost3_handle h, const float *dfield_dev, int32_t K, float *dcolors_dev, void *stream);
int wost3_exits_progress(wost3_handle h, int32_t *n_points, int32_t *walks);
/* Exit lists of the gradient in 3-D: wost_exits_walk_gradient & co. with the same rules in every clause (DIM = 3: two draws per
 * direction as in wost3_solve_gradient_points; grad, grad_stderr and dgrad hold K * n * 3 * 3 floats). */
int wost3_exits_walk_gradient(wost3_handle h, const float *pts_xyz, int32_t n, int32_t walks, int32_t seed_base, int32_t walk_seed_base,
                              int32_t seed_width, wost_stats *stats);
int wost3_exits_walk_gradient_dev(wost3_handle h, const float *pts_xyz_dev, int32_t n, int32_t walks, int32_t seed_base, int32_t walk_seed_base,
                                  int32_t seed_width, void *stream, wost_stats *stats);
int wost3_exits_gradient_records(wost3_handle h, const wost_exit_gradient_records *out);
int wost3_exits_apply_gradient(wost3_handle h, const float *colors, int32_t K, float *grad, float *grad_stderr, float *field_rgb);
int wost3_exits_apply_gradient_dev(wost3_handle h, const float *colors_dev, int32_t K, float *grad_dev, float *grad_stderr_dev,
                                   float *field_rgb_dev, void *stream);
int wost3_exits_gradient_terms(wost3_handle h, double *T, double *seT, double *U);
int wost3_exits_adjoint_gradient(wost3_handle h, const float *dgrad, int32_t K, float *dcolors);
int wost3_exits_adjoint_gradient_dev(wost3_handle h, const float *dgrad_dev, int32_t K, float *dcolors_dev, void *stream);
/* The index and the ordered adjoint in 3-D: wost_exits_index & co. with the same rules in every clause (DIM = 3: three
 * incidences per absorbed walk, v = tris[prim][j], three axes in q). */
int wost3_exits_index(wost3_handle h);
int wost3_exits_index_info(wost3_handle h, int64_t *n_incidences, int64_t *longest_bin);
int wost3_exits_index_records(wost3_handle h, int64_t *bin_begin, int32_t *inc);
int wost3_exits_adjoint_ordered(wost3_handle h, const float *dfield, int32_t K, float *dcolors);
int wost3_exits_adjoint_ordered_dev(wost3_handle h, const float *dfield_dev, int32_t K, float *dcolors_dev, void *stream);
int wost3_exits_adjoint_gradient_ordered(wost3_handle h, const float *dgrad, int32_t K, float *dcolors);
int wost3_exits_adjoint_gradient_ordered_dev(wost3_handle h, const float *dgrad_dev, int32_t K, float *dcolors_dev, void *stream);
/* lbvh::nearest + checkPointSide + computeProjectionRatio for triangles (call sites integrator.cu:138,154-155):
 * winning triangle (lowest index on ties), distance, barycentric (u, v) of the projection, side */
int wost3_closest_point(wost3_handle h, int which_mesh, const float *pts, int32_t n, int32_t *out_idx, float *out_dist,
                        float *out_uv, int32_t *out_side);
/* lbvh::nearest_silhouette in 3-D: distance to the closest silhouette EDGE within rmax (NULL = unbounded) */
int wost3_closest_silhouette(wost3_handle h, int which_mesh, const float *pts, const float *rmax, int32_t n, float *out_dist);
/* lbvh::ray_intersect on triangles: closest hit (flag, t, triangle) */
int wost3_ray_intersect(wost3_handle h, int which_mesh, const float *origins, const float *dirs, const float *tmax, int32_t n,
                        int32_t *out_hit, float *out_t, int32_t *out_idx);
/* Problem<3>::build_bvh (core/problem.cu:31-37, 48-54: the reference builds its trees on the device).  wost3_create builds
 * every mesh with HIP kernels (csrc/wost_build3.hip); this developer / test entry builds `mesh` with those kernels AND with the
 * host builder kept as their checker, `repeat` times, and compares the two uploaded meshes byte for byte:
 * mismatch[0..13] = differing bytes of nodes, tri, triOrig, slotOfOrig, triVerts, colors, flat, flatVerts, edges, slotEdges,
 * cones, obox, areas, sampTri; [14] = differing scalars (the arrays are not compared then); [15] = bytes compared.
 * host_ms / device_ms (either may be NULL) = the fastest wall-clock time of each build, uploads and the final wait included. */
int wost3_mesh_build_check(const wost3_mesh_desc *mesh, int device, int32_t repeat, double *host_ms, double *device_ms,
                           int64_t *mismatch);
/* VMF (reference util/vmf.h:21-70), the lobe of the 3-D guided integrator's mixture (that integrator is not built; this is
 * its distribution layer, batch entry points over HOST arrays like wost_vonmises_*): eval(cosTheta) for n (kappa,
 * cos_theta) pairs; sample(sampler, mu): per point a PCG32 stream setSeed(seed[i], 1) and per_point consecutive unit
 * directions about mu[n*3] in dirs[n*per_point*3]. */
int wost3_vmf_eval(int device, const float *kappa, const float *cos_theta, int32_t n, float *pdf);
int wost3_vmf_sample(int device, const float *kappa, const float *mu, const uint64_t *seed, int32_t n, int32_t per_point,
                     float *dirs);
/* VMM<3,8> built from 40 raw network outputs per point (integrator/guided/distribution.h:279-345, train.h:50-79 with
 * common3d: 8 x (lambda, kappa, mean vector)): mixture pdf at direction wi[n*3] (pdf may be NULL) and one sampled
 * direction per point with the stream setSeed(seed[i], 1) (sample_dir may be NULL). */
int wost3_vmm_pdf_sample(int device, const float *raw, const float *wi, const uint64_t *seed, int32_t n, float *pdf,
                         float *sample_dir);
/* compute_dL_doutput_divergence with common3d::GuidedOutput (train.h:492-553) around VMM<3,N>::gradients_probability
 * (distribution.h:348-421): raw and dl_draw 41 floats per sample (the selection logit last); record dir[n*3], li, dir_pdf,
 * on_neumann (may be NULL), normal[n*3]; likelihood may be NULL. */
int wost3_vmm_loss_gradients(int device, const float *raw, const float *dir, const float *li, const float *dir_pdf,
                             const uint8_t *on_neumann, const float *normal, int32_t n, float loss_scale, float *dl_draw,
                             float *likelihood);
/* renderDirichletSDF / renderSilhouetteSDF / renderSource with DIM = 3 (integrator/common.h:52-163): one query per pixel
 * of the frame at its evaluation point; which_mesh as above; out_dist width*height floats (+inf without that mesh),
 * out_rgb width*height*3 floats (zeros without a source term) */
int wost3_render_sdf(wost3_handle h, int which_mesh, float *out_dist);
int wost3_render_source(wost3_handle h, float *out_rgb);
/* The options of a 3-D handle, as wost_set_option: "grad_source" and "exits_grad_source" (0 / 1 each, the rules of
 * wost_set_option's) are the only keys; any other is WOST_ERR_INVALID "unknown option: KEY", a null handle or key WOST_ERR_INVALID "null argument". */
int wost3_set_option(wost3_handle h, const char *key, double value);
int wost3_destroy(wost3_handle h);

/* ---- 3-D: GuidedIntegrator<3> (SURVEY.md 8a rows a21-a27 with DIM == 3) -----------------------------------------------
 * Replaces the GuidedIntegrator<3> alternative of run_expr's variant (exec.cu:102-122) and its solve() -- the DIM == 3
 * branches of integrator/guided/integrator.cu (:181-215 triangle side / barycentric uv, :347 three Neumann draws, :508-511,
 * :690-693, :800-803 VMM<3,8> and the reflection about the Neumann normal), guided/parameters.h:26-33 (3 network inputs,
 * 8 x (lambda, kappa, mean vector) + selection logit = 41 outputs padded to 48), train.h:289-353 (3-D records) -- on the
 * scene types of the 3-D uniform integrator above.  The network is the one of wost3_net_create: the DenseGrid encoding
 * with three inputs (trilinear, res^3 entries per level), otherwise the configuration of data/ladybug/n.json:49-81; fp32.
 * Scenes with a source term are solved like the others (sampleSourceImpl with DIM == 3, integrator.cu:277-364; the
 * dense-grid stand-in for nanovdb of wost3_source_desc): tests/test_guided_3d.py::test_gpu_guided3_source_term_matches_oracle. */
int wost3_net_create(int device, const wost_net_config *cfg, uint64_t seed, wost_net_handle *out);   /* inputs: 3 floats per point */
typedef struct wost3_guided_settings {
    int32_t width, height, spp, max_depth;
    float eps_shell;
    int32_t train_spp_count;
    float uniform_fraction_training, uniform_fraction_guiding;
    int32_t max_guided_depth_training, max_guided_depth_guiding;
    float aabb_min[3], aabb_max[3];             /* scene.aabb */
    int32_t max_train_depth, batch_size, min_batch_size, batches_per_spp, train_pixel_stride, train_pixel_offset;
    float loss_scale;                           /* meanings and reference defaults as in wost_guided_settings */
} wost3_guided_settings;
typedef struct wost3_guided *wost3_guided_handle;
/* integrator/guided/integrator.h:127,175 (ctor + resetNetwork) with DIM == 3; net->n_output must be 41 */
int wost3_guided_create(const wost3_scene_desc *scene, const wost3_guided_settings *settings, const wost_net_config *net,
                        uint64_t net_seed, int device, wost3_guided_handle *out);
int wost3_guided_destroy(wost3_guided_handle h);
int wost3_guided_network(wost3_guided_handle h, wost_net_handle *net);            /* borrowed: owned by the integrator */
int wost3_guided_scene(wost3_guided_handle h, wost3_handle *scene);               /* borrowed: for the SDF / source channels */
/* solve() (integrator.cu:1189-1195): field_rgb = width*height*3 floats on the host / in device memory (tile shard as in
 * wost3_solve_sharded, every shard its own network) */
int wost3_guided_solve(wost3_guided_handle h, float *field_rgb, wost_guided_stats *stats);
int wost3_guided_solve_sharded(wost3_guided_handle h, int32_t shard_index, int32_t shard_count, float *field_rgb_dev,
                               wost_guided_stats *stats);
/* The guided solve at n evaluation points of the caller (pts_xyz: n * 3 floats), which need not lie on one slice: the contract of
 * wost_guided_solve_points in every clause (point identity, frame equivalence with wost3_guided_solve, train_spp_count, the capacity
 * n <= width * height, the argument checks, host and device variants), with wost3_guided_train_set afterwards. */
int wost3_guided_solve_points(wost3_guided_handle h, const float *pts_xyz, int32_t n, int32_t seed_base, int32_t seed_width,
                              int32_t train_spp_count, float *field_rgb, wost_guided_stats *stats);
int wost3_guided_solve_points_dev(wost3_guided_handle h, const float *pts_xyz_dev, int32_t n, int32_t seed_base, int32_t seed_width,
                                  int32_t train_spp_count, float *field_rgb_dev, wost_guided_stats *stats);
/* queryNetwork(Vector3f) (exec.cu:175-186): raw = n * 41 mixture parameters of the inference weights at pts (n * 3, world) */
int wost3_guided_query_network(wost3_guided_handle h, const float *pts, int32_t n, float *raw);
/* the ordered training set of the last training pass (tests): xyz = normalised inputs, dir / normal 3 floats per sample */
int wost3_guided_train_set(wost3_guided_handle h, int32_t capacity, int32_t *n, float *xyz, float *dir, float *solution,
                           float *dir_pdf, float *normal, uint8_t *on_neumann);

const char *wost_last_error(void);
const char *wost_version(void);
/* Problem<2>::build_bvh (core/problem.cu:31-37, 48-54: the reference builds its trees on the device).  wost_create builds every
 * mesh of 512 segments or more with HIP kernels (csrc/wost_build2.hip); this developer / test entry builds `mesh` with those kernels
 * AND with the host builder kept as their checker (csrc/lbvh_build.cpp), `repeat` times, and compares the two uploaded trees byte
 * for byte: mismatch[0..13] = differing bytes of nodes, cones, segA, segInv, segOrig, segCol, segVerts, flat, flatCol, sil, silN,
 * scanBox, scanHl, scanId; [14] = differing scalars (the arrays are not compared then); [15] = bytes compared.
 * host_ms / device_ms (either may be NULL) = the fastest wall-clock time of each build, uploads and the final wait included. */
int wost_mesh_build_check(const wost_mesh_desc *mesh, int device, int32_t repeat, double *host_ms, double *device_ms, int64_t *mismatch);

#ifdef __cplusplus
}
#endif
#endif
