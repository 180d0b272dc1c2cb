// wost_internal2.h -- host-side declarations shared by the translation units of the 2-D uniform path (wost_hip.hip,
// wost_build2.hip; not part of the C-ABI): the uploaded mesh, the walk-state queue and the context behind wost_handle.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/wost.h"
#include "lbvh.h"
#include "wost_device.h"
#include "wost_order.h"
#include "wost_uniform.h"

namespace wost {

struct DeviceMeshStorage {
    DevMesh view{};
    std::vector<void *> allocs;
    HostTree host;
};

// ------------------------------------------------------------------------------------------
// queue layout
// ------------------------------------------------------------------------------------------
struct WalkQueue {
    uint32_t *pix;     // global pixel id
    float *x0, *y0;    // evaluation point of the pixel (start of every sample)
    float *px, *py;    // current walk position
    uint64_t *rng;     // PCG32 state (inc == 1 for every pixel: setSeed(.., seq 0))
    uint32_t *meta;    // sample[0:20) | depth[20:30) | onNeumann[30]
    float *nx, *ny;    // Neumann normal at the current point (valid when onNeumann)
    int32_t *hint;     // slot of the closest Dirichlet segment of the previous step
    float *thp;        // throughput (scalar: all three channels are always equal)
    float *sr, *sg, *sb;  // running solution of the pixel
    float *d0_d2;      // cached closest-point result of the evaluation point (depth 0 of
    int32_t *d0_slot;  //   every sample starts at the same point)
    float *est;        // written when a persistent launch hands a pixel over mid-way: walk steps the pixel is expected to need still
                       //   (not part of a walker's state: no kernel loads it back; the host orders the next launch by it)
};

struct StatsDev;       // the counters of the walk kernels (wost_hip.hip)

}  // namespace wost

// (the handle type of the C-ABI lives outside the namespace.  device, settings, dst, mask, n_pixels, field -- n_pixels * 3, used by
// wost_solve -- stream, the events and the carried states: HandleBase, wost_uniform.h)
struct wost_context : wost::HandleBase {
    wost::DevProbe probe{};
    wost::DeviceMeshStorage dm, nm;
    wost::DevSource src{};          // rgb == nullptr: no source term
    // queues
    void *queue_mem[2] = {nullptr, nullptr};
    wost::WalkQueue queue[2]{};
    uint32_t *counts = nullptr;     // [2]
    wost::StatsDev *stats = nullptr;
    uint32_t *host_count = nullptr; // pinned
    // options
    int steps_per_round = 0;   // 0 = automatic (see run_solve)
    int thin_waves = 1;        // spread the walkers of an under-full launch over more waves
    int block_size = 256;
    int wait_weight = 0;       // 0 = automatic: this and trav_burst per launch (set_schedule)
    int trav_burst = 0;        // 0 = automatic
    int time_kernels = 1;
    int refill = -1;       // -1 = automatic (few samples per pixel), 0 = never, 1 = always
    int persist = -1;      // many samples per pixel, more walkers than resident lanes: the first launch is persistent (lanes take pixels,
                           //   longest expected chain first, until none is left; the rest of the solve runs in rounds): -1 = automatic, 0, 1
    int persist_order = 1; // ... in the order of wost_order.h (0: queue order; comparison runs)
    int few_order = 1;     // the one-launch path of few samples per pixel in that order too (config 2's frame at 1 / 2 / 4 spp: 2.64 -> 2.48, 4.09 -> 3.55, 6.79 -> 5.68 ms)
    int dry_stop = 1;      // the persistent launch: once its input queue is dry every wave stops at its next look at the cursor (1), or only a
                           //   wave that needs a refill does (0: the rule until this option existed; comparison runs)
    int dry_cadence = 4;   // ... a wave looks again after dry_cadence walk steps of its busiest lane (a power of two), less often while the queue is far from dry
    int chain_start = 1;   // the round and quad kernels: a lane whose walk is absorbed takes the depth-0 step of its pixel's next sample in the
                           //   same step trip (1), or in the wave's next one (0: the rule until this option existed; comparison runs)
    int root_visit = 1;    // the round kernels: a lane that begins a closest-point query visits the tree's root in the same step trip, its
                           //   rows read on the scalar path (1), or in its first traversal burst (0: the rule until this option existed; comparison runs)
    int resident_blocks = 0;  // blocks of a one-launch / persistent launch; 0 = as many as the chip holds (tests: a few blocks drain a small frame)
    // what a persistent launch hands over (run_solve): the pixels expected to need `long_steps` walk steps or more run to their end at
    // once, four lanes to a walker, on a stream of higher priority beside the rounds of the others (0 = none do); the first round
    // takes the others in the order of their expected remainders (tail_sort), so that a wave's walkers finish together
    int long_steps = 1024;
    int long_cap = 32768;
    int tail_sort = 1;
    void *long_mem = nullptr;
    wost::WalkQueue long_queue{};
    int long_thin = 2048;         // ... the first long_thin of them four to a wave, the others sixteen
    // Their stream has the highest priority: they are the critical path of the solve's end, and the runtime keeps the hardware
    // queues of a priority level apart from those of the others -- a stream of ordinary priority can land on the hardware queue
    // of the caller's stream (four queues per level), and then the launch meant to run BESIDE the rounds runs behind them (seen
    // in bench.py, which makes a second handle first: the solve waited 27 ms for it).
    hipStream_t long_stream = nullptr;
    hipEvent_t long_ev0 = nullptr, long_ev1 = nullptr;
    wost::WalkOrder order;
    int quad = -1;         // four lanes per walker in under-filled launches: -1 = automatic, 0 = never, 1 = every ordinary round
    double quad_fill = 1.0;   // automatic: when 4 x walkers <= quad_fill x resident lanes
    int coop = 1;             // a Neumann mesh on the tree: its silhouette and ray queries by the wave as a whole (wost_coop.h); 0 = per lane
    int pool_cap = 0;         // ... tasks per pool and wave; 0 = automatic: 128 per level of the Neumann tree (a deeper tree keeps more tasks in flight)
    int ray_slot_trigger = 32;
    uint32_t *cursor = nullptr;
    hipStream_t far_stream = nullptr;          // the launches that take strayed walkers through the SLACK kernel (run_solve)
    hipEvent_t far_ev0 = nullptr, far_ev1 = nullptr;
    int n_cus = 256;
    wost::StatsDev *host_stats = nullptr;            // pinned: the counters as they stood after each launch (last_launches)
    std::vector<wost_launch_info> last_launches;
    uint64_t steps_before = 0;                 // a point solve in chunks: the walk steps of its earlier chunks (wost_launch_info::walk_steps_done)
};
