// wost_carry.h -- the carried frame solve behind wost_solve_more & co., shared by the 2-D and the 3-D
// context: the per-pixel state, the kernel that closes a continued call (wost_carry.hip) and the drivers of the calls that
// continue a selection of pixels or stop by a per-pixel error estimate.  Not part of the C-ABI.
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

}  // namespace wost
