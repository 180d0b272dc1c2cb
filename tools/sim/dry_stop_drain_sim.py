"""The drain at the end of the persistent launch, as list scheduling on the CPU (EXPERIMENTS 32).

Resident lanes take whole pixels in the order of a predictor of their length until the queue is dry.  Under the wave-local rule a
wave then walks on until one of ITS lanes completes a pixel and finds no unread slot; under the global look every wave stops
within `cadence` steps of the moment the queue ran dry.  Time is counted in wave-steps (every lane of every resident wave
advances one walk step per unit: the waves share the chip evenly while all of them run).

The input is SYNTHETIC unless --steps names a file of per-pixel step counts (tools/sim/collect_steps_per_pixel.py writes
one: the npz's "steps" array); the synthetic lengths are a broad bulk with a mean near 1 800 steps and 6 % short pixels of 256 .. 420,
ordered by a predictor with a 13.5 % residual (what EXPERIMENTS 25 reports for the distance key).

    python tools/sim/dry_stop_drain_sim.py [--steps steps.npz] [--waves 6144] [--cadence 4]
"""
import argparse
import heapq

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--steps", default=None)
ap.add_argument("--waves", type=int, default=6144)
ap.add_argument("--cadence", type=int, default=4)
ap.add_argument("--residual", type=float, default=0.135)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
rng = np.random.default_rng(a.seed)
if a.steps:
    st = np.load(a.steps)["steps"].astype(np.int64).ravel()
    what = a.steps
else:
    n = 1 << 20
    st = np.maximum(rng.gamma(4.0, 1900.0 / 4.0, n), 430.0)
    short = rng.uniform(size=n) < 0.06
    st[short] = rng.uniform(256, 420, int(short.sum()))
    st = st.astype(np.int64)
    what = "synthetic"
order = np.argsort(-st * np.exp(rng.normal(0.0, a.residual, len(st))), kind="stable")
lanes = a.waves * 64
print("input: %s, %d pixels, mean %.0f steps, %d lanes in %d waves" % (what, len(st), st.mean(), lanes, a.waves))

# list scheduling: the lane that is free first takes the next pixel; `done[l]` collects the moments lane l completed a pixel
heap = [(int(st[order[l]]), l) for l in range(lanes)]
heapq.heapify(heap)
t_dry = 0
for i in order[lanes:]:
    t, l = heapq.heappop(heap)
    t_dry = t                      # the moment this slot was claimed; after the loop: the moment the last slot was
    heapq.heappush(heap, (t + int(st[i]), l))
# the pixel each lane holds when the queue runs dry ends at end[l]: the lane's next completion, its wave's stop under the wave-local rule
end = np.zeros(lanes, np.int64)
for t, l in heap:
    end[l] = t
stop_local = end.reshape(a.waves, 64).min(axis=1) - t_dry
stop_global = np.minimum(stop_local, a.cadence)
for name, s in (("wave-local rule", stop_local), ("global look, cadence %d" % a.cadence, stop_global)):
    idle = (s.max() - s).mean()
    print("%-28s a wave stops %.1f steps after the queue is dry on average, the last one after %d; the chip idles %.1f of those %d step-times; "
          "%d of %d lanes hand a pixel over" % (name, s.mean(), s.max(), idle, s.max(), int((end.reshape(a.waves, 64) - t_dry > s[:, None]).sum()), lanes))
print("steps handed over: wave-local %.3g, global %.3g of %.3g" % (
    np.maximum(end.reshape(a.waves, 64) - t_dry - stop_local[:, None], 0).sum(), np.maximum(end.reshape(a.waves, 64) - t_dry - stop_global[:, None], 0).sum(), st.sum()))
