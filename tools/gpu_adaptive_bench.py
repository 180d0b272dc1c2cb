#!/usr/bin/env python3
"""What the per-pixel state of the carried solve costs a plain continued call, and what an adaptive solve saves.  One process,
one JSON line on stdout (EXPERIMENTS "Adaptive continued solves").

  more1     ladybug 1024^2, depth 64: the wall time of a 1-spp solve_more() call, the first after a restart and the one after
            it, the host clock around the synchronising call.  Uses nothing a tree before the per-pixel state lacks, so the
            same file times both trees; run the two alternately in one session and compare medians against the spread.
  kernels   the same frame: a restart, five 1-spp calls, one call on a 30 % selection and a short adaptive solve -- the work
            to put under `rocprofv3 --kernel-trace --stats` for the time of carry_kernel (88 bytes per pixel when it closes a
            plain call: it reads n, K, sum, prev, q and writes q, prev, K, n and the field).
  adaptive  the same frame: solve_adaptive(batch_spp, min_batches 4, max_spp) at the given tolerances beside the uniform
            solve_more(max_spp): samples used, wall time, and the share of pixels at each count.

    python tools/gpu_adaptive_bench.py more1|kernels|adaptive [--repeats 15] [--max-spp 64] [--batch-spp 4] [--abs-tol 0.05 ...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "n": len(ms)}


def integrator(frame=1024, depth=64):
    from elaina_amd import Problem, UniformIntegrator, UniformIntegratorSettings
    return UniformIntegrator(Problem.load_scene("ladybug"), UniformIntegratorSettings((frame, frame), 1, depth, 1.0))


def bench_more1(repeats):
    it = integrator()
    for _ in range(3):
        it.restart()
        it.solve_more(1)
        it.solve_more(1)
    first, second = [], []
    for _ in range(repeats):
        it.restart()
        first.append(timed(lambda: it.solve_more(1)))
        second.append(timed(lambda: it.solve_more(1)))
    steps = it.last_stats["walk_steps"]
    it.close()
    return {"tree": os.path.basename(_ROOT), "first_call_after_restart": summary(first), "second_call": summary(second), "walk_steps_of_the_last_call": int(steps)}


def bench_kernels():
    it = integrator()
    it.restart()
    for _ in range(5):
        it.solve_more(1)
    it.solve_more_where(1, np.random.default_rng(1).random(it.n_pixels) < 0.3)
    it.solve_adaptive(4, 16, abs_tol=0.05, min_batches=2)
    out = {"spp_done": it.spp_done, "samples": int(it.spp_map.sum())}
    it.close()
    return out


def bench_adaptive(repeats, max_spp, tolerances, batch_spp=4):
    it = integrator()
    out = {"max_spp": max_spp, "batch_spp": batch_spp, "min_batches": 4, "pixels": it.n_pixels, "runs": []}

    def uniform():
        it.restart()
        it.solve_more(max_spp)
    uniform()
    want = it.solution.copy()
    out["uniform"] = dict(summary([timed(uniform) for _ in range(repeats)]), samples=it.n_pixels * max_spp, walk_steps=int(it.last_stats["walk_steps"]))
    for tol in tolerances:
        def adaptive():
            it.restart()
            it.solve_adaptive(batch_spp, max_spp, abs_tol=tol, min_batches=4)
        adaptive()
        full = it.spp_map == max_spp
        assert np.array_equal(it.solution[full], want[full]), "a pixel that ran to max_spp differs from the uniform solve"
        counts, pixels = np.unique(it.spp_map, return_counts=True)
        run = dict(summary([timed(adaptive) for _ in range(repeats)]), abs_tol=tol, samples=int(it.spp_map.sum()),
                   walk_steps=int(it.last_stats["walk_steps"]), kernel_launches=int(it.last_stats["kernel_launches"]),
                   pixels_at_count={int(c): int(p) for c, p in zip(counts, pixels)},
                   rms_stderr=float(np.sqrt(np.mean(np.square(it.stderr[np.isfinite(it.stderr)], dtype=np.float64)))))
        out["runs"].append(run)
    it.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("what", choices=["more1", "kernels", "adaptive"])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--max-spp", type=int, default=64)
    ap.add_argument("--batch-spp", type=int, default=4)
    ap.add_argument("--abs-tol", type=float, action="append", default=[])
    a = ap.parse_args()
    if a.what == "more1":
        line = bench_more1(a.repeats)
    elif a.what == "kernels":
        line = bench_kernels()
    else:
        line = bench_adaptive(max(1, a.repeats // 5), a.max_spp, a.abs_tol or [0.05, 0.02], a.batch_spp)
    print(json.dumps({a.what: line}))


if __name__ == "__main__":
    main()
