#!/usr/bin/env python3
"""What a point solve (wost_solve_points / wost3_solve_points) costs beside the frame solve of the same points, and what the
order of a caller's list costs.  One process, one JSON line on stdout.

  2-D  config 2 (ladybug 1024^2, 256 spp, depth 64): solve() against solve_points of the frame's own points in row-major order
       and under a seeded permutation.  Before anything is timed the walk-step count of the
       row-major point solve is checked against the frame's (1 949 024 384) and its field against solve() bit for bit.
  3-D  the icosphere of bench.py's uniform3d entry at 512^2, 64 spp: solve() (8x8 tiles) against solve_points in row-major order,
       in the order of the tiles, and under the permutation.

Every shape is warmed up, the variants alternate inside each repeat (--repeats, at least 5), times are the host clock around the
synchronising call; per variant the median, the extremes and the launches of the last repeat are reported.

    python tools/gpu_points_bench.py [--repeats 5] [--only 2d|3d]
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

CONFIG2_STEPS = 1949024384


def grid_points2(probe, w, h):
    """eval_point (csrc/wost_device.h) for every pixel, row-major, operation for operation in float32"""
    f = np.float32
    scale, posx, posy, upx, upy = (f(v) for v in probe)
    py, px = np.divmod(np.arange(w * h), w)
    ndcx = f(2.0) * px.astype(f) / f(w) + f(-1.0)
    ndcy = f(2.0) * py.astype(f) / f(h) + f(-1.0)
    ux, uy, vx, vy = upy, -upx, upx, upy
    return np.stack([scale * (ndcx * ux + ndcy * vx) + posx, scale * (ndcx * uy + ndcy * vy) + posy], 1).astype(f)


def grid_points3(probe, w, h):
    """eval_point3 (csrc/wost_device3.h) likewise"""
    f = np.float32
    scale, pos, up, right = probe
    py, px = np.divmod(np.arange(w * h), w)
    ndcx = f(2.0) * px.astype(f) / f(w) + f(-1.0)
    ndcy = f(2.0) * py.astype(f) / f(h) + f(-1.0)
    return np.stack([f(scale) * (ndcx * f(right[k]) + ndcy * f(up[k])) + f(pos[k]) for k in range(3)], 1).astype(f)


def tile_order(w, h):
    """the pixels in the order the frame solves hand them out: 8x8 tiles, row-major inside a tile"""
    py, px = np.divmod(np.arange(w * h), w)
    return np.lexsort((px & 7, py & 7, px >> 3, py >> 3))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(variants, repeats, launches_of=None):
    """variants: {name: callable}; warm up each, then `repeats` rounds with the variants alternating"""
    for fn in variants.values():
        fn()
    ms = {k: [] for k in variants}
    launches = {}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(timed(fn))
            if launches_of is not None:
                launches[k] = launches_of()
    out = {}
    for k, v in ms.items():
        out[k] = {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v), "all_ms": [round(x, 3) for x in v]}
        if k in launches:
            out[k]["launches"] = launches[k]
    return out


def run_2d(repeats):
    from elaina_amd import Problem, UniformIntegrator, UniformIntegratorSettings
    w = 1024
    p = Problem.load_scene("ladybug")
    it = UniformIntegrator(p, UniformIntegratorSettings((w, w), 256, 64, 1.0))
    pts = grid_points2(p.probe, w, w)
    perm = np.random.default_rng(2024).permutation(len(pts))
    # (a permuted list pairs the points with other streams: the same work statistically, its own step count, reported below)
    shuffled = np.ascontiguousarray(pts[perm])
    it.solve()
    frame, steps = it.solution.copy(), it.last_stats["walk_steps"]
    assert steps == CONFIG2_STEPS, steps
    field = it.solve_points(pts, 0, w)
    assert it.last_stats["walk_steps"] == CONFIG2_STEPS, it.last_stats["walk_steps"]
    assert np.array_equal(field, frame)

    def launches():
        return [{"kind": l["kind_name"], "walkers": l["walkers"], "beside": l["walkers_beside"], "ms": round(l["ms"], 3), "steps": l.get("steps")}
                for l in it.last_launches()]
    out = measure({"solve": it.solve, "points_row_major": lambda: it.solve_points(pts, 0, w),
                   "points_permuted": lambda: it.solve_points(shuffled, 0, w)}, repeats, launches)
    out["points_permuted"]["walk_steps"] = it.last_stats["walk_steps"]
    out["walk_steps"] = steps
    it.close()
    return out


def run_3d(repeats):
    import bench
    from elaina_amd import UniformIntegratorSettings
    from elaina_amd.integrator3d import Problem3, UniformIntegrator3
    w = 512
    V, T = bench.icosphere(3, 1.0)
    col = np.repeat((V[:, 0] * V[:, 1] + V[:, 2]).astype(np.float32)[:, None], 6, axis=1)
    sd = {"d_verts": V, "d_tris": T, "d_colors": col, "n_verts": None, "n_tris": None, "n_colors": None,
          "probe": (0.6, (0.0, 0.0, 0.1), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)), "dirichlet_intensity": 1.0, "neumann_intensity": 1.0}
    it = UniformIntegrator3(Problem3.from_dict(sd), UniformIntegratorSettings((w, w), 64, 64, 2e-3))
    pts = grid_points3(sd["probe"], w, w)
    tiles = tile_order(w, w)
    perm = np.random.default_rng(2024).permutation(len(pts))
    it.solve()
    frame, steps = it.solution.copy(), it.last_stats["walk_steps"]
    field = it.solve_points(pts, 0, w)
    assert it.last_stats["walk_steps"] == steps and np.array_equal(field, frame)
    by_tiles, shuffled = np.ascontiguousarray(pts[tiles]), np.ascontiguousarray(pts[perm])
    out = measure({"solve": it.solve, "points_row_major": lambda: it.solve_points(pts, 0, w),
                   "points_tile_order": lambda: it.solve_points(by_tiles, 0, w),
                   "points_permuted": lambda: it.solve_points(shuffled, 0, w)}, repeats)
    out["walk_steps"] = steps
    it.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["2d", "3d"], default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    out = {"repeats": args.repeats}
    if args.only != "3d":
        out["config2"] = run_2d(args.repeats)
    if args.only != "2d":
        out["icosphere_512"] = run_3d(args.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
