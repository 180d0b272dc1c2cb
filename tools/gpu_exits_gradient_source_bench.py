#!/usr/bin/env python3
"""What the in-ball term costs an exit list of the gradient (EXPERIMENTS "Exit lists of the gradient: the in-ball term").  One
process, one JSON line on stdout.

  The unit square with Dirichlet data on two sides and Neumann data on the other two, once with a source grid over it and once
  without: the same geometry, so the same walks' lengths up to what the source adds to a record.  n = 256^2 points on a grid
  inside the square, a 256 x 256 frame (blocks of 1024 points at S = 64), depth 32, shell 1e-3, S = 64, K = 1.
    - the walk of each list: the host clock around the call and the launches' device time (kernel_ms), --walks times
    - wost_exits_apply_gradient_dev on the list with the term (the BALL kernel) against the list without (the other one)

The shapes are warmed up, the two lists alternate inside each repeat (--repeats, at least 5), times are the host clock around
calls that are complete on return; per variant the median and the extremes are reported.

    python tools/gpu_exits_gradient_source_bench.py [--repeats 5] [--grid 256] [--S 64] [--sets 1]
"""
import argparse
import json
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tools.gpu_points_bench import measure, timed      # noqa: E402


def _box(source):
    """the mixed box of tests/test_gpu_points.py, and with the source grid of tests/test_gpu_gradient_source.py"""
    from conftest import box_problem
    p = box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: 1.0 + x + 2.0 * y, flux=lambda x, y, s: 0.3 * (s - 2))
    if source:
        rng = np.random.default_rng(9)
        gx, gy = np.meshgrid(np.linspace(0, 1, 25), np.linspace(0, 1, 25))
        rgb = np.stack([np.sin(3 * gx + 2 * gy) + 0.3 * rng.normal(size=gx.shape), gx * gy, 1.0 - gy], -1).astype(np.float32)
        p.source = {"rgb": rgb, "index_scale": (24.0, 24.0), "index_offset": (0.0, 0.0), "intensity": 0.7}
    return p


def run(grid, S, K, repeats, walks):
    import torch
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    x = (np.arange(grid, dtype=np.float64) + 0.5) / grid
    pts = np.stack(np.meshgrid(x, x), -1).reshape(-1, 2).astype(np.float32)
    n = len(pts)
    d_pts = torch.from_numpy(pts).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    out = {"n": n, "S": S, "K": K, "frame": grid}
    its, bufs = {}, {}
    for name, source in (("with_term", True), ("without", False)):
        it = its[name] = UniformIntegrator(_box(source), UniformIntegratorSettings((grid, grid), 1, 32, 1e-3))
        it.set_option("exits_grad_source", 1)
        r = out[name] = {"walk_ms": [], "walk_kernel_ms": []}
        for _ in range(walks):
            torch.cuda.synchronize()
            r["walk_ms"].append(round(timed(lambda: it.exits_walk_gradient_dev(d_pts.data_ptr(), n, S, stream, 0, n, grid)), 3))
            r["walk_kernel_ms"].append(round(it.last_stats["kernel_ms"], 3))
        r["kernel_launches"] = it.last_stats["kernel_launches"]
        r["carries_the_term"] = getattr(it.lib, "wost_exits_gradient_terms")(it._handle, None, None, None) == 0
        n_verts = len(it.problem.d_verts)
        sets = torch.from_numpy(np.random.default_rng(5).uniform(-1.0, 2.0, size=(K, n_verts, 6)).astype(np.float32)).cuda()
        grad, se = (torch.zeros((K, n, 2, 3), dtype=torch.float32, device="cuda") for _ in range(2))
        field = torch.zeros((K, n, 3), dtype=torch.float32, device="cuda")
        bufs[name] = (sets, grad, se, field)
    torch.cuda.synchronize()

    def apply(name):
        sets, grad, se, field = bufs[name]
        return lambda: its[name].exits_apply_gradient_dev(sets.data_ptr(), K, grad.data_ptr(), stream, se.data_ptr(), field.data_ptr())

    out["apply"] = measure({name: apply(name) for name in its}, repeats)
    for name in its:
        out[name]["finite_grad_fraction"] = float(torch.isfinite(bufs[name][1]).float().mean())
        its[name].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--sets", type=int, default=1)
    ap.add_argument("--walks", type=int, default=3, help="walks per list (the first of a process is the cold one)")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    print(json.dumps(run(args.grid, args.S, args.sets, args.repeats, args.walks)))


if __name__ == "__main__":
    main()
