#!/usr/bin/env python3
"""What the index of an exit list costs and what the ordered adjoints cost beside the atomic ones (EXPERIMENTS "The index of an
exit list").  One process, one JSON line on stdout.

  ladybug, n = 1024^2 points on the pixel grid of the scene's probe, depth 64, S in {8, 64}, K in {1, 4}:
    - the walk of the list (host clock around the call, and the launches' device time) and the build of its index, --builds
      times in a row (both allocate arrays of the size of the list, so the first of a process is the cold one)
    - exits_adjoint_dev against exits_adjoint_ordered_dev, exits_adjoint_gradient_dev against exits_adjoint_gradient_ordered_dev
    - the incidences, the longest bin and the mean length of the bins that hold any

Every shape is warmed up, the two forms alternate inside each repeat (--repeats, at least 5), times are the host clock around
calls that are complete on return; per variant the median and the extremes are reported.  Before anything is timed the ordered
result is checked against the atomic one (the largest difference over the largest entry) and against a second ordered call (bit
for bit).

    python tools/gpu_exits_index_bench.py [--repeats 5] [--frame 1024] [--walks 8 64] [--sets 1 4]
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

from tools.gpu_points_bench import grid_points2, measure, timed      # noqa: E402


def run(frame, walks, sets, repeats, builds=3):
    import torch
    from elaina_amd import Problem, UniformIntegrator, UniformIntegratorSettings, capi
    p = Problem.load_scene("ladybug")
    it = UniformIntegrator(p, UniformIntegratorSettings((frame, frame), 1, 64, p.default_eps))
    n_verts = len(p.d_verts)
    pts = grid_points2(p.probe, frame, frame)
    n = len(pts)
    d_pts = torch.from_numpy(pts).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(5)
    out = {"n": n, "n_verts": n_verts, "bins": 2 * n_verts}
    for S in walks:
        for gradient in (False, True):
            key = "S%d_%s" % (S, "gradient" if gradient else "field")
            r = out[key] = {}
            torch.cuda.synchronize()
            try:
                if gradient:
                    r["walk_ms"] = timed(lambda: it.exits_walk_gradient_dev(d_pts.data_ptr(), n, S, stream, 0, n, frame))
                else:
                    r["walk_ms"] = timed(lambda: it.exits_walk_dev(d_pts.data_ptr(), n, S, stream, 0, frame))
            except capi.WostError as e:
                r["refused"] = str(e)
                continue
            r["walk_kernel_ms"] = it.last_stats["kernel_ms"]
            r["index_ms"] = timed(it.exits_index)
            r["index_again_ms"] = timed(it.exits_index)
            # the walk and the build allocate (and the build frees) arrays of the size of the list: both once more, `builds` times
            walk = (lambda: it.exits_walk_gradient_dev(d_pts.data_ptr(), n, S, stream, 0, n, frame)) if gradient else \
                   (lambda: it.exits_walk_dev(d_pts.data_ptr(), n, S, stream, 0, frame))
            r["walk_all_ms"], r["index_all_ms"] = [round(r["walk_ms"], 3)], [round(r["index_ms"], 3)]
            for _ in range(builds - 1):
                r["walk_all_ms"].append(round(timed(walk), 3))
                r["index_all_ms"].append(round(timed(it.exits_index), 3))
            n_inc, longest = it.exits_index_info
            begin = it.exits_index_records()["bin_begin"]
            lengths = np.diff(begin)
            r.update(n_incidences=n_inc, longest_bin=longest, bins_in_use=int((lengths > 0).sum()),
                     mean_bin_in_use=float(lengths[lengths > 0].mean()) if n_inc else 0.0,
                     median_bin_in_use=float(np.median(lengths[lengths > 0])) if n_inc else 0.0)
            plain, ordered = ("exits_adjoint_gradient_dev", "exits_adjoint_gradient_ordered_dev") if gradient else \
                             ("exits_adjoint_dev", "exits_adjoint_ordered_dev")
            for K in sets:
                shape = (K, n, 2, 3) if gradient else (K, n, 3)
                d_in = torch.from_numpy(rng.normal(size=shape).astype(np.float32)).cuda()
                a, b, c = (torch.full((K, n_verts, 6), -1.0, dtype=torch.float32, device="cuda") for _ in range(3))
                torch.cuda.synchronize()
                getattr(it, plain)(d_in.data_ptr(), K, a.data_ptr(), stream)
                getattr(it, ordered)(d_in.data_ptr(), K, b.data_ptr(), stream)
                getattr(it, ordered)(d_in.data_ptr(), K, c.data_ptr(), stream)
                m = measure({"atomic": lambda: getattr(it, plain)(d_in.data_ptr(), K, a.data_ptr(), stream),
                             "ordered": lambda: getattr(it, ordered)(d_in.data_ptr(), K, b.data_ptr(), stream)}, repeats)
                m["ordered_twice_same_bits"] = bool(torch.equal(b.view(torch.int32), c.view(torch.int32)))
                m["max_difference_over_max_entry"] = float((a - b).abs().max() / b.abs().max())
                m["max_entry"] = float(b.abs().max())
                m["entries_that_differ"] = int((a != b).sum())
                r["K%d" % K] = m
                print("%s K=%d: atomic %.3f ms, ordered %.3f ms" % (key, K, m["atomic"]["median_ms"], m["ordered"]["median_ms"]), file=sys.stderr, flush=True)
    it.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frame", type=int, default=1024)
    ap.add_argument("--walks", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--builds", type=int, default=3, help="walks and index builds per list (the first is the cold one)")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    print(json.dumps(run(args.frame, args.walks, args.sets, args.repeats, args.builds)))


if __name__ == "__main__":
    main()
