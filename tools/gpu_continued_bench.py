#!/usr/bin/env python3
"""What a continued solve (wost_solve_more) costs beside the single solve of the same samples, and what it saves the host's
metric frames.  One process, one JSON line on stdout.

  solve   ladybug 1024^2, depth 64: one solve() of 256 spp against four continued calls of 64 samples.  Before anything is
          timed the field of the four calls is checked against solve() bit for bit and the walk steps against its count.  The
          variants alternate inside each repeat; times are the host clock around the synchronising calls.
  host    elaina-exec on ladybug 1024^2, depth 64, 16 spp with saveSppMetricsDuration 1: sixteen frames.  --exec names further
          builds of the host program to run on the same configuration (a build that solves every frame from scratch does
          136 spp-units of work for them, one on continued solves 16).

    python tools/gpu_continued_bench.py [--repeats 5] [--only solve|host] [--exec PATH ...]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
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
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def bench_solve(repeats, frame=1024, spp=256, calls=4, depth=64):
    from elaina_amd import Problem, UniformIntegrator, UniformIntegratorSettings
    it = UniformIntegrator(Problem.load_scene("ladybug"), UniformIntegratorSettings((frame, frame), spp, depth, 1.0))
    per = spp // calls

    def continued():
        it.restart()
        steps, kinds = 0, []
        for _ in range(calls):
            it.solve_more(per)
            steps += it.last_stats["walk_steps"]
            kinds.append([l["kind_name"] for l in it.last_launches()])
        return steps, kinds

    it.solve()
    want, want_steps = it.solution.copy(), it.last_stats["walk_steps"]
    steps, kinds = continued()
    assert it.spp_done == per * calls == spp
    assert steps == want_steps and np.array_equal(it.solution, want), "continued calls differ from the single solve"
    single, split = [], []
    for _ in range(repeats):
        single.append(timed(it.solve))
        split.append(timed(continued))
    it.close()
    return {"frame": frame, "spp": spp, "calls": calls, "walk_steps": int(want_steps), "single_solve": summary(single),
            "continued_calls": summary(split), "launches_of_the_calls": kinds}


def bench_host(repeats, exes, frame=1024, spp=16, depth=64):
    sys.path.insert(0, os.path.join(_ROOT, "tools"))
    import export_scene
    out = {}
    with tempfile.TemporaryDirectory() as d:
        conf = export_scene.export("ladybug", d, frame=frame, spp=spp, depth=depth)
        c = json.load(open(conf))
        c["integrator"]["setting"].update({"saveSppMetricsDuration": 1, "saveSppMetricsUntil": spp})
        json.dump(c, open(conf, "w"))
        for exe in exes:
            ms = []
            for _ in range(repeats):
                r = subprocess.run([exe, conf], capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError("%s failed: %s" % (exe, r.stderr[-400:]))
                res = json.load(open(os.path.join(d, "exp", "ladybug_u", "result.json")))
                ms.append(float(res["duration"]))
            frames = len(os.listdir(os.path.join(d, "exp", "ladybug_u", "frames")))
            out[exe] = dict(summary(ms), frames_written=frames, unit="solve() milliseconds of result.json")
    return {"frame": frame, "spp": spp, "runs": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["solve", "host"], default=None)
    ap.add_argument("--exec", action="append", default=[], help="another build of elaina-exec to time on the same configuration")
    a = ap.parse_args()
    line = {}
    if a.only != "host":
        line["solve"] = bench_solve(a.repeats)
    if a.only != "solve":
        from elaina_amd import build
        line["host"] = bench_host(max(1, a.repeats // 2), [build.HOST_EXE] + a.exec)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
