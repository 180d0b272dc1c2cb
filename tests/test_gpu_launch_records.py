"""What wost_last_launches says about a uniform solve with a persistent first launch: the records add up.

The field of such a solve does not depend on how run_solve schedules it, so the parity tests (test_gpu_parity.py:
test_persistent_first_launch_matches_oracle, the same option rows) cannot see a hand-over that sends the wrong number of walkers
beside the rounds, a pass that is recorded but not counted, or a record of a launch that never ran.  These tests read the
records of the same small solves -- 96 x 80, 7 680 walkers -- and check them against wost_stats and against what a persistent
launch can hand over at all.  No timing is asserted: `ms` is only finite and not negative.

Strayed walkers.  A walker whose query leaves the plain visits' range is parked and restarted on a side stream with the next
pass; it is counted in that pass's walkers_beside.  With long_steps = 0 nothing else is: the sum of walkers_beside over such a
solve is the number S of those events.  A walk is the same walk under every schedule and only the plain kernels park walkers (the
launch of the long remainders is exact at any distance), so no other schedule of the same solve has more than S of them: S is
the allowance for strayed walkers wherever a bound below speaks of them."""
import math

import numpy as np
import pytest

from test_gpu_parity import _integrator

pytestmark = pytest.mark.gpu

W, H = 96, 80
N_WALKERS = W * H
BLOCK_SIZE = 256        # the handle's default
LONG_CAP = 32768        # the handle's default
MAX_STRAYED_BESIDE = 1024

ROWS = [
    # the rows of test_persistent_first_launch_matches_oracle that name long_steps, long_cap, tail_sort or long_thin
    ("ladybug", 24, 64, {"resident_blocks": 6, "long_steps": 8}),
    ("ladybug", 24, 64, {"resident_blocks": 6, "long_steps": 64, "long_cap": 37}),
    ("ladybug", 24, 64, {"resident_blocks": 6, "long_steps": 0, "tail_sort": 0}),
    ("ladybug", 24, 64, {"resident_blocks": 6, "long_steps": 48, "tail_sort": 0}),
    ("fille", 9, 128, {"resident_blocks": 8, "long_steps": 40, "steps_per_round": 8}),
    ("fille", 9, 128, {"resident_blocks": 8, "long_steps": 16, "long_thin": 5}),
    ("ladybug", 24, 64, {"resident_blocks": 6, "long_steps": 8, "long_thin": 0}),
    # the default hand-over; every handed-over pixel beside the rounds, one at a time; as many resident lanes as walkers: the
    # queue is dry at once
    ("ladybug", 24, 64, {"resident_blocks": 6}),
    ("ladybug", 24, 64, {"resident_blocks": 6, "long_steps": 8, "long_cap": 1}),
    ("ladybug", 24, 64, {"resident_blocks": 30, "long_steps": 8}),
]

_SCENES, _STRAY_EVENTS = {}, {}


def _scene(name):
    if name not in _SCENES:
        from elaina_amd import Problem
        _SCENES[name] = Problem.load_scene(name)
    return _SCENES[name]


def _stray_events(name, spp, depth):
    """S of the module's docstring for the frame solve of a scene, measured once"""
    key = (name, spp, depth)
    if key not in _STRAY_EVENTS:
        it = _integrator(_scene(name), W, H, spp, depth, 1.0)
        for k, v in {"persist": 1, "resident_blocks": 6, "long_steps": 0}.items():
            it.set_option(k, v)
        it.solve()
        _STRAY_EVENTS[key] = sum(l["walkers_beside"] for l in it.last_launches())
        it.close()
    return _STRAY_EVENTS[key]


def _points(problem):
    """7 680 evaluation points spread over the box of the scene's Dirichlet boundary"""
    rng = np.random.default_rng(96 * 80)
    lo, hi = problem.d_verts.min(axis=0), problem.d_verts.max(axis=0)
    return (lo + (hi - lo) * rng.uniform(0.02, 0.98, size=(N_WALKERS, 2))).astype(np.float32)


def _check_records(ll, stats, opts, strayed, what):
    from elaina_amd import capi
    kinds_of_a_launch = (capi.LAUNCH_ROUND, capi.LAUNCH_QUAD, capi.LAUNCH_ONE, capi.LAUNCH_PERSISTENT)
    block_size = opts.get("block_size", BLOCK_SIZE)
    assert ll, what
    real = [l for l in ll if l["kind"] != capi.LAUNCH_WAIT]
    waits = [i for i, l in enumerate(ll) if l["kind"] == capi.LAUNCH_WAIT]
    # -- every solve
    assert len(real) == stats["kernel_launches"], (what, [l["kind_name"] for l in ll], stats["kernel_launches"])
    for i, l in enumerate(ll):
        assert l["kind"] in kinds_of_a_launch + (capi.LAUNCH_WAIT, capi.LAUNCH_BESIDE), (what, i, l)
        assert math.isfinite(l["ms"]) and l["ms"] >= 0.0, (what, i, l)
        if l["kind"] in kinds_of_a_launch:
            assert l["walkers"] > 0 and l["grid"] > 0, (what, i, l)
        elif l["kind"] == capi.LAUNCH_BESIDE:
            assert l["walkers"] == 0 and l["grid"] == 0 and l["walkers_beside"] > 0, (what, i, l)
    first = ll[0]
    assert first["kind"] == capi.LAUNCH_PERSISTENT, (what, first)
    assert first["walkers"] == N_WALKERS, (what, first)
    assert first["grid"] == min(-(-N_WALKERS // block_size), opts["resident_blocks"]), (what, first)
    assert all(l["kind"] != capi.LAUNCH_PERSISTENT for l in ll[1:]), what
    done = [l["walk_steps_done"] for l in real]
    assert all(a <= b for a, b in zip(done, done[1:])), (what, done)
    assert done[-1] <= stats["walk_steps"], (what, done, stats["walk_steps"])
    assert len(waits) <= 1 and (not waits or waits[0] == len(ll) - 1), (what, waits)
    if not waits:
        assert ll[-1]["walk_steps_done"] == stats["walk_steps"], (what, done, stats["walk_steps"])
    # -- what the persistent launch handed over: one pixel per lane is all it can
    assert len(real) >= 2, (what, "a persistent launch on fewer lanes than walkers hands its last pixels over")
    second = real[1]
    assert second["walkers"] + second["walkers_beside"] <= first["grid"] * block_size, (what, first, second)
    long_steps = opts.get("long_steps", 1024)
    if long_steps == 0:
        assert not waits, what
        assert sum(l["walkers_beside"] for l in real) <= strayed, (what, real, strayed)
    else:
        cap = opts.get("long_cap", LONG_CAP)
        assert second["walkers_beside"] <= cap + strayed, (what, second, cap, strayed)
        if strayed <= min(MAX_STRAYED_BESIDE, cap):
            # (so few strayed walkers join the long remainders, inside the cap)
            assert second["walkers_beside"] <= cap, (what, second, cap)
    # a wait is for the launch of the long remainders: none without one
    if waits:
        assert long_steps > 0 and second["walkers_beside"] > 0, (what, ll)


@pytest.mark.parametrize("scene,spp,depth,opts", ROWS, ids=lambda v: "-".join("%s%d" % (k[:6], x) for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_launch_records_add_up(scene, spp, depth, opts):
    """the frame solve, a continued solve of as many samples again on the same handle (it starts a list of its own) and a
    point solve of as many points as the frame has pixels"""
    problem = _scene(scene)
    strayed = _stray_events(scene, spp, depth)
    it = _integrator(problem, W, H, spp, depth, 1.0)
    it.set_option("persist", 1)
    for k, v in opts.items():
        it.set_option(k, v)
    it.solve()
    frame = it.last_launches()
    _check_records(frame, it.last_stats, opts, strayed, "solve")
    it.solve_more(spp)
    assert it.spp_done == spp
    _check_records(it.last_launches(), it.last_stats, opts, strayed, "solve_more")
    # (the points are not the frame's: their stray events are their own, and the bounds that need them are checked on the frame)
    pts = _points(problem)
    field = it.solve_points(pts)
    assert field.shape == (N_WALKERS, 3) and np.isfinite(field).all()
    ll = it.last_launches()
    _check_records(ll, it.last_stats, opts, sum(l["walkers_beside"] for l in ll), "solve_points")
    it.close()


def test_the_order_of_the_first_round_does_not_change_the_records_structure():
    """tail_sort 0 and 1: the same walkers go beside the rounds and to the first round, only their order differs -- the
    persistent launch ends when the queue is dry, which no option of the hand-over moves"""
    lists = []
    for tail_sort in (0, 1):
        it = _integrator(_scene("ladybug"), W, H, 24, 64, 1.0)
        for k, v in {"persist": 1, "resident_blocks": 6, "long_steps": 0, "tail_sort": tail_sort}.items():
            it.set_option(k, v)
        it.solve()
        lists.append((it.last_launches(), dict(it.last_stats)))
        it.close()
    (a, sa), (b, sb) = lists
    assert sa["walk_steps"] == sb["walk_steps"]
    assert a[0]["kind"] == b[0]["kind"] and a[0]["walkers"] == b[0]["walkers"] and a[0]["grid"] == b[0]["grid"]
    assert a[-1]["walk_steps_done"] == b[-1]["walk_steps_done"] == sa["walk_steps"]
