"""The wave-uniform fetches of the flat Neumann paths (wost_device.h: uniform_load): the silhouette vertices and their
normals, the segment records of the ray, sampling and closest-point loops come in through scalar loads issued together, not
through per-lane loads of one address.  Only the instruction that brings the operands changed: the arithmetic, the order of
the tests and the order of the draws are what they were, so every case below must give the oracle's field and its five
counters bit for bit -- the four-vertex box of the shipped scenes in every kind of launch, the square-root / division branch
of its silhouette test, the general loops (an open polyline of 5 and of WOST_FLAT_MAX = 64 segments), emissive sides, no
Neumann mesh at all (no read through a null table), and the guided kernels, which compile the same inline functions.

The half-precision guided solve has no oracle: its fixture, tests/golden/flat_neumann_guided_half.npz, is what the library
of the commit before this change wrote (python tests/test_gpu_flat_neumann_loads.py FILE writes it with the running library).
"""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import box_problem

pytestmark = pytest.mark.gpu

COUNTERS = ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits")
GOLDEN_HALF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flat_neumann_guided_half.npz")


def _ids(o):
    return "-".join("%s%d" % (k[:5], v) for k, v in o.items()) or "defaults"


def _same_solve(oracle, problem, key, w, h, spp, depth, eps, **opts):
    from test_gpu_parity import _assert_same_solve, _cached_ref
    ref = _cached_ref(oracle, problem, key, w, h, spp, depth, eps)
    _assert_same_solve(oracle, problem, w, h, spp, depth, eps, ref=ref, **opts)
    return ref


# ---- the ladybug frame (a four-vertex Neumann box): every kind of launch -----------------------------------------------------
@pytest.mark.parametrize("opts", [
    {"persist": 1, "resident_blocks": 2}, {"persist": 1, "resident_blocks": 6},
    {"persist": 1, "resident_blocks": 2, "block_size": 64}, {"persist": 1, "resident_blocks": 6, "block_size": 64},
    {"steps_per_round": 1}, {"steps_per_round": 7}, {"steps_per_round": 256},
    {"quad": 1},
    # long_steps small enough that the launch of the long remainders runs beside the rounds
    {"persist": 1, "resident_blocks": 2, "long_steps": 16},
], ids=_ids)
def test_ladybug_in_every_kind_of_launch(oracle, ladybug, opts):
    _same_solve(oracle, ladybug, "persist-ladybug", 96, 80, 24, 64, 1.0, **opts)


# ---- a Neumann box seen from outside: its corners are silhouettes within R_D --------------------------------------------------
OBSTACLE = dict(w=56, h=44, spp=6, depth=24, eps=1e-3, lo=0.4, hi=0.6)


def _obstacle_problem():
    """the unit square with Dirichlet sides and a four-vertex Neumann box [0.4, 0.6]^2 inside it: seen from outside the small
    box a corner is a silhouette vertex, and nearly every evaluation point is closer to one than to the Dirichlet sides"""
    from elaina_amd import Problem
    d = box_problem(value=lambda x, y: 1.0 + x - 0.5 * y)
    lo, hi = OBSTACLE["lo"], OBSTACLE["hi"]
    nv = np.asarray([(lo, lo), (hi, lo), (hi, hi), (lo, hi)], np.float32)
    ns = np.asarray([(0, 1), (1, 2), (2, 3), (3, 0)], np.int32)
    return Problem(d_verts=d.d_verts, d_segs=d.d_segs, d_colors=d.d_colors, n_verts=nv, n_segs=ns, n_colors=None, probe=d.probe)


def _fraction_with_a_corner_within_R_D():
    """share of the frame's evaluation points (probe: scale 0.45 around (0.5, 0.5), up = +y) that lie outside the small box and
    closer to one of its corners than to the unit square's sides: there the vertex test goes on to the square root"""
    s = OBSTACLE
    px = 0.45 * (2.0 * np.arange(s["w"]) / s["w"] - 1.0) + 0.5
    py = 0.45 * (2.0 * np.arange(s["h"]) / s["h"] - 1.0) + 0.5
    x, y = np.meshgrid(px, py)
    r_d = np.minimum(np.minimum(x, 1.0 - x), np.minimum(y, 1.0 - y))
    corner = np.min([np.hypot(x - cx, y - cy) for cx in (s["lo"], s["hi"]) for cy in (s["lo"], s["hi"])], axis=0)
    outside = (np.maximum(abs(x - 0.5), abs(y - 0.5)) > 0.5 * (s["hi"] - s["lo"]))
    return float(np.mean(outside & (corner < r_d)))


@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 2}, {"quad": 1}, {"steps_per_round": 3, "block_size": 64}], ids=_ids)
def test_box_corners_within_R_D(oracle, opts):
    share = _fraction_with_a_corner_within_R_D()
    print("evaluation points with a silhouette corner within R_D: %.1f %%" % (100.0 * share))
    assert share > 0.2
    s = OBSTACLE
    ref = _same_solve(oracle, _obstacle_problem(), "flat-loads-obstacle", s["w"], s["h"], s["spp"], s["depth"], s["eps"], **opts)
    assert ref["neumann_hits"] > 0


# ---- an open Neumann polyline: the general flat loops, vertices with one segment, the WOST_FLAT_MAX edge ---------------------
def _polyline_problem(n_segs, emissive):
    """the unit square with Dirichlet sides and an open zigzag of n_segs Neumann segments across it; its two end vertices
    have prev < 0 or next < 0"""
    from elaina_amd import Problem
    d = box_problem(value=lambda x, y: x + 2.0 * y)
    t = np.arange(n_segs + 1, dtype=np.float64) / n_segs
    nv = np.stack([0.2 + 0.6 * t, 0.5 + 0.12 * np.where(np.arange(n_segs + 1) % 2 == 0, -1.0, 1.0) + 0.1 * (t - 0.5)], 1).astype(np.float32)
    ns = np.stack([np.arange(n_segs), np.arange(n_segs) + 1], 1).astype(np.int32)
    nc = None
    if emissive:
        v = (0.2 * np.cos(5.0 * t)).astype(np.float32)
        nc = np.stack([v, 0.5 * v, -v, 0.3 * v, v, 0.25 * v], 1).astype(np.float32)
    return Problem(d_verts=d.d_verts, d_segs=d.d_segs, d_colors=d.d_colors, n_verts=nv, n_segs=ns, n_colors=nc, probe=d.probe)


@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 2}, {"quad": 1}], ids=_ids)
@pytest.mark.parametrize("emissive", [0, 1])
@pytest.mark.parametrize("n_segs", [5, 64])
def test_open_polyline(oracle, n_segs, emissive, opts):
    ref = _same_solve(oracle, _polyline_problem(n_segs, bool(emissive)), "flat-loads-polyline-%d-%d" % (n_segs, emissive),
                      48, 40, 6, 24, 1e-3, **opts)
    assert ref["neumann_hits"] > 0


# ---- flat emissive Neumann sides under a mask: sample_in_sphere_flat ----------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 2}, {"quad": 1, "steps_per_round": 3}], ids=_ids)
def test_masked_emissive_sides(oracle, opts):
    from test_gpu_chained_start import _emissive_box
    p = _emissive_box()
    ref = _same_solve(oracle, p, "dry-masked-box", 70, 50, 12, 32, 1e-3, **opts)
    assert ref["neumann_hits"] > 0
    assert np.all(ref["field"][p.mask == 0] == 0)


# ---- no Neumann mesh at all: nothing is read through its null tables -----------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 2}, {"quad": 1}], ids=_ids)
def test_no_neumann_mesh(oracle, opts):
    p = box_problem(value=lambda x, y: 0.5 + x * y)
    assert p.n_segs is None or len(p.n_segs) == 0
    ref = _same_solve(oracle, p, "flat-loads-dirichlet-only", 48, 40, 8, 32, 1e-3, **opts)
    assert ref["neumann_hits"] == 0


# ---- the guided kernels compile the same inline functions --------------------------------------------------------------------
GUIDED = dict(w=32, h=32, spp=4, depth=32, train_spp=2, seed=7)
GUIDED_STATS = COUNTERS + ("guided_steps", "train_samples", "optimizer_steps")


def _guided_half_solve():
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    from test_guided_integrator import AABB, EPS, laplace_box
    g = GUIDED
    st = GuidedIntegratorSettings(frameSize=(g["w"], g["h"]), samplesPerPixel=g["spp"], trainSppCount=g["train_spp"],
                                  maxWalkingDepth=g["depth"], epsilonShell=EPS, batchSize=2048, minBatchSize=512)
    gi = GuidedIntegrator(laplace_box(), st, AABB, seed=g["seed"])
    gi.network.set_option("precision", 16)
    gi.network.set_option("train_precision", 16)
    gi.solve()
    # the 74 848 trained weights by their digest: the fixture stays small
    out = {"field": gi.solution.copy(), "params_sha256": np.frombuffer(hashlib.sha256(gi.network.params().tobytes()).digest(), np.uint8)}
    out.update({k: np.int64(gi.last_stats[k]) for k in GUIDED_STATS})
    gi.close()
    return out


def test_guided_solve_fp32_matches_oracle(oracle):
    from test_guided_integrator import _gpu_and_oracle, laplace_box
    g = GUIDED
    gi, ref = _gpu_and_oracle(oracle, laplace_box(), g["w"], g["h"], g["spp"], g["depth"], g["train_spp"], seed=g["seed"], dump=False)
    assert gi.last_stats["optimizer_steps"] == ref["optimizer_steps"] > 0
    for k in COUNTERS + ("guided_steps", "train_samples"):
        assert gi.last_stats[k] == ref[k], k
    assert ref["neumann_hits"] > 0
    assert np.array_equal(gi.solution, ref["field"]), float(np.abs(gi.solution - ref["field"]).max())
    assert np.array_equal(gi.network.params(), ref["params"])
    gi.close()


def test_guided_solve_half_precision_matches_the_parent(oracle):
    want = np.load(GOLDEN_HALF)
    got = _guided_half_solve()
    assert int(want["optimizer_steps"]) > 0 and int(want["neumann_hits"]) > 0
    for k in GUIDED_STATS:
        assert int(got[k]) == int(want[k]), k
    assert np.array_equal(got["field"], want["field"]), float(np.abs(got["field"] - want["field"]).max())
    assert np.array_equal(got["params_sha256"], want["params_sha256"])


if __name__ == "__main__":
    # writes the half-precision fixture with the running library, after checking that a second solve repeats the first
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a, b = _guided_half_solve(), _guided_half_solve()
    assert all(np.array_equal(a[k], b[k]) for k in a), "the half-precision solve does not repeat itself"
    np.savez(sys.argv[1], **a)
    print({k: int(a[k]) for k in GUIDED_STATS})
