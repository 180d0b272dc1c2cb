"""The root visit at query start (wost_set_option "root_visit"): a lane of the round kernels that begins a closest-point query
visits the root of the Dirichlet tree in the same step trip, the root's six rows read on the scalar path (wost_device.h:
trav_visit_root), not as the first gather of its first traversal burst.  Only where and how the root's record is fetched
changed: the distances, the keys, the pushes and the traversal state after the visit are what a first trav_visit leaves, so
both rules must give the oracle's field and its five counters bit for bit in every kind of launch, and count the same node
visits.  The small meshes are where a root form can go wrong: a root whose children are leaves, padding children, a query
that is complete at the root, a tie on the first descent, and the walkers beyond far2 / huge2 that must not take it."""
import numpy as np
import pytest

from conftest import box_problem, wiggly_problem
from test_gpu_parity import _cached_ref, _integrator, _with_source

pytestmark = pytest.mark.gpu

ROOT = [0, 1]
COUNTERS = ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits")


def _ids(o):
    return "-".join("%s%d" % (k[:5], v) for k, v in o.items()) or "defaults"


def _both_rules(oracle, problem, key, w, h, spp, depth, eps, same_visits=True, **opts):
    """the solve under root_visit 0 and 1: each the oracle's bits, and the same node visits; returns (ref, stats by rule).
    same_visits=False where the node visits of a solve are no function of the solve under EITHER rule -- see
    test_ladybug_in_every_kind_of_launch."""
    ref = _cached_ref(oracle, problem, key, w, h, spp, depth, eps)
    got = {}
    for rule in ROOT:
        it = _integrator(problem, w, h, spp, depth, eps)
        it.set_option("root_visit", rule)
        for k, v in opts.items():
            it.set_option(k, v)
        it.solve()
        s = got[rule] = dict(it.last_stats)
        for c in COUNTERS:
            assert s[c] == ref[c], (rule, c)
        assert np.array_equal(it.solution, ref["field"]), (rule, float(np.abs(it.solution - ref["field"]).max()))
        it.close()
    print({r: {k: got[r][k] for k in ("inner_visits", "trav_trips", "step_trips")} for r in ROOT})
    if same_visits:
        assert got[0]["inner_visits"] == got[1]["inner_visits"]
    return ref, got


# ---- the ladybug frame: persistent launch, rounds, quads, the long remainders ---------------------------------------------------
@pytest.mark.parametrize("opts", [
    {"persist": 1, "resident_blocks": 2}, {"persist": 1, "resident_blocks": 6},
    {"persist": 1, "resident_blocks": 2, "block_size": 64}, {"persist": 1, "resident_blocks": 6, "block_size": 64},
    {"steps_per_round": 1}, {"steps_per_round": 7}, {"steps_per_round": 256},
    {"quad": 1},
    # long_steps small enough that the launch of the long remainders runs beside the rounds
    {"persist": 1, "resident_blocks": 2, "long_steps": 16},
], ids=_ids)
def test_ladybug_in_every_kind_of_launch(oracle, ladybug, opts):
    """With long_steps the node visits are compared with nothing: the launch of the long remainders is the SLACK quad kernel,
    whose visits prune with the relative slack and so open a box more now and then, and WHICH pixels it takes is decided by
    the moment each wave of the persistent launch stops.  Six solves of this case under one rule counted 13 065 948 .. 13 065 959
    visits with root_visit 0 and 13 065 945 .. 13 065 950 with 1 (the same 1 334 577 walk steps every time); without long_steps
    all twelve counted 13 065 904.  Field and counters are compared in every case."""
    _both_rules(oracle, ladybug, "persist-ladybug", 96, 80, 24, 64, 1.0, same_visits="long_steps" not in opts, **opts)


def test_fille(oracle, fille):
    _both_rules(oracle, fille, "persist-fille", 96, 80, 9, 128, 1.0, same_visits=False, persist=1, resident_blocks=8, long_steps=16)
    _both_rules(oracle, fille, "persist-fille", 96, 80, 9, 128, 1.0, persist=1, resident_blocks=8)


# ---- tiny Dirichlet meshes: one leaf, the largest tree of one level, the smallest of two, the sizes around the next edge -----------
def _arc(n_segs):
    """an open Dirichlet polyline of n_segs segments on 300 degrees of a wobbling circle"""
    from elaina_amd import Problem
    t = np.linspace(0.0, 300.0 / 180.0 * np.pi, n_segs + 1)
    r = 1.0 + 0.15 * np.sin(5.0 * t)
    verts = np.stack([r * np.cos(t), r * np.sin(t)], 1).astype(np.float32)
    segs = np.stack([np.arange(n_segs), np.arange(n_segs) + 1], 1).astype(np.int32)
    cols = np.random.default_rng(n_segs).uniform(0.0, 1.0, size=(n_segs + 1, 6)).astype(np.float32)
    return Problem(d_verts=verts, d_segs=segs, d_colors=cols, probe=(1.3, 0.0, 0.0, 0.0, 1.0))


@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 1}], ids=_ids)
@pytest.mark.parametrize("n_segs", [1, 4, 5, 16, 17, 64, 65])
def test_tiny_meshes(oracle, n_segs, opts):
    ref, _ = _both_rules(oracle, _arc(n_segs), "root-arc-%d" % n_segs, 32, 32, 6, 16, 1e-2, **opts)
    assert ref["walk_steps"] > ref["walks_started"] > 0       # queries beyond the cached depth-0 one were made


# ---- two exactly coincident segments: a tie on the first descent -------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 1}, {"quad": 1}], ids=_ids)
def test_coincident_segments(oracle, opts):
    from elaina_amd import Problem
    a = _arc(12)
    # segment 3 once more at the end, and segment 7 once more with its ends swapped: the lowest original index wins
    segs = np.concatenate([a.d_segs, a.d_segs[3:4], a.d_segs[7:8, ::-1]]).astype(np.int32)
    p = Problem(d_verts=a.d_verts, d_segs=segs, d_colors=a.d_colors, probe=(1.3, 0.0, 0.0, 0.0, 1.0))
    _both_rules(oracle, p, "root-coincident", 32, 32, 6, 16, 1e-2, **opts)


# ---- a frame far around a small mesh: the slack launch takes its root form, the lanes beyond huge2 skip it ---------------------------
@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 2}, {"quad": 1}], ids=_ids)
def test_frame_beyond_far2_and_huge2(oracle, opts):
    """far2 = (1.5 extents)^2 and huge2 = (64 extents)^2 of the mesh: the frame spans 150 extents, so its walks begin beyond
    either and come back through both ranges"""
    from elaina_amd import Problem
    a = _arc(40)
    ext = float(np.abs(a.d_verts).max())
    p = Problem(d_verts=a.d_verts, d_segs=a.d_segs, d_colors=a.d_colors, probe=(150.0 * ext, 0.0, 0.0, 0.0, 1.0))
    px = 150.0 * ext * (2.0 * np.arange(32) / 32.0 - 1.0)
    d, rmax = np.hypot(*np.meshgrid(px, px)), float(np.hypot(a.d_verts[:, 0], a.d_verts[:, 1]).max())
    # pixels surely beyond huge2 (86 %), and surely between far2 and huge2 (14 %); the one at the origin is within far2
    assert np.mean(d - rmax > 64.0 * ext) > 0.3 and np.mean((d - rmax > 1.5 * ext) & (d + rmax < 64.0 * ext)) > 0.05
    ref, _ = _both_rules(oracle, p, "root-afar", 32, 32, 6, 16, 1e-2, **opts)
    assert ref["walk_steps"] > ref["walks_started"]


# ---- the other step bodies ------------------------------------------------------------------------------------------------------------
def test_masked_emissive_flat_neumann_box(oracle):
    from test_gpu_chained_start import _emissive_box
    p = _emissive_box()
    ref, _ = _both_rules(oracle, p, "dry-masked-box", 70, 50, 12, 32, 1e-3, persist=1, resident_blocks=2)
    assert ref["neumann_hits"] > 0
    assert np.all(ref["field"][p.mask == 0] == 0)


def test_tree_borne_neumann_mesh(oracle):
    p = wiggly_problem(emissive=True)
    _both_rules(oracle, p, "chain-wiggly", 40, 40, 2, 24, 0.05)


def test_source_term(oracle):
    mixed = _with_source(box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: y, flux=lambda x, y, s: 0.2), 0.0, 1.0)
    _both_rules(oracle, mixed, "dry-source-box", 48, 40, 14, 32, 1e-3, persist=1, resident_blocks=2)


@pytest.mark.parametrize("rule", ROOT)
def test_continued_solve_in_three_cuts(oracle, fille, rule):
    """the carry bodies: 3 + 5 + 1 samples are the 9 of one solve"""
    ref = _cached_ref(oracle, fille, "persist-fille", 96, 80, 9, 128, 1.0)
    it = _integrator(fille, 96, 80, 4, 128, 1.0)
    it.set_option("root_visit", rule)
    sums = dict.fromkeys(COUNTERS, 0)
    for more in (3, 5, 1):
        it.solve_more(more)
        for c in COUNTERS:
            sums[c] += it.last_stats[c]
    assert it.spp_done == 9
    for c in COUNTERS:
        assert sums[c] == ref[c], c
    assert np.array_equal(it.solution, ref["field"]), float(np.abs(it.solution - ref["field"]).max())
    it.close()


# ---- the rule acts ---------------------------------------------------------------------------------------------------------------------
def test_the_rule_acts(ladybug):
    """the same walk steps and node visits in fewer traversal trips: the root visits left the bursts"""
    it = _integrator(ladybug, 96, 80, 24, 64, 1.0)
    it.set_option("persist", 1)
    it.set_option("resident_blocks", 6)
    got = {}
    for rule in ROOT:
        it.set_option("root_visit", rule)
        it.solve()
        got[rule] = dict(it.last_stats)
        print("root_visit", rule, {k: got[rule][k] for k in ("walk_steps", "inner_visits", "step_trips", "trav_trips")})
    it.close()
    assert got[1]["walk_steps"] == got[0]["walk_steps"] > 0
    assert got[1]["inner_visits"] == got[0]["inner_visits"] > 0
    assert got[1]["trav_trips"] < got[0]["trav_trips"]


def test_option_takes_zero_and_one_only(ladybug):
    it = _integrator(ladybug, 8, 8, 1, 4, 1.0)
    for bad in (-1, 2, 0.5):
        with pytest.raises(Exception):
            it.set_option("root_visit", bad)
    it.set_option("root_visit", 0)
    it.set_option("root_visit", 1)
    it.close()
