"""Uniform solves at the caller's evaluation points (wost_solve_points & co.) against the unchanged oracle, bit for bit.

The oracle has no point list, but a probe with scale 0 and position p makes its evaluation point p exactly (0 * finite + p),
so a solve of the single pixel k of a frame seed_width wide walks exactly point p on the random stream of pixel k: one such
oracle solve per point is the reference of a point solve with seed_base + i = k.  Fields are compared with np.array_equal,
the five counters as sums over the points."""
import ctypes as C

import numpy as np
import pytest

from conftest import box_problem, cube_scene3, sphere_scene3, wiggly_problem
from test_gpu_parity import _cached_ref, _integrator, _with_source

pytestmark = pytest.mark.gpu

COUNTERS = ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits")
_ORACLE_POINTS = {}


def _oracle_points(oracle, key, sd, pts, seed_base, seed_width, spp, depth, eps, dim=2):
    """one oracle solve per point, once per key: {"field": (n, 3), counter: per-point array}"""
    if key not in _ORACLE_POINTS:
        sd = dict(sd)
        n = len(pts)
        height = -(-(seed_base + n) // seed_width)
        out = {"field": np.zeros((n, 3), np.float32)}
        out.update({k: np.zeros(n, np.int64) for k in COUNTERS})
        for i, p in enumerate(pts):
            k = seed_base + i
            if dim == 2:
                sd["probe"] = (0.0, float(p[0]), float(p[1]), 0.0, 1.0)
                r = oracle.solve(sd, seed_width, height, spp, depth, eps, pixel_begin=k, pixel_end=k + 1, threads=1)
            else:
                sd["probe"] = (0.0, tuple(float(v) for v in p), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0))
                r = oracle.solve3(sd, seed_width, height, spp, depth, eps, pixel_begin=k, pixel_end=k + 1, threads=1)
            out["field"][i] = r["field"][0]
            for c in COUNTERS:
                out[c][i] = r[c]
        _ORACLE_POINTS[key] = out
    return _ORACLE_POINTS[key]


def _assert_points(field, stats, ref, rows=slice(None)):
    for c in COUNTERS:
        assert stats[c] == int(ref[c][rows].sum()), (c, stats[c], int(ref[c][rows].sum()))
    assert field.dtype == np.float32 and field.shape == ref["field"][rows].shape
    assert np.array_equal(field, ref["field"][rows]), float(np.abs(field - ref["field"][rows]).max())


def _grid_points(oracle, problem, w, h):
    """the evaluation points of the frame, row-major, from the oracle's own wo_eval_point"""
    sc = oracle.make_scene(problem.as_dict())
    pts = np.zeros((w * h, 2), np.float32)
    x, y = C.c_float(), C.c_float()
    for p in range(w * h):
        oracle.lib.wo_eval_point(C.byref(sc), p % w, p // w, w, h, C.byref(x), C.byref(y))
        pts[p] = x.value, y.value
    return pts


# ---- 1. the frame's own points ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ladybug_grid(oracle, ladybug):
    return _grid_points(oracle, ladybug, 96, 80)


@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 2}, {"block_size": 64}],
                         ids=lambda o: "-".join("%s%d" % (k[:5], v) for k, v in o.items()) or "defaults")
def test_the_frames_own_points_reproduce_the_frame_solve(oracle, ladybug, ladybug_grid, opts):
    """7 680 walkers: rounds by default, the persistent launch with its hand-over and quads on two blocks, blocks of one wave"""
    ref = _cached_ref(oracle, ladybug, "persist-ladybug", 96, 80, 24, 64, 1.0)
    it = _integrator(ladybug, 96, 80, 24, 64, 1.0)
    for k, v in opts.items():
        it.set_option(k, v)
    field = it.solve_points(ladybug_grid, 0, 96)
    for c in COUNTERS:
        assert it.last_stats[c] == ref[c], c
    assert np.array_equal(field, ref["field"])
    if opts.get("persist"):
        from elaina_amd import capi
        assert it.last_launches()[0]["kind"] == capi.LAUNCH_PERSISTENT
    it.close()


def test_the_frames_own_points_at_few_samples(ladybug, ladybug_grid):
    """3 spp: the one-launch path of few samples, against solve() of the same handle; seed_width defaults to the frame's"""
    it = _integrator(ladybug, 96, 80, 3, 64, 1.0)
    it.set_option("refill", 1)
    it.solve()
    want, stats = it.solution.copy(), dict(it.last_stats)
    field = it.solve_points(ladybug_grid)
    from elaina_amd import capi
    assert [l["kind"] for l in it.last_launches()][0] == capi.LAUNCH_ONE
    for c in COUNTERS:
        assert it.last_stats[c] == stats[c], c
    assert np.array_equal(field, want)
    it.close()


# ---- 2. / 3. arbitrary points against the oracle; chunks and cuts ---------------------------------------------------------
BOX = dict(spp=8, depth=32, eps=1e-3, seed_base=70, seed_width=16)


def _mixed_box():
    return box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: 1.0 + x + 2.0 * y, flux=lambda x, y, s: 0.3 * (s - 2))


def _box_points():
    pts = np.random.default_rng(7).uniform(-0.25, 1.25, size=(200, 2)).astype(np.float32)
    pts[0] = pts[1] = (0.5, 0.0)      # a mesh vertex, twice: equal coordinates, different streams
    pts[2] = (1.0, 0.5)               # on the Neumann side
    pts[3] = (0.5, 0.5)
    return pts


@pytest.fixture(scope="module")
def box_ref(oracle):
    p = _mixed_box()
    ref = _oracle_points(oracle, "box", p.as_dict(), _box_points(), BOX["seed_base"], BOX["seed_width"], BOX["spp"], BOX["depth"], BOX["eps"])
    # the oracle's answers are what the issue recorded: every point walks, the two equal points differ
    assert np.all(np.any(ref["field"] != 0, axis=1))
    assert int(ref["walk_steps"].sum()) == 26147 and int(ref["walks_truncated"].sum()) == 329
    assert ref["field"][0, 0] != ref["field"][1, 0]
    return ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_arbitrary_points_match_the_oracle(box_ref, n):
    it = _integrator(_mixed_box(), 32, 32, BOX["spp"], BOX["depth"], BOX["eps"])
    field = it.solve_points(_box_points()[:n], BOX["seed_base"], BOX["seed_width"])
    _assert_points(field, it.last_stats, box_ref, slice(0, n))
    it.close()


def test_a_list_longer_than_the_frame_runs_in_chunks(box_ref):
    """an 8 x 8 frame holds 64 walkers: chunks of 64, 64, 64 and 8 points"""
    it = _integrator(_mixed_box(), 8, 8, BOX["spp"], BOX["depth"], BOX["eps"])
    field = it.solve_points(_box_points(), BOX["seed_base"], BOX["seed_width"])
    _assert_points(field, it.last_stats, box_ref)
    launches = [l for l in it.last_launches() if "steps" in l]
    assert len(launches) >= 4
    assert sum(l["steps"] for l in launches) == it.last_stats["walk_steps"]
    assert launches[-1]["walk_steps_done"] == it.last_stats["walk_steps"]
    assert it.last_stats["kernel_launches"] >= 4
    # a cut of the list with seed_base moved along
    part = it.solve_points(_box_points()[70:130], BOX["seed_base"] + 70, BOX["seed_width"])
    _assert_points(part, it.last_stats, box_ref, slice(70, 130))
    it.close()


# ---- 4. far and strayed ----------------------------------------------------------------------------------------------------
def _wiggly_points():
    pts = np.random.default_rng(11).uniform(-150.0, 150.0, size=(64, 2)).astype(np.float32)
    pts[:5] = [(6e4, -2e4), (-5.5e4, 5.5e4), (40.0, 10.0), (5.0, -3.0), (20.0, -3.0)]
    return pts


def test_far_and_strayed_points_match_the_oracle(oracle):
    """two points hundreds of extents away (the wave scan of the init, every walk truncated far outside), points outside the
    Neumann boundary that stray, on the emissive and tree instantiations"""
    p = wiggly_problem(emissive=True)
    pts = _wiggly_points()
    ref = _oracle_points(oracle, "wiggly", p.as_dict(), pts, 0, 16, 4, 16, 0.5)
    # the oracle's answers for the two far points: non-zero and distinct (0.00555788 and 0.001697), every walk truncated
    # (a check of the reference at the precision those figures were printed with; the parity check below is bit for bit)
    assert abs(float(ref["field"][0, 0]) - 0.00555788) < 5e-9 and abs(float(ref["field"][1, 0]) - 0.001697) < 5e-7
    assert ref["field"][0, 0] != ref["field"][1, 0]
    assert ref["walks_truncated"][0] == 4 == ref["walks_truncated"][1]
    it = _integrator(p, 16, 16, 4, 16, 0.5)
    field = it.solve_points(pts, 0, 16)
    _assert_points(field, it.last_stats, ref)
    it.close()


def test_points_with_a_source_term_match_the_oracle(oracle):
    p = _with_source(_mixed_box(), 0.0, 1.0)
    pts = _box_points()[:70]
    ref = _oracle_points(oracle, "box-source", p.as_dict(), pts, 9, 16, BOX["spp"], BOX["depth"], BOX["eps"])
    it = _integrator(p, 32, 32, BOX["spp"], BOX["depth"], BOX["eps"])
    field = it.solve_points(pts, 9, 16)
    _assert_points(field, it.last_stats, ref)
    it.set_option("persist", 1)
    it.set_option("resident_blocks", 1)
    field = it.solve_points(pts, 9, 16)
    _assert_points(field, it.last_stats, ref)
    it.close()


# ---- 5. device arrays, argument checks -------------------------------------------------------------------------------------
def test_device_arrays_on_the_callers_stream(box_ref):
    import torch
    it = _integrator(_mixed_box(), 32, 32, BOX["spp"], BOX["depth"], BOX["eps"])
    pts = torch.from_numpy(_box_points()).cuda()
    field = torch.full((len(pts), 3), -1.0, dtype=torch.float32, device="cuda")
    stats = it.solve_points_dev(pts.data_ptr(), len(pts), field.data_ptr(), torch.cuda.current_stream().cuda_stream, BOX["seed_base"], BOX["seed_width"])
    _assert_points(field.cpu().numpy(), stats, box_ref)
    it.close()


def test_bad_arguments_are_refused_before_any_launch(ladybug):
    from elaina_amd import capi
    it = _integrator(ladybug, 16, 16, 2, 8, 1.0)
    pts = np.zeros((4, 2), np.float32)
    for kw, word in (({"seed_base": -1}, "seed_base"), ({"seed_width": 0}, "seed_width"), ({"seed_base": (1 << 28) - 3}, r"2\^28")):
        with pytest.raises(capi.WostError, match=word):
            it.solve_points(pts, **kw)
    bad = pts.copy()
    bad[2, 1] = np.inf
    with pytest.raises(capi.WostError, match="point 2 "):
        it.solve_points(bad)
    bad[1, 0] = np.nan
    with pytest.raises(capi.WostError, match="point 1 "):
        it.solve_points(bad)
    st = capi.Stats()
    st.walk_steps = 5
    field = np.zeros((4, 3), np.float32)
    assert it.lib.wost_solve_points(it._handle, capi._fp(pts), -1, 0, 16, capi._fp(field), C.byref(st)) == -1
    assert it.lib.wost_solve_points(it._handle, capi._fp(pts), 0, 0, 16, capi._fp(field), C.byref(st)) == 0
    assert st.walk_steps == 0 and st.kernel_launches == 0
    assert it.solve_points(np.zeros((0, 2), np.float32)).shape == (0, 3)
    it.close()


# ---- 3-D -------------------------------------------------------------------------------------------------------------------
def _it3(sd, w, h, spp, depth, eps):
    from elaina_amd import UniformIntegratorSettings
    from elaina_amd.integrator3d import Problem3, UniformIntegrator3
    return UniformIntegrator3(Problem3.from_dict(sd), UniformIntegratorSettings((w, h), spp, depth, eps))


def test_3d_the_frames_own_points_reproduce_the_frame_solve():
    """the tiled frame path against the untiled point path.  Scale 0.5, axis-aligned up and right and a 32 x 32 frame make every
    operation of the evaluation grid exact, so numpy float32 gives the frame's points"""
    sd = sphere_scene3(subdiv=2, value=lambda x, y, z: x + 0.5 * z, probe=(0.5, (0.0, 0.0, 0.25), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)))
    it = _it3(sd, 32, 32, 8, 32, 1e-3)
    it.solve()
    want, stats = it.solution.copy(), dict(it.last_stats)
    py, px = np.divmod(np.arange(32 * 32), 32)
    ndcx, ndcy = (2.0 * px / 32 - 1.0).astype(np.float32), (2.0 * py / 32 - 1.0).astype(np.float32)
    pts = np.stack([np.float32(0.5) * ndcx, np.float32(0.5) * ndcy, np.full(32 * 32, 0.25, np.float32)], 1).astype(np.float32)
    field = it.solve_points(pts, 0, 32)
    for c in COUNTERS:
        assert it.last_stats[c] == stats[c], c
    assert np.any(want != 0) and np.array_equal(field, want)
    it.close()


def _cube_points():
    pts = np.random.default_rng(3).uniform(-0.2, 1.2, size=(130, 3)).astype(np.float32)
    pts[129] = (3e3, 0.0, 0.0)        # beyond huge2: the wave scan at every step
    return pts


@pytest.fixture(scope="module")
def cube_ref(oracle):
    sd = cube_scene3(n=3, d_faces=(0, 1, 4, 5), n_faces=(2, 3), value=lambda x, y, z: x + z)
    return sd, _oracle_points(oracle, "cube3", sd, _cube_points(), 5, 16, 4, 32, 1e-3, dim=3)


@pytest.mark.parametrize("n", [1, 65, 130])
def test_3d_volumetric_points_match_the_oracle(cube_ref, n):
    """points off any slice and partly outside the cube; 130 of them cross two cursor reservations of 64"""
    sd, ref = cube_ref
    it = _it3(sd, 16, 16, 4, 32, 1e-3)
    field = it.solve_points(_cube_points()[:n], 5, 16)
    _assert_points(field, it.last_stats, ref, slice(0, n))
    it.close()


def test_3d_device_arrays_and_bad_arguments(cube_ref):
    import torch
    from elaina_amd import capi
    sd, ref = cube_ref
    it = _it3(sd, 16, 16, 4, 32, 1e-3)
    pts = torch.from_numpy(_cube_points()).cuda()
    field = torch.full((len(pts), 3), -1.0, dtype=torch.float32, device="cuda")
    stats = it.solve_points_dev(pts.data_ptr(), len(pts), field.data_ptr(), torch.cuda.current_stream().cuda_stream, 5, 16)
    _assert_points(field.cpu().numpy(), stats, ref)
    bad = _cube_points()[:3].copy()
    bad[1, 2] = np.nan
    with pytest.raises(capi.WostError, match="point 1 "):
        it.solve_points(bad)
    with pytest.raises(capi.WostError, match="seed_width"):
        it.solve_points(bad[:1], 0, -4)
    it.close()
