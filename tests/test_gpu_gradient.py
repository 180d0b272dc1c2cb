"""The gradient of the solution at the caller's points (wost_solve_gradient_points & co.) against the estimator in numpy on top
of the unchanged oracle (gradient_emulation.py), and against the analytic gradient of linear boundary data.

Tolerances, all derived and none measured: the radius is the oracle's min(dD, 0.875f dN) bit for bit; a first point is
x + R n to 1 ulp of max(|x_k|, R); the five counters equal the emulation's sums exactly; with fp32 sums in any order
|grad - emulated| <= S 2^-23 d / (R (S - 1)) sum_s |n_sk| (|W_s| + |mean|), the field is within S 2^-24 mean|W| and the standard
error within a relative 2 S 2^-23."""
import numpy as np
import pytest

import gradient_emulation as ge
from conftest import box_problem, cube_scene3
from test_gpu_parity import _integrator, _with_source
from test_gpu_points import _it3, _mixed_box

pytestmark = pytest.mark.gpu

ALL = ("stderr", "field", "radius", "first_pts")
BOX = dict(S=8, depth=32, eps=1e-3, seed_base=70, walk_seed_base=3000, seed_width=16)


def _gradient(it, pts, seed_base, walk_seed_base, seed_width):
    out = it.solve_gradient_points(pts, seed_base, walk_seed_base, seed_width, want=ALL)
    assert out["grad"].shape == (len(pts), pts.shape[1], 3) and all(a.dtype == np.float32 for a in out.values())
    return out, dict(it.last_stats)


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("grad",) + ALL)


def _cut(it, pts, at, S, seed_base, walk_seed_base, seed_width):
    """two calls cut at point `at`, both seeds moved with the cut, joined"""
    head, _ = _gradient(it, pts[:at], seed_base, walk_seed_base, seed_width)
    tail, _ = _gradient(it, pts[at:], seed_base + at, walk_seed_base + at * S, seed_width)
    return {k: np.concatenate([head[k], tail[k]]) for k in head}


# ---- 1. blocks and edges, 2-D ----------------------------------------------------------------------------------------------
def _box_points():
    pts = np.random.default_rng(7).uniform(-0.25, 1.25, size=(200, 2)).astype(np.float32)
    pts[0] = (0.5, 0.0)          # on the Dirichlet boundary: degenerate
    pts[1] = (0.5, 0.0005)       # inside the shell: degenerate
    pts[2] = (0.97, 0.5)         # R is set by the Neumann side
    pts[3] = (300.0, -200.0)     # the far query: the scan by the wave
    return pts


def _box_it():
    return _integrator(_mixed_box(), 16, 16, BOX["S"], BOX["depth"], BOX["eps"])


@pytest.mark.parametrize("n", [1, 31, 32, 33, 200])
def test_blocks_and_edges_match_the_emulation(oracle, n):
    """a 16 x 16 frame holds 32 points of 8 walks: a part of a block, one short of it, a block, one more, seven blocks"""
    pts = _box_points()[:n]
    it = _box_it()
    out, stats = _gradient(it, pts, BOX["seed_base"], BOX["walk_seed_base"], BOX["seed_width"])
    it.close()
    emu = ge.emulate(oracle, "box", _mixed_box().as_dict(), pts, out["first_pts"], BOX["seed_base"], BOX["walk_seed_base"], BOX["seed_width"],
                     BOX["depth"], BOX["eps"], 2)
    ge.assert_matches(out, stats, emu, pts)
    assert stats["walks_started"] == n * BOX["S"]
    assert emu["degenerate"][:2].all() and not emu["degenerate"][2:4].any()      # (one of the random points lies in the shell as well)
    if n >= 4:
        assert emu["R"][2] == ge.NEUMANN_SHRINK * emu["dN"][2] < emu["dD"][2]
        assert emu["R"][3] > 200.0 and np.all(np.isfinite(out["grad"][3]))
        # the two degenerate points: NaN gradient (assert_matches) and still the mean of their walks
        assert np.all(np.isfinite(out["field"][:2])) and np.all(out["field"][0] != 0)


def test_a_cut_list_gives_the_same_bits():
    pts = _box_points()
    it = _box_it()
    whole, _ = _gradient(it, pts, BOX["seed_base"], BOX["walk_seed_base"], BOX["seed_width"])
    joined = _cut(it, pts, 77, BOX["S"], BOX["seed_base"], BOX["walk_seed_base"], BOX["seed_width"])
    it.close()
    assert _same_bits(whole, joined)
    # walk_seed_base defaults to seed_base + n, right behind the directions' seeds
    it = _box_it()
    a = it.solve_gradient_points(pts[:40], 70, None, 16)
    b = it.solve_gradient_points(pts[:40], 70, 110, 16)
    it.close()
    assert sorted(a) == ["field", "grad", "radius", "stderr"] and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


# ---- 2. the device form ----------------------------------------------------------------------------------------------------
def test_device_arrays_on_the_callers_stream():
    import torch
    pts = _box_points()[:70]
    n, S = len(pts), BOX["S"]
    it = _box_it()
    host, host_stats = _gradient(it, pts, BOX["seed_base"], BOX["walk_seed_base"], BOX["seed_width"])

    def on_device(p):
        d_pts = torch.from_numpy(p).cuda()
        d = {"grad": (n, 2, 3), "stderr": (n, 2, 3), "field": (n, 3), "radius": (n,), "first_pts": (n, S, 2)}
        d = {k: torch.full(shape, -1.0, dtype=torch.float32, device="cuda") for k, shape in d.items()}
        stats = it.solve_gradient_points_dev(d_pts.data_ptr(), n, d["grad"].data_ptr(), torch.cuda.current_stream().cuda_stream, BOX["seed_base"],
                                             BOX["walk_seed_base"], BOX["seed_width"], stderr_ptr=d["stderr"].data_ptr(),
                                             field_ptr=d["field"].data_ptr(), radius_ptr=d["radius"].data_ptr(), first_pts_ptr=d["first_pts"].data_ptr())
        return {k: v.cpu().numpy() for k, v in d.items()}, stats

    dev, stats = on_device(pts)
    assert _same_bits(host, dev)
    for c in ge.COUNTERS:
        assert stats[c] == host_stats[c], c
    # a NaN coordinate: that point is never walked and answers NaN everywhere; its neighbours keep their bits
    bad = pts.copy()
    bad[37, 1] = np.nan
    dev, stats = on_device(bad)
    assert all(np.all(np.isnan(dev[k][37])) for k in dev)
    rest = np.arange(n) != 37
    assert all(np.array_equal(dev[k][rest], host[k][rest], equal_nan=True) for k in dev)
    assert stats["walks_started"] == (n - 1) * S
    # only grad is required
    d_pts, grad = torch.from_numpy(pts).cuda(), torch.full((n, 2, 3), -1.0, dtype=torch.float32, device="cuda")
    it.solve_gradient_points_dev(d_pts.data_ptr(), n, grad.data_ptr(), None, BOX["seed_base"], BOX["walk_seed_base"], BOX["seed_width"])
    assert np.array_equal(grad.cpu().numpy(), host["grad"], equal_nan=True)
    it.close()


# ---- 3. blocks, 3-D --------------------------------------------------------------------------------------------------------
def _mixed_cube():
    return cube_scene3(n=4, d_faces=(0, 1), n_faces=(2, 3, 4, 5), value=lambda x, y, z: 1.0 + 3.0 * x)


def test_3d_blocks_match_the_emulation_and_a_cut_list_gives_the_same_bits(oracle):
    """100 points in blocks of 32, 32, 32 and 4; one of them hundreds of extents away, where both queries of the kernel in front
    are the scan by the wave: its radius has the bits of the handle's batch closest-point queries"""
    sd = _mixed_cube()
    pts = np.random.default_rng(7).uniform(0.05, 0.95, size=(100, 3)).astype(np.float32)
    pts[3] = (300.0, -200.0, 40.0)
    it = _it3(sd, 16, 16, BOX["S"], BOX["depth"], BOX["eps"])
    out, stats = _gradient(it, pts, BOX["seed_base"], BOX["walk_seed_base"], BOX["seed_width"])
    joined = _cut(it, pts, 41, BOX["S"], BOX["seed_base"], BOX["walk_seed_base"], BOX["seed_width"])
    dD, dN = it.closest_point(pts[3:4])[1][0], it.closest_point(pts[3:4], which=1)[1][0]
    it.close()
    assert dD > 300.0 and out["radius"][3] == min(dD, ge.NEUMANN_SHRINK * dN)
    emu = ge.emulate(oracle, "cube", sd, pts, out["first_pts"], BOX["seed_base"], BOX["walk_seed_base"], BOX["seed_width"], BOX["depth"], BOX["eps"], 3)
    ge.assert_matches(out, stats, emu, pts)
    assert not emu["degenerate"].any() and stats["walks_started"] == 100 * BOX["S"]
    assert _same_bits(out, joined)


# ---- 4. the analytic gradient ------------------------------------------------------------------------------------------------
LIN = dict(S=256, depth=128, eps=1e-3, frame=32, seed_base=5, walk_seed_base=4096, seed_width=64)
ANALYTIC = {
    # the oracle emulation of these very inputs (first points in unfused numpy fp32) gave max |z| / rms ratio:
    "2d-dirichlet": (2, lambda: box_problem(value=lambda x, y: 1.0 + x + 2.0 * y), (1.0, 2.0)),                                           # 3.54 / 0.995
    "2d-mixed": (2, lambda: box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: 1.0 + 2.0 * y, flux=lambda x, y, s: 0.0), (0.0, 2.0)),  # 3.35 / 1.195
    "3d-dirichlet": (3, lambda: cube_scene3(n=4, value=lambda x, y, z: 1.0 + x + 2.0 * y + 3.0 * z), (1.0, 2.0, 3.0)),                    # 2.88 / 1.010
    "3d-mixed": (3, _mixed_cube, (3.0, 0.0, 0.0)),                                                                                        # 3.06 / 1.015
}


@pytest.mark.parametrize("case", sorted(ANALYTIC))
def test_the_gradient_of_linear_boundary_data(oracle, case):
    """u is linear, so grad u is known at every point: the sign and the factor d / R have an anchor outside the emulation, and
    the standard error has to be honest -- every entry within 5 of its own, and the rms of the errors over the rms of the
    standard errors in [0.8, 1.4]"""
    dim, scene, truth = ANALYTIC[case]
    scene = scene()
    if dim == 2:
        pts = np.random.default_rng(3).uniform(0.08, 0.92, size=(64, 2)).astype(np.float32)
        it, sd = _integrator(scene, LIN["frame"], LIN["frame"], LIN["S"], LIN["depth"], LIN["eps"]), scene.as_dict()
    else:
        pts = np.random.default_rng(3).uniform(0.1, 0.9, size=(48, 3)).astype(np.float32)
        it, sd = _it3(scene, LIN["frame"], LIN["frame"], LIN["S"], LIN["depth"], LIN["eps"]), scene
    out, stats = _gradient(it, pts, LIN["seed_base"], LIN["walk_seed_base"], LIN["seed_width"])
    it.close()
    err = out["grad"].astype(np.float64) - np.asarray(truth, np.float64)[None, :, None]
    se = out["stderr"].astype(np.float64)
    z = np.abs(err) / se
    ratio = float(np.sqrt((err ** 2).mean()) / np.sqrt((se ** 2).mean()))
    print("%s: max |z| %.3f, rms ratio %.3f" % (case, float(z.max()), ratio))
    assert np.all(np.abs(err) <= 5.0 * se), float(z.max())
    assert 0.8 <= ratio <= 1.4, ratio
    emu = ge.emulate(oracle, case, sd, pts, out["first_pts"], LIN["seed_base"], LIN["walk_seed_base"], LIN["seed_width"], LIN["depth"], LIN["eps"], dim)
    ge.assert_matches(out, stats, emu, pts)


# ---- 5. refusals that need the handle ----------------------------------------------------------------------------------------
WOST_ERR_INVALID, WOST_ERR_UNSUPPORTED = -1, -3


def _refused(it, word, code, pts, *seeds):
    import ctypes as C
    from elaina_amd import capi
    n, dim = pts.shape
    S = it.settings.samplesPerPixel
    outs = [np.full(k, -1.0, np.float32) for k in (n * dim * 3, n * dim * 3, n * 3, n, n * max(S, 1) * dim)]
    go = capi.GradientOut(*[a.ctypes.data for a in outs])
    fn = getattr(it.lib, it._prefix + "solve_gradient_points")
    assert fn(it._handle, capi._fp(pts), n, *seeds, C.byref(go), None) == code
    assert word in it.lib.wost_last_error().decode(), it.lib.wost_last_error()
    assert all(np.all(a == -1.0) for a in outs)


@pytest.mark.parametrize("dim", [2, 3])
def test_refusals_that_need_the_handle(dim):
    make = (lambda w, h, S: _integrator(_mixed_box(), w, h, S, 8, 1e-3)) if dim == 2 else (lambda w, h, S: _it3(_mixed_cube(), w, h, S, 8, 1e-3))
    pts = np.full((6, dim), 0.5, np.float32)
    it = make(8, 8, 1)
    _refused(it, "spp", WOST_ERR_INVALID, pts, 0, 100, 16)                                    # S = 1
    it.close()
    it = make(8, 8, 65)
    _refused(it, "n_pixels", WOST_ERR_INVALID, pts, 0, 100, 16)                               # S > n_pixels
    it.close()
    it = make(8, 8, 8)
    _refused(it, "overlap", WOST_ERR_INVALID, pts, 0, 5, 16)                                  # [0, 6) and [5, 53)
    _refused(it, "overlap", WOST_ERR_INVALID, pts, 40, 0, 16)                                 # [40, 46) and [0, 48)
    _refused(it, "2^28", WOST_ERR_INVALID, pts, 0, (1 << 28) - 47, 16)                        # ends at 2^28 + 1
    it.close()
    if dim == 2:
        it = _integrator(_with_source(_mixed_box(), 0.0, 1.0), 8, 8, 8, 8, 1e-3)
        _refused(it, "source", WOST_ERR_UNSUPPORTED, pts, 0, 100, 16)
        it.close()


def test_the_walk_seed_bound_is_computed_in_64_bits():
    """n * S = 2^24 * 256 = 2^32 is 0 in 32 bits.  The device form reads no point before it refuses, so a list of 2^24 points
    need not exist"""
    import ctypes as C
    import torch
    from elaina_amd import capi
    it = _integrator(_mixed_box(), 16, 16, 256, 8, 1e-3)
    d_pts = torch.zeros(2, dtype=torch.float32, device="cuda")
    grad = torch.full((8,), -1.0, dtype=torch.float32, device="cuda")
    go = capi.GradientOut(grad.data_ptr(), None, None, None, None)
    rc = it.lib.wost_solve_gradient_points_dev(it._handle, C.c_void_p(d_pts.data_ptr()), 1 << 24, 0, 1 << 24, 16, C.byref(go), None, None)
    assert rc == WOST_ERR_INVALID and "2^28" in it.lib.wost_last_error().decode(), it.lib.wost_last_error()
    assert bool((grad == -1.0).all())
    it.close()


# ---- 6. it leaves the rest alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_a_gradient_call_leaves_the_carried_solves_and_the_frame_solve_alone(dim):
    make = (lambda: _integrator(_mixed_box(), 16, 16, 8, 32, 1e-3)) if dim == 2 else (lambda: _it3(_mixed_cube(), 16, 16, 8, 32, 1e-3))
    pts = np.random.default_rng(5).uniform(0.1, 0.9, size=(40, dim)).astype(np.float32)
    listed = np.random.default_rng(6).uniform(0.1, 0.9, size=(50, dim)).astype(np.float32)

    def run(with_gradient):
        it = make()
        fields = []
        it.solve()
        fields.append(it.solution.copy())
        it.solve_more(3)
        it.points_carry(listed, 9, 16)
        fields.append(it.points_more(2))
        if with_gradient:
            it.solve_gradient_points(pts, 500, 1000, 32)
        it.solve_more(5)
        fields.append(it.solution.copy())
        fields.append(it.points_more(4))
        assert it.spp_done == 8 and it.points_done == 6
        it.solve()
        fields.append(it.solution.copy())
        it.close()
        return fields

    plain, mixed = run(False), run(True)
    assert np.any(plain[0] != 0) and np.array_equal(plain[0], plain[4])
    assert all(np.array_equal(a, b) for a, b in zip(plain, mixed))
