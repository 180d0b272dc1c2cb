"""The gradient at the caller's points on a scene with a source term (the option "grad_source"; include/wost.h "The gradient on a
scene with a source term") against the estimator in numpy on top of the unchanged oracle -- gradient_emulation.py for the walk
part, gradient_source_emulation.py for the in-ball part -- and against the analytic gradient of a Poisson problem.

Tolerances, all derived and none measured: radius, first points and counters as in test_gpu_gradient.py; with fp64 sums in any
order and one rounding, grad within the walk part's bound + 2^-23 (|T| + (R / S) sum |a_s|), field within the walk part's bound +
2^-23 (|U| + (R^2 / S) sum |wu ms|), the standard error within the relative 2 S 2^-23.  Cuts, device forms, the option on a scene
without a source term and the carried list are compared bit for bit."""
import numpy as np
import pytest

import gradient_emulation as ge
import gradient_source_emulation as gs
from conftest import box_problem, cube_scene3
from test_gpu_gradient import ALL, BOX, _box_points, _cut, _gradient, _mixed_cube, _refused, _same_bits
from test_gpu_gradient_carried import _assert_state, _combine, _third, _walkable
from test_gpu_parity import _integrator, _with_source
from test_gpu_points import _it3, _mixed_box

pytestmark = pytest.mark.gpu

WOST_ERR_UNSUPPORTED = -3
SEEDS = (BOX["seed_base"], BOX["walk_seed_base"], BOX["seed_width"])


def _source_box():
    return _with_source(_mixed_box(), 0.0, 1.0)


def _source_cube():
    """the mixed cube with a non-constant source grid of 3 x 4 x 5 nodes over the unit cube"""
    sd = _mixed_cube()
    sd["source"] = {"rgb": np.random.default_rng(11).uniform(-2.0, 3.0, size=(5, 4, 3, 3)).astype(np.float32),
                    "index_scale": (2.0, 3.0, 4.0), "index_offset": (0.0, 0.0, 0.0), "intensity": 0.8}
    return sd


def _cube_points():
    return np.random.default_rng(7).uniform(0.05, 0.95, size=(100, 3)).astype(np.float32)


def _make(dim, source=True, S=BOX["S"], option=1):
    if dim == 2:
        it = _integrator(_source_box() if source else _mixed_box(), 16, 16, S, BOX["depth"], BOX["eps"])
    else:
        it = _it3(_source_cube() if source else _mixed_cube(), 16, 16, S, BOX["depth"], BOX["eps"])
    if option is not None:
        it.set_option("grad_source", option)
    return it


def _assert_matches_the_emulation(oracle, key, sd, pts, out, stats, dim):
    S = out["first_pts"].shape[1]
    emu = ge.emulate(oracle, key, sd, pts, out["first_pts"], *SEEDS, BOX["depth"], BOX["eps"], dim)
    smp = gs.samples(oracle, key, sd, pts, emu["R"], emu["degenerate"], S, BOX["seed_base"], BOX["seed_width"], dim)
    red = gs.reduce(smp, emu["R"])
    ge.assert_matches(out, stats, gs.combine(emu, red), pts)
    ok = ~emu["degenerate"]
    if ok.any():      # the term is there, and it is no rounding error: it moves the answer by far more than the bounds for those
        assert np.any(np.abs(red["T"][ok]) > 10.0 * emu["tol_grad"][ok]) and np.any(np.abs(red["U"][ok]) > 10.0 * emu["tol_field"][ok])
    return emu, red


# ---- 1. blocks and edges, 2-D ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 32, 33, 200])
def test_blocks_and_edges_match_the_emulation(oracle, n):
    """a 16 x 16 frame holds 32 points of 8 walks: a part of a block, a block, one more, seven blocks; the points of
    test_gpu_gradient.py: two degenerate ones, one whose R the Neumann side sets, one far away"""
    pts = _box_points()[:n]
    it = _make(2)
    out, stats = _gradient(it, pts, *SEEDS)
    it.close()
    emu, _ = _assert_matches_the_emulation(oracle, "box-source", _source_box().as_dict(), pts, out, stats, 2)
    assert stats["walks_started"] == n * BOX["S"]
    assert emu["degenerate"][:2].all() and not emu["degenerate"][2:4].any()
    if n >= 4:
        assert emu["R"][2] == ge.NEUMANN_SHRINK * emu["dN"][2] < emu["dD"][2]
        assert emu["R"][3] > 200.0 and np.all(np.isfinite(out["grad"][3]))
        assert np.all(np.isfinite(out["field"][:2]))


def test_both_wave_loops_take_a_second_trip(oracle):
    """72 walks and 72 in-ball samples per point: the lanes of a wave take two each; a 16 x 16 frame holds 3 such points"""
    pts = _box_points()[:7]
    it = _make(2, S=72)
    out, stats = _gradient(it, pts, *SEEDS)
    it.close()
    _assert_matches_the_emulation(oracle, "box-source", _source_box().as_dict(), pts, out, stats, 2)


# ---- 2. blocks, 3-D --------------------------------------------------------------------------------------------------------
def test_3d_blocks_match_the_emulation(oracle):
    """100 points in blocks of 32, 32, 32 and 4"""
    pts = _cube_points()
    it = _make(3)
    out, stats = _gradient(it, pts, *SEEDS)
    it.close()
    emu, _ = _assert_matches_the_emulation(oracle, "cube-source", _source_cube(), pts, out, stats, 3)
    assert not emu["degenerate"].any() and stats["walks_started"] == 100 * BOX["S"]


# ---- 3. the cut list and the device form -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_a_cut_list_gives_the_same_bits(dim):
    pts = _box_points() if dim == 2 else _cube_points()
    it = _make(dim)
    whole, _ = _gradient(it, pts, *SEEDS)
    joined = _cut(it, pts, 77 if dim == 2 else 41, BOX["S"], *SEEDS)
    it.close()
    assert _same_bits(whole, joined)


def test_device_arrays_on_the_callers_stream():
    import torch
    pts = _box_points()[:70]
    n, S = len(pts), BOX["S"]
    it = _make(2)
    host, host_stats = _gradient(it, pts, *SEEDS)

    def on_device(p):
        d_pts = torch.from_numpy(p).cuda()
        d = {"grad": (n, 2, 3), "stderr": (n, 2, 3), "field": (n, 3), "radius": (n,), "first_pts": (n, S, 2)}
        d = {k: torch.full(shape, -1.0, dtype=torch.float32, device="cuda") for k, shape in d.items()}
        stats = it.solve_gradient_points_dev(d_pts.data_ptr(), n, d["grad"].data_ptr(), torch.cuda.current_stream().cuda_stream, *SEEDS,
                                             stderr_ptr=d["stderr"].data_ptr(), field_ptr=d["field"].data_ptr(), radius_ptr=d["radius"].data_ptr(),
                                             first_pts_ptr=d["first_pts"].data_ptr())
        return {k: v.cpu().numpy() for k, v in d.items()}, stats

    dev, stats = on_device(pts)
    assert _same_bits(host, dev)
    for c in ge.COUNTERS:
        assert stats[c] == host_stats[c], c
    # a NaN coordinate: that point is never walked and answers NaN everywhere; its neighbours keep their bits
    bad = pts.copy()
    bad[37, 1] = np.nan
    dev, stats = on_device(bad)
    it.close()
    assert all(np.all(np.isnan(dev[k][37])) for k in dev)
    rest = np.arange(n) != 37
    assert all(np.array_equal(dev[k][rest], host[k][rest], equal_nan=True) for k in dev)
    assert stats["walks_started"] == (n - 1) * S


# ---- 4. nothing moves without the option -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_the_option_changes_nothing_on_a_scene_without_a_source_term(dim):
    pts = _box_points()[:70] if dim == 2 else _cube_points()[:70]
    outs = []
    for option in (None, 1):
        it = _make(dim, source=False, option=option)
        outs.append(_gradient(it, pts, *SEEDS))
        it.close()
    (off, off_stats), (on, on_stats) = outs
    assert _same_bits(off, on) and np.any(np.isfinite(off["grad"]))
    for c in ge.COUNTERS + ("kernel_launches",):
        assert off_stats[c] == on_stats[c], c


@pytest.mark.parametrize("dim", [2, 3])
def test_without_the_option_a_source_scene_is_still_refused(dim):
    from elaina_amd.capi import WostError
    pts = np.full((6, dim), 0.5, np.float32)
    it = _make(dim, option=None)
    _refused(it, "source", WOST_ERR_UNSUPPORTED, pts, 0, 100, 16)
    it.set_option("grad_source", 1)
    assert np.all(np.isfinite(it.solve_gradient_points(pts, 0, 100, 16)["grad"]))
    it.set_option("grad_source", 0)
    _refused(it, "source", WOST_ERR_UNSUPPORTED, pts, 0, 100, 16)
    with pytest.raises(WostError, match=r"\(-3\).*source"):
        it.gradient_points_carry(pts, 8, 6, 2, 0, 100, 16)
    for bad in (0.5, 2, -1, float("nan")):
        with pytest.raises(WostError, match=r"\(-1\).*grad_source"):
            it.set_option("grad_source", bad)
    it.close()


# ---- 5. the carried list ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_a_batch_of_the_carried_list_is_a_row_of_the_single_call(dim):
    """three rounds, the second on a third of the points; the option is switched off after the bind, and the list, which
    recorded it, goes on"""
    n, S, stride = 40, BOX["S"], 64
    pts = _box_points()[:n] if dim == 2 else _cube_points()[:n]
    masks = [None, _third(n), None]
    ref = _make(dim)
    rows = [ref.solve_gradient_points(pts, BOX["seed_base"] + r * stride, BOX["walk_seed_base"] + r * stride * S, BOX["seed_width"]) for r in range(3)]
    ref.close()
    walkable = _walkable(rows[0], BOX["eps"])
    assert walkable.any() and (dim == 3 or not walkable[0])
    it = _make(dim)
    it.gradient_points_carry(pts, S, stride, 3, *SEEDS)
    it.set_option("grad_source", 0)
    for r, m in enumerate(masks):
        out = it.gradient_points_more(m)
        _assert_state(out, _combine(rows[:r + 1], masks[:r + 1], walkable))
        assert it.last_stats["walks_started"] == S * int((walkable if m is None else walkable & (m != 0)).sum())
    assert np.any(out["batches"] == 3) and np.any(out["batches"] == 2) and np.all(np.isfinite(out["grad"][walkable]))
    it.close()


# ---- 6. the analytic anchor ------------------------------------------------------------------------------------------------
# u_c = 1 - a_c x^2 / 2 - b_c x^3 / 6 solves laplace(u) = -(a_c + b_c x) with zero flux across the faces along x.  Channel 0 has
# a = -b / 3: u(0) = u(1) = 1, its Dirichlet data is constant and the variance of its walks comes from the source alone, which
# makes it the channel that sees a missing in-ball term best.  Channel 2 has b = 0.
POISSON = dict(ab=((-2.0, 6.0), (1.0, -1.5), (2.0, 0.0)), S=1024, depth=128, eps=1e-3, frame=32, seed_base=5, walk_seed_base=4096, seed_width=64)


def _poisson_u(x, c):
    a, b = POISSON["ab"][c]
    return 1.0 - a * x * x / 2.0 - b * x * x * x / 6.0


def _poisson_source(dim):
    """f at the nodes x = i / 4 - 1 / 2, i = 0 .. 8: a margin of two cells around the box"""
    x = np.arange(9) / 4.0 - 0.5
    line = np.stack([a + b * x for a, b in POISSON["ab"]], 1).astype(np.float32)
    return {"rgb": np.broadcast_to(line, (9,) * (dim - 1) + (9, 3)).copy(), "index_scale": (4.0,) * dim, "index_offset": (2.0,) * dim, "intensity": 1.0}


def _poisson_colors(verts):
    """per vertex the Dirichlet value of each channel, on both sides of the surface"""
    col = np.stack([_poisson_u(verts[:, 0].astype(np.float64), c) for c in range(3)], 1).astype(np.float32)
    return np.concatenate([col, col], 1)


def _poisson(dim):
    if dim == 2:
        p = box_problem(d_sides=(1, 3), n_sides=(0, 2), value=lambda x, y: 1.0, flux=lambda x, y, s: 0.0)
        p.d_colors = _poisson_colors(p.d_verts)
        p.source = _poisson_source(2)
        pts = np.random.default_rng(3).uniform(0.08, 0.92, size=(64, 2)).astype(np.float32)
        return _integrator(p, POISSON["frame"], POISSON["frame"], POISSON["S"], POISSON["depth"], POISSON["eps"]), pts
    sd = cube_scene3(n=4, d_faces=(0, 1), n_faces=(2, 3, 4, 5), value=lambda x, y, z: 1.0)
    sd["d_colors"] = _poisson_colors(sd["d_verts"])
    sd["source"] = _poisson_source(3)
    pts = np.random.default_rng(3).uniform(0.08, 0.92, size=(48, 3)).astype(np.float32)
    return _it3(sd, POISSON["frame"], POISSON["frame"], POISSON["S"], POISSON["depth"], POISSON["eps"]), pts


@pytest.mark.parametrize("dim", [2, 3])
def test_the_gradient_of_a_poisson_problem(dim):
    """grad u = (-a x - b x^2 / 2, 0[, 0]) at 64 (2-D) and 48 (3-D) points in [0.08, 0.92]^d with 1024 walks each: every entry
    within 5 of its own standard error, rms(error) / rms(stderr) in [0.8, 1.4], and per entry the mean error over the points
    within 4 sqrt(sum_i se_i^2) / n.  The last is what a missing in-ball term would break: dropping T shifts the mean error of
    entry (x, channel c) by mean_i(b_c R_i^2 / 8) in 2-D and / 10 in 3-D, computed below from the returned radii.
    Shift against bound on entry (x, channel 0), b = 6, as the run that wrote this printed them: 2-D 0.04002 against 0.01465, so
    a missing T lies 2.7 bounds out; 3-D 0.02104 against 0.02590, 0.8 bounds -- in 3-D the four Neumann faces keep the balls
    small (the shift falls with R^2, the standard error grows with 1 / R), both scale with b alike, and S = 1024 is all a 32 x 32
    frame takes, so twice the bound is out of reach there: in 3-D the term is pinned by the emulation (test_3d_blocks_match_the_emulation),
    and this case anchors sign and scale of the estimate as a whole."""
    it, pts = _poisson(dim)
    it.set_option("grad_source", 1)
    out, _ = _gradient(it, pts, POISSON["seed_base"], POISSON["walk_seed_base"], POISSON["seed_width"])
    it.close()
    x = pts[:, 0].astype(np.float64)
    truth = np.zeros((len(pts), dim, 3))
    for c, (a, b) in enumerate(POISSON["ab"]):
        truth[:, 0, c] = -a * x - b * x * x / 2.0
    err, se = out["grad"].astype(np.float64) - truth, out["stderr"].astype(np.float64)
    z = np.abs(err) / se
    ratio = float(np.sqrt((err ** 2).mean()) / np.sqrt((se ** 2).mean()))
    mean_err, bound = err.mean(axis=0), 4.0 * np.sqrt((se ** 2).sum(axis=0)) / len(pts)
    R = out["radius"].astype(np.float64)
    shift = np.array([b for _, b in POISSON["ab"]]) * (R * R).mean() / (8.0 if dim == 2 else 10.0)
    print("%d-D: max |z| %.3f, rms ratio %.3f, largest |mean error| / bound %.3f" % (dim, float(z.max()), ratio, float((np.abs(mean_err) / bound).max())))
    print("%d-D: the shift without T on axis x per channel %s, the bound there %s" % (dim, shift, bound[0]))
    assert np.all(np.isfinite(out["grad"])) and np.all(se > 0)
    assert np.all(np.abs(err) <= 5.0 * se), float(z.max())
    assert 0.8 <= ratio <= 1.4, ratio
    assert np.all(np.abs(mean_err) <= bound), (mean_err, bound)
