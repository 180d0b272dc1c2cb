"""Exit lists of the gradient (wost_exits_walk_gradient & co.; include/wost.h "Exit lists of the gradient"): walk once from the
first points of the gradient's estimator, then grad u, its standard error and the mean for any Dirichlet data, and the adjoint.

Every check stands on something outside the code under test: the library's own single call (wost_solve_gradient_points on a
handle made with the colours in question) has to give the very bits apply_gradient gives; the adjoint is compared with the
float64 scatter of exits_gradient_emulation.py within the bound derived there; and a harmonic linear function anchors the whole
against the analytic gradient, with the criterion of tests/test_gpu_gradient.py's own linear anchor.

Scenes, colours, frame (16 x 16), depth, shell and intensity are those of tests/test_gpu_exits.py.

Mutation check (run once on scratch copies of the library, not part of the suite; all 51 cases pass on the library as it is):
nbar left out of the adjoint kernel fails 10 cases -- every case of test_adjoint_against_the_fp64_scatter_and_the_dot_product_identity,
test_vertices_nobody_exits_at_get_exactly_zero, the adjoint part of the analytic anchor and the device forms --, the side offset
flipped in it fails the same without the anchor, whose colours are the same on both sides."""
import ctypes as C

import numpy as np
import pytest

import exits_emulation as xe
import exits_gradient_emulation as xg
import gradient_emulation as ge
from conftest import box_problem, cube_scene3
from test_gpu_exits import BASE, DEPTH, EPS, FRAME, INTENSITY, S, WIDTH, _colors, _make, _points, _same_records, _scene
from test_gpu_gradient import LIN
from test_gpu_points import COUNTERS

pytestmark = pytest.mark.gpu

SEED = 70          # the directions' seeds; BASE (3000) the walks'
ALL = ("stderr", "field", "radius", "first_pts")
WOST_ERR_INVALID, WOST_ERR_UNSUPPORTED = -1, -3


def _colors_of(dim, scene):
    return scene.d_colors if dim == 2 else scene["d_colors"]


def _walk(it, pts, S_=S, seed=SEED, base=BASE, width=WIDTH):
    stats = it.exits_walk_gradient(pts, S_, seed, base, width)
    assert it.exits_done == (len(pts), S_)
    grec = it.exits_gradient_records()
    dim = pts.shape[1]
    assert grec["radius"].shape == (len(pts),) and grec["dirs"].shape == grec["first_pts"].shape == (len(pts), S_, dim)
    assert all(a.dtype == np.float32 for a in grec.values())
    return it.exits_records(), grec, dict(stats)


def _single(it, pts, S_=S, seed=SEED, base=BASE, width=WIDTH):
    out = it.solve_gradient_points(pts, seed, base, width, want=ALL, spp=S_)
    return out, dict(it.last_stats)


def _same_outputs(got, k, want):
    """set k of apply_gradient against a single call's outputs, bit for bit"""
    return all(np.array_equal(got[a][k], want[a], equal_nan=True) for a in ("grad", "stderr", "field"))


# ---- 1. bit for bit against the single call ------------------------------------------------------------------------------------
CASES = [(n, S) for n in (1, 31, 32, 33, 200)] + [(5, s) for s in (2, 64, 65, 130)]


@pytest.mark.parametrize("n,S_", CASES)
@pytest.mark.parametrize("kind", ["mixed", "dirichlet", "cube"])
def test_the_handles_own_colours_give_the_single_call_bit_for_bit(oracle, kind, n, S_):
    """n: a part of a launch of the walks, one point short of one, a launch, one more, seven; S: the smallest, a full wave, one
    past it, two strides and a remainder.  The first points: on the boundary and inside the shell (degenerate), next to the
    Neumann side, the far point"""
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:n]
    it = _make(dim, scene, spp=S_)
    rec, grec, stats = _walk(it, pts, S_)
    got = it.exits_apply_gradient(_colors_of(dim, scene))
    only = it.exits_apply_gradient(_colors_of(dim, scene), want=())
    want, want_stats = _single(it, pts, S_)
    it.exits_walk(grec["first_pts"].reshape(-1, dim), 1, BASE, WIDTH)
    plain = it.exits_records()
    it.close()
    assert np.array_equal(grec["radius"], want["radius"]) and np.array_equal(grec["first_pts"], want["first_pts"])
    assert np.array_equal(grec["dirs"], ge.directions(oracle, n, S_, SEED, WIDTH, dim))
    assert got["grad"].shape == (1, n, dim, 3) and got["field"].shape == (1, n, 3) and set(only) == {"grad"}
    assert _same_outputs(got, 0, want), float(np.nanmax(np.abs(got["grad"][0] - want["grad"])))
    assert np.array_equal(only["grad"], got["grad"], equal_nan=True)
    for c in COUNTERS:
        assert stats[c] == want_stats[c], (c, stats[c], want_stats[c])
    assert stats["walks_started"] == n * S_ and stats["kernel_launches"] == -(-n // (FRAME * FRAME)) + -(-n * S_ // (FRAME * FRAME))
    assert all(np.array_equal(rec[k].reshape(plain[k].shape), plain[k]) for k in rec)
    # the degenerate points are there, walk from themselves and keep their mean
    deg = xg.degenerate(grec["radius"], EPS)
    assert np.array_equal(grec["first_pts"][deg], np.broadcast_to(pts[:, None], grec["first_pts"].shape)[deg])
    assert np.all(np.isnan(got["grad"][0][deg])) and np.all(np.isnan(got["stderr"][0][deg])) and np.all(np.isfinite(got["field"]))
    assert np.all(np.isfinite(got["grad"][0][~deg])) and np.all(np.isfinite(got["stderr"][0][~deg]))
    if n >= 4:
        assert deg[0] and deg[1] and not deg[2] and not deg[3]
    if n == 200:
        assert np.any(got["grad"][0][~deg] != 0) and np.any(rec["prim"] < 0) and np.any(rec["prim"] >= 0)


# ---- 2. other data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_other_data_match_a_fresh_handle_made_with_them(kind):
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:70]
    sets = np.stack([_colors(n_verts, 200 + k) for k in range(3)])
    it = _make(dim, scene)
    _walk(it, pts)
    got = it.exits_apply_gradient(sets)
    ones = [it.exits_apply_gradient(sets[k]) for k in range(3)]
    it.close()
    assert got["grad"].shape == got["stderr"].shape == (3, 70, dim, 3) and got["field"].shape == (3, 70, 3)
    for k in range(3):
        fresh = _make(dim, _scene(kind, sets[k])[1], spp=S)
        want, _ = _single(fresh, pts)
        fresh.close()
        assert _same_outputs(got, k, want), (k, float(np.nanmax(np.abs(got["grad"][k] - want["grad"]))))
        assert all(np.array_equal(ones[k][a][0], got[a][k], equal_nan=True) for a in got)
    assert np.any(got["grad"][0] != got["grad"][1])


# ---- 3. the adjoint --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_", [8, 70])
@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_adjoint_against_the_fp64_scatter_and_the_dot_product_identity(kind, S_):
    """identity: with J c the linear part of grad, evaluated by the emulation in float64 from the list's records,
    <dgrad, J c> = <adjoint(dgrad), c>.  The library's adjoint is within adjoint_bound of the exact scatter entry by entry, and
    the float64 evaluation of the left side carries the same products in its own order (identity_slack): hence
    |lhs - rhs| <= sum |c| (adjoint_bound + identity_slack)"""
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:70]
    K = 2
    dgrad = np.random.default_rng(17).normal(size=(K, len(pts), dim, 3)).astype(np.float32)
    it = _make(dim, scene)
    rec, grec, stats = _walk(it, pts, S_)
    got, again = it.exits_adjoint_gradient(dgrad), it.exits_adjoint_gradient(dgrad)
    one = it.exits_adjoint_gradient(dgrad[1])
    it.close()
    assert got.shape == (K, n_verts, 6) and got.dtype == np.float32
    emu = xg.adjoint(rec, grec, dgrad, prims, n_verts, INTENSITY, EPS, dim)
    bound = xg.adjoint_bound(emu)
    for out in (got, again):
        err = np.abs(out.astype(np.float64) - emu["value"])
        assert np.all(err <= bound), float((err - bound).max())
        assert np.all(out[emu["terms"] == 0] == 0.0)
    print("adjoint: max error / bound %.3f" % float((np.abs(got.astype(np.float64) - emu["value"]) / np.maximum(bound, 1e-300)).max()))
    assert np.all(np.abs(one[0].astype(np.float64) - emu["value"][1]) <= bound[1])
    deg = xg.degenerate(grec["radius"], EPS)
    assert deg.any() and int(emu["terms"].sum()) == int((rec["prim"][~deg] >= 0).sum()) * dim * 3 * K and np.any(emu["terms"] > 1)
    c = np.stack([_colors(n_verts, 300 + k) for k in range(K)]).astype(np.float64)
    lhs = float((dgrad.astype(np.float64) * xg.linear(rec, grec, c, prims, INTENSITY, EPS, dim)).sum())
    rhs = float((got.astype(np.float64) * c).sum())
    tol = float((np.abs(c) * (bound + xg.identity_slack(emu))).sum())
    print("identity: lhs %.9g rhs %.9g, |difference| / tolerance %.3f" % (lhs, rhs, abs(lhs - rhs) / tol))
    assert abs(lhs - rhs) <= tol and abs(lhs) > 1e3 * tol


@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_vertices_nobody_exits_at_get_exactly_zero(kind):
    """two interior points of two walks: at most 4 dim of the entries of a channel can be touched, far fewer than there are"""
    dim, scene, prims, n_verts = _scene(kind)
    pts = np.full((2, dim), 0.5, np.float32)
    pts[1, 0] = 0.25
    dgrad = np.random.default_rng(19).normal(size=(1, 2, dim, 3)).astype(np.float32)
    it = _make(dim, scene, depth=512)
    rec, grec, stats = _walk(it, pts, S_=2)
    got = it.exits_adjoint_gradient(dgrad)
    it.close()
    emu = xg.adjoint(rec, grec, dgrad, prims, n_verts, INTENSITY, EPS, dim)
    assert 4 * dim < n_verts * 2 and stats["walks_absorbed"] >= 2
    assert np.any(emu["terms"] == 0) and np.any(emu["terms"] > 0)
    assert np.all(got[emu["terms"] == 0] == 0.0) and np.any(got[emu["terms"] > 0] != 0.0)
    assert np.all(np.abs(got.astype(np.float64) - emu["value"]) <= xg.adjoint_bound(emu))


@pytest.mark.parametrize("dim", [2, 3])
def test_a_list_of_degenerate_or_unabsorbed_walks_gives_all_zeros(dim):
    """the two degenerate points of the list alone -- their walks are absorbed, and add nothing --, and interior points of a scene
    whose walks all end by truncation (depth 1 from the middle of the domain)"""
    kind = "mixed" if dim == 2 else "cube"
    _, scene, prims, n_verts = _scene(kind)
    dgrad = np.random.default_rng(21).normal(size=(1, 2, dim, 3)).astype(np.float32)
    it = _make(dim, scene)
    rec, grec, stats = _walk(it, _points(dim)[:2])
    assert np.all(xg.degenerate(grec["radius"], EPS)) and stats["walks_absorbed"] > 0
    out = it.exits_adjoint_gradient(dgrad)
    it.close()
    assert np.all(out == 0.0) and not np.any(np.signbit(out))
    it = _make(dim, scene, depth=1)
    pts = np.full((2, dim), 0.5, np.float32)
    pts[1, 0] = 0.45
    rec, grec, stats = _walk(it, pts)
    assert not np.any(xg.degenerate(grec["radius"], EPS)) and stats["walks_absorbed"] == 0 and np.all(rec["prim"] == -1)
    out = it.exits_adjoint_gradient(dgrad)
    it.close()
    assert np.all(out == 0.0)


# ---- 4. the analytic anchor --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_the_analytic_anchor_of_linear_data(dim):
    """u = intensity (a . x + b) is harmonic and linear, so grad u = intensity a at every point.  The criterion is that of
    test_gpu_gradient.test_the_gradient_of_linear_boundary_data, with its S, depth, frame and seeds: every entry within 5 of its
    own standard error, the rms of the errors over the rms of the standard errors in [0.8, 1.4].  The handle is made with other
    colours (the constant 1); the linear ones are an argument.  Then the adjoint: grad(0) is 0 here (no Neumann data, no source:
    every base is 0), and <dgrad, grad(c) - grad(0)> = <adjoint(dgrad), c> up to the roundings of the fp32 results -- 2^-24 of
    each grad entry, the five fp32 roundings of each walk's W weighed by scale |n - nbar| <= 2 scale, 2^-24 of each adjoint entry
    -- and the bound of the adjoint itself"""
    a = np.array([1.0, 2.0, 3.0][:dim])
    if dim == 2:
        scene = box_problem(value=lambda x, y: 1.0)
        scene.dirichlet_intensity = INTENSITY
        verts, prims, n = scene.d_verts, scene.d_segs, 64
        pts = np.random.default_rng(3).uniform(0.08, 0.92, size=(n, 2)).astype(np.float32)
    else:
        scene = cube_scene3(n=4, value=lambda x, y, z: 1.0)
        scene["dirichlet_intensity"] = INTENSITY
        verts, prims, n = scene["d_verts"], scene["d_tris"], 48
        pts = np.random.default_rng(3).uniform(0.1, 0.9, size=(n, 3)).astype(np.float32)
    lin = (np.asarray(verts, np.float64) @ a + 1.0).astype(np.float32)
    sets = np.stack([np.repeat(lin[:, None], 6, axis=1), np.zeros((len(verts), 6), np.float32)])
    it = _make(dim, scene, depth=LIN["depth"], frame=LIN["frame"])
    stats = it.exits_walk_gradient(pts, LIN["S"], LIN["seed_base"], LIN["walk_seed_base"], LIN["seed_width"])
    rec, grec = it.exits_records(), it.exits_gradient_records()
    out = it.exits_apply_gradient(sets)
    dgrad = np.random.default_rng(5).normal(size=(2, n, dim, 3)).astype(np.float32)
    adj = it.exits_adjoint_gradient(dgrad)
    it.close()
    assert stats["walks_started"] == n * LIN["S"] and not np.any(xg.degenerate(grec["radius"], EPS))
    err = out["grad"][0].astype(np.float64) - (INTENSITY * a)[None, :, None]
    se = out["stderr"][0].astype(np.float64)
    z = np.abs(err) / se
    ratio = float(np.sqrt((err ** 2).mean()) / np.sqrt((se ** 2).mean()))
    print("dim %d: max |z| %.3f, rms ratio %.3f" % (dim, float(z.max()), ratio))
    assert np.all(np.abs(err) <= 5.0 * se), float(z.max())
    assert 0.8 <= ratio <= 1.4, ratio
    assert np.all(out["grad"][1] == 0.0) and np.all(rec["base"] == 0.0)
    # the adjoint contracted with the colours (set 0 of dgrad; the zero colours contract to nothing)
    emu = xg.adjoint(rec, grec, dgrad, prims, len(verts), INTENSITY, EPS, dim)
    W = np.abs(xe.walk_values(rec, sets[0], prims, INTENSITY, dim).astype(np.float64)).sum(1)          # (n, 3)
    scale = dim / (grec["radius"].astype(np.float64) * (LIN["S"] - 1))
    d64, c64 = dgrad[0].astype(np.float64), sets[0].astype(np.float64)
    lhs = float((d64 * (out["grad"][0].astype(np.float64) - out["grad"][1])).sum())
    rhs = float((adj[0].astype(np.float64) * c64).sum())
    tol = 2.0 ** -24 * float((np.abs(d64) * (np.abs(out["grad"][0]) + (2.0 * scale[:, None] * 5.0 * W)[:, None, :])).sum()
                             + (np.abs(c64) * np.abs(adj[0])).sum())
    tol += float((np.abs(c64) * (xg.adjoint_bound(emu)[0] + xg.identity_slack(emu)[0])).sum())
    print("dim %d identity: lhs %.9g rhs %.9g, |difference| / tolerance %.3f" % (dim, lhs, rhs, abs(lhs - rhs) / tol))
    assert abs(lhs - rhs) <= tol and abs(lhs) > 1e2 * tol


# ---- 5. behaviour of the list ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_a_cut_list_gives_the_same_rows(kind):
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)
    sets = np.stack([_colors(n_verts, 500 + k) for k in range(2)])
    it = _make(dim, scene)
    rec, grec, _ = _walk(it, pts)
    whole = it.exits_apply_gradient(sets)
    hrec, hgrec, _ = _walk(it, pts[:77])
    head = it.exits_apply_gradient(sets)
    trec, tgrec, _ = _walk(it, pts[77:], seed=SEED + 77, base=BASE + 77 * S)
    tail = it.exits_apply_gradient(sets)
    it.close()
    assert _same_records(rec, hrec, slice(0, 77)) and _same_records(rec, trec, slice(77, None))
    for k in grec:
        assert np.array_equal(grec[k][:77], hgrec[k]) and np.array_equal(grec[k][77:], tgrec[k])
    for k in whole:
        assert np.array_equal(whole[k][:, :77], head[k], equal_nan=True) and np.array_equal(whole[k][:, 77:], tail[k], equal_nan=True)


@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_device_arrays_on_the_callers_stream(kind):
    import torch
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:70]
    n, K = len(pts), 2
    sets = np.stack([_colors(n_verts, 600 + k) for k in range(K)])
    dgrad = np.random.default_rng(29).normal(size=(K, n, dim, 3)).astype(np.float32)
    it = _make(dim, scene)
    host_rec, host_grec, host_stats = _walk(it, pts)
    host = it.exits_apply_gradient(sets)
    emu = xg.adjoint(host_rec, host_grec, dgrad, prims, n_verts, INTENSITY, EPS, dim)
    stream = torch.cuda.current_stream().cuda_stream

    def on_device(p):
        d_pts = torch.from_numpy(p).cuda()
        stats = it.exits_walk_gradient_dev(d_pts.data_ptr(), n, S, stream, SEED, BASE, WIDTH)
        rec, grec = it.exits_records(), it.exits_gradient_records()
        d_sets, d_dgrad = torch.from_numpy(sets).cuda(), torch.from_numpy(dgrad).cuda()
        grad, se = (torch.full((K, n, dim, 3), -1.0, dtype=torch.float32, device="cuda") for _ in range(2))
        field = torch.full((K, n, 3), -1.0, dtype=torch.float32, device="cuda")
        adj = torch.full((K, n_verts, 6), -1.0, dtype=torch.float32, device="cuda")
        it.exits_apply_gradient_dev(d_sets.data_ptr(), K, grad.data_ptr(), stream, se.data_ptr(), field.data_ptr())
        it.exits_adjoint_gradient_dev(d_dgrad.data_ptr(), K, adj.data_ptr(), stream)
        only = torch.full((K, n, dim, 3), -1.0, dtype=torch.float32, device="cuda")
        it.exits_apply_gradient_dev(d_sets.data_ptr(), K, only.data_ptr(), None)
        assert np.array_equal(only.cpu().numpy(), grad.cpu().numpy(), equal_nan=True)
        return rec, grec, stats, {"grad": grad.cpu().numpy(), "stderr": se.cpu().numpy(), "field": field.cpu().numpy()}, adj.cpu().numpy()

    rec, grec, stats, out, adj = on_device(pts)
    assert _same_records(host_rec, rec) and all(np.array_equal(host_grec[k], grec[k]) for k in grec)
    assert all(np.array_equal(out[k], host[k], equal_nan=True) for k in host)
    for c in COUNTERS:
        assert stats[c] == host_stats[c], c
    assert np.all(np.abs(adj.astype(np.float64) - emu["value"]) <= xg.adjoint_bound(emu))
    # a NaN coordinate: that point is never walked, its rows are NaN; its neighbours keep their bits
    bad = pts.copy()
    bad[37, 1] = np.nan
    rec, grec, stats, out, adj = on_device(bad)
    rest = np.arange(n) != 37
    assert np.all(rec["prim"][37] == -1) and np.all(np.isnan(rec["thp"][37])) and np.all(np.isnan(rec["base"][37]))
    assert all(np.all(np.isnan(grec[k][37])) and np.array_equal(grec[k][rest], host_grec[k][rest]) for k in grec)
    assert all(np.all(np.isnan(out[k][:, 37])) and np.array_equal(out[k][:, rest], host[k][:, rest], equal_nan=True) for k in out)
    assert all(np.array_equal(rec[k][rest], host_rec[k][rest]) for k in rec)
    assert stats["walks_started"] == (n - 1) * S
    # (a point that is not walked exits nowhere: the adjoint is that of the list without it, and its dgrad is not read)
    part = xg.adjoint(rec, grec, dgrad, prims, n_verts, INTENSITY, EPS, dim)
    assert np.all(np.isfinite(adj)) and np.all(np.abs(adj.astype(np.float64) - part["value"]) <= xg.adjoint_bound(part))
    it.close()


@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_the_plain_calls_work_on_the_list_and_a_plain_walk_replaces_it(kind):
    """exits_apply and exits_adjoint see the mean of the walks from the first points: what they give on a plain list of those
    very points, one walk each, folded per point"""
    from elaina_amd import capi
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:40]
    sets = np.stack([_colors(n_verts, 900 + k) for k in range(2)])
    v = np.random.default_rng(31).normal(size=(2, len(pts), 3)).astype(np.float32)
    it = _make(dim, scene)
    rec, grec, _ = _walk(it, pts)
    field, se = it.exits_apply(sets, want_stderr=True)
    adj = it.exits_adjoint(v)
    both = it.exits_apply_gradient(sets)
    emu = xe.apply(rec, sets, prims, INTENSITY, dim)
    assert np.all(np.abs(field.astype(np.float64) - emu["mean"]) <= xe.field_bound(emu)) and np.array_equal(field, both["field"], equal_nan=True)
    aemu = xe.adjoint(rec, v, prims, n_verts, INTENSITY, dim)
    assert np.all(np.abs(adj.astype(np.float64) - aemu["value"]) <= xe.adjoint_bound(aemu)) and np.any(adj != 0)
    assert se.shape == field.shape and np.all(se >= 0)
    # a plain walk replaces the list: the gradient calls then refuse, and say which call binds what they need
    it.exits_walk(pts, S, BASE, WIDTH)
    dgrad = np.zeros((1, len(pts), dim, 3), np.float32)
    for call in (lambda: it.exits_apply_gradient(sets), lambda: it.exits_adjoint_gradient(dgrad), it.exits_gradient_records):
        with pytest.raises(capi.WostError, match="wost_exits_walk_gradient"):
            call()
    assert it.exits_done == (len(pts), S) and it.exits_apply(sets).shape == (2, len(pts), 3)
    # ... and a walk of the gradient replaces the plain list
    again, ggrec, _ = _walk(it, pts)
    assert _same_records(rec, again) and all(np.array_equal(grec[k], ggrec[k]) for k in grec)
    it.close()


@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_the_list_and_its_neighbours_leave_one_another_alone(kind):
    """the neighbours test of tests/test_gpu_exits.py with a list of the gradient in place of the plain one, and a carried
    gradient list among the neighbours"""
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:60]
    listed = np.random.default_rng(6).uniform(0.1, 0.9, size=(50, dim)).astype(np.float32)
    sets = np.stack([_colors(n_verts, 700 + k) for k in range(2)])

    def run(with_list):
        it = _make(dim, scene, spp=8)
        out, mine = [], None
        it.solve()
        out.append(it.solution.copy())
        if with_list:
            rec, grec, _ = _walk(it, pts)
            mine = [rec, grec, it.exits_apply_gradient(sets)]
        out.append(it.solve_points(listed, 9, 16))
        it.solve_more(3)
        out.append(it.solution.copy())
        it.points_carry(listed, 9, 16)
        out.append(it.points_more(2))
        g = it.solve_gradient_points(listed[:20], 500, 1000, 32)
        out += [g["grad"], g["field"]]
        it.gradient_points_carry(listed[:20], 4, max_rounds=2, seed_base=600, walk_seed_base=2000, seed_width=32)
        out.append(it.gradient_points_more()["grad"])
        if dim == 2:
            it.set_option("spp", 5)      # (the 3-D handle has no such option)
        it.solve()
        out.append(it.solution.copy())
        it.solve_more(2)
        out.append(it.solution.copy())
        out.append(it.gradient_points_more()["grad"])
        if with_list:
            assert it.exits_done == (len(pts), S)
            assert _same_records(mine[0], it.exits_records()) and all(np.array_equal(mine[1][k], v, equal_nan=True) for k, v in it.exits_gradient_records().items())
            again = it.exits_apply_gradient(sets)
            assert all(np.array_equal(mine[2][k], again[k], equal_nan=True) for k in again)
        it.close()
        return out

    plain, mixed = run(False), run(True)
    assert np.any(plain[0] != 0) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(plain, mixed))


# ---- 6. refusals that need the handle --------------------------------------------------------------------------------------------
def test_a_scene_with_a_source_term_is_refused_whatever_the_option_says():
    from elaina_amd import capi
    dim, scene, prims, n_verts = _scene("source")
    pts = _points(2)[:10]
    it = _make(dim, scene)
    rec = it.exits_walk(pts, S, BASE, WIDTH)      # (the plain list takes such a scene)
    before = it.exits_records()
    for option in (0, 1):
        it.set_option("grad_source", option)
        st = capi.Stats()
        rc = it.lib.wost_exits_walk_gradient(it._handle, capi._fp(pts), len(pts), S, SEED, BASE, WIDTH, C.byref(st))
        assert rc == WOST_ERR_UNSUPPORTED and b"source term" in it.lib.wost_last_error(), it.lib.wost_last_error()
        assert it.exits_done == (len(pts), S) and _same_records(before, it.exits_records())      # the old list stands
    it.close()


def test_the_adjoint_needs_a_dirichlet_mesh():
    """a scene of Neumann sides only: every radius is set by them, the walks end by truncation, apply gives the gradient of the
    bases -- and there are no colours to differentiate by"""
    from elaina_amd import capi
    p = box_problem(d_sides=(), n_sides=(0, 1, 2, 3), flux=lambda x, y, s: 0.5)
    it = _make(2, p, spp=S)
    pts = np.random.default_rng(2).uniform(0.2, 0.8, size=(12, 2)).astype(np.float32)
    rec, grec, stats = _walk(it, pts)
    want, want_stats = _single(it, pts)
    assert np.all(rec["prim"] == -1) and stats["walks_absorbed"] == 0 and np.array_equal(grec["radius"], want["radius"])
    colors = np.zeros(1, np.float32)
    grad, se, field = np.full((1, 12, 2, 3), -1.0, np.float32), np.full((1, 12, 2, 3), -1.0, np.float32), np.full((1, 12, 3), -1.0, np.float32)
    assert it.lib.wost_exits_apply_gradient(it._handle, capi._fp(colors), 1, capi._fp(grad), capi._fp(se), capi._fp(field)) == 0
    assert np.array_equal(grad[0], want["grad"]) and np.array_equal(se[0], want["stderr"]) and np.array_equal(field[0], want["field"])
    out = np.full(6, -1.0, np.float32)
    assert it.lib.wost_exits_adjoint_gradient(it._handle, capi._fp(grad), 1, capi._fp(out)) == WOST_ERR_UNSUPPORTED
    assert b"Dirichlet" in it.lib.wost_last_error() and np.all(out == -1.0)
    it.close()


@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_no_list_and_a_refused_walk(kind):
    from elaina_amd import capi
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:10]
    it = _make(dim, scene)
    sets = _colors(n_verts, 800)[None]
    for call in (lambda: it.exits_apply_gradient(sets), it.exits_gradient_records):
        with pytest.raises(capi.WostError, match="no exit list is bound"):
            call()
    rec, grec, _ = _walk(it, pts)
    out = it.exits_apply_gradient(sets)
    # a refused walk leaves the list as it was
    with pytest.raises(capi.WostError, match="overlap"):
        it.exits_walk_gradient(pts[:3], S, 5, 5, WIDTH)
    bad = pts.copy()
    bad[4, 0] = np.inf
    with pytest.raises(capi.WostError, match="point 4 "):
        it.exits_walk_gradient(bad, S, SEED, BASE, WIDTH)
    again = it.exits_apply_gradient(sets)
    assert it.exits_done == (10, S) and _same_records(rec, it.exits_records()) and all(np.array_equal(out[k], again[k], equal_nan=True) for k in out)
    # n = 0 releases it
    it.exits_walk_gradient(pts[:0], S, SEED, BASE, WIDTH)
    assert it.exits_done == (0, 0)
    with pytest.raises(capi.WostError, match="no exit list is bound"):
        it.exits_apply_gradient(sets)
    it.close()
